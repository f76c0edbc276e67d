"""tests/shared_protocol_restatement.py checked on the host: a float32 NumPy emulation of each call of the shared-dictionary protocol stays
inside every bar and reproduces the bit-for-bit sums at every case shape tests/test_gpu_shared_protocol.py runs (so a correct float32
implementation passes them; the worst shares are printed), six wrong variants of the emulation each miss a check at every multi-file case
(the checks have teeth), the workspace layout written out there adds up to the library's three size functions, and the case table reaches the
launch forms it is there for.

The emulation rounds to float32 after each stage (NumPy float32 arithmetic; its BLAS products and pairwise row sums are one of the orders
the bars allow) and adds the files in ascending order."""
import numpy as np
import pytest

import klnmf_stages_restatement as S
import shared_protocol_restatement as P

f32 = np.float32
IDS = [c.id for c in P.ALL_CASES]


def _copy(st, **over):
    new = dict(st, shards=[dict(sh) for sh in st['shards']])
    new.update(over)
    return new


def emu_begin(st):
    new = _copy(st, colsumW=st['W'].sum(0, dtype=f32), hscale=np.ones(st['W'].shape[1], f32))
    for sh in new['shards']:
        sh['R'] = [np.zeros_like(V) for V in sh['V']]
    return new


def emu_step_a(st, wrong=None):
    """wrong: None | 'file left out' | 'shard overwrites' | 'one column late' | 'hscale ignored in K1' | 'colsumW of another W'"""
    W, s, cs = st['W'], st['hscale'], st['colsumW']
    if wrong == 'colsumW of another W':
        cs = W[:W.shape[0] // 2].sum(0, dtype=f32)              # (the column sums of a W that lacks the upper bins)
    den_k2 = (cs + S.ALPHA + S.EPS)[:, None]
    new, num, den = _copy(st), None, None
    for i, sh in enumerate(new['shards']):
        Vs = sh['V']
        if wrong == 'one column late':                          # the last block of every shard starts one column late in [V0 | V1 | ...]
            N, b = Vs[0].shape[1], len(Vs) - 1
            Vs = Vs[:-1] + [np.roll(np.concatenate(Vs, 1), -1, 1)[:, b * N:(b + 1) * N]]
        sh['H'], sh['R'], sh['U'], sh['rowsum'] = [], [], [], []
        for V, H in zip(Vs, st['shards'][i]['H']):
            Hs = s[:, None] * H
            R1 = V / np.dot(W, H if wrong == 'hscale ignored in K1' else Hs)
            H2 = Hs * np.dot(W.T, R1) / den_k2
            R3 = V / np.dot(W, H2)
            U, rs = np.dot(R3, H2.T), H2.sum(1, dtype=f32)
            assert all(a.dtype == f32 for a in (H2, R3, U, rs))
            sh['H'].append(H2), sh['R'].append(R3), sh['U'].append(U), sh['rowsum'].append(rs)
        parts = (sh['U'][:-1], sh['rowsum'][:-1]) if wrong == 'file left out' and i == 0 else (sh['U'], sh['rowsum'])
        if wrong == 'shard overwrites':
            num = den = None
        num, den = P.file_order_sum(parts[0], num), P.file_order_sum(parts[1], den)
    new['num'], new['den'] = num, den
    return new


def emu_step_b(st):
    Wt = st['W'] * (st['num'] / st['den'])
    s = np.sqrt((Wt * Wt).sum(0, dtype=f32))
    W = Wt / s
    assert W.dtype == f32 and s.dtype == f32
    return _copy(st, W=W, hscale=s, colsumW=W.sum(0, dtype=f32))


def emu_finish(st, wrong=None):
    new = _copy(st, hscale=np.ones_like(st['hscale']))
    files = 0
    for sh in new['shards']:
        sh['H'] = [H * st['hscale'][:, None] if not (wrong and files + b) else H for b, H in enumerate(sh['H'])]
        files += len(sh['H'])
    return new


def _protocol(case):
    """begin, (the lazy scale poked to [0.5, 2), as the GPU test does), step A, step B, finish: the states in between"""
    st0, s = case.problem()
    st1 = emu_begin(st0)
    poked = _copy(st1, hscale=np.array(s))
    return st0, st1, poked


@pytest.mark.parametrize('case', P.ALL_CASES, ids=IDS)
def test_float32_numpy_passes_every_check(case, capsys):
    rep = P.Report(str(case))
    st0, st1, poked = _protocol(case)
    P.check_begin(rep, st0, st1)
    a = emu_step_a(poked)
    P.check_step_a(rep, poked, a)
    b = emu_step_b(a)
    P.check_step_b(rep, a, b)
    if case.iterations == 2:                                     # the second step A meets the real hscale != 1 of the first step B
        a, b = b, emu_step_a(b)
        P.check_step_a(rep, a, b, 'step A (2)')
        a, b = b, emu_step_b(b)
        P.check_step_b(rep, a, b, 'step B (2)')
    P.check_finish(rep, b, emu_finish(b))
    capsys.readouterr()                                          # (the per-check lines: one summary line per case is enough on the host)
    rep.summary('float32 NumPy')
    assert rep.shares and max(rep.shares.values()) < 1


MULTI_FILE = [c for c in P.ALL_CASES if c.files > 1]
STEP_A_WRONG = ['file left out', 'shard overwrites', 'one column late', 'hscale ignored in K1', 'colsumW of another W']


@pytest.mark.parametrize('wrong', STEP_A_WRONG)
@pytest.mark.parametrize('case', MULTI_FILE, ids=[c.id for c in MULTI_FILE])
def test_wrong_variants_of_step_a_miss_a_check(case, wrong, capsys):
    """Each variant at every multi-file case.  'shard overwrites' is a different program only where there is a second shard: at a one-shard
    case it IS the correct emulation (asserted: bit-identical partials), at the others it must miss."""
    _, _, poked = _protocol(case)
    bad = emu_step_a(poked, wrong)
    if wrong == 'shard overwrites' and len(case.spec) == 1:
        good = emu_step_a(poked)
        assert bad['num'].tobytes() == good['num'].tobytes() and bad['den'].tobytes() == good['den'].tobytes()
        return
    with pytest.raises(AssertionError) as e:
        P.check_step_a(P.Report(str(case)), poked, bad)
    capsys.readouterr()
    print('%s: %s: %s' % (case, wrong, str(e.value)[:200]))
    want = 'partial' if wrong in ('file left out', 'shard overwrites') else 'misses its bar'
    assert want in str(e.value)


@pytest.mark.parametrize('case', MULTI_FILE, ids=[c.id for c in MULTI_FILE])
def test_finish_that_scales_file_0_only_misses(case, capsys):
    _, _, poked = _protocol(case)
    a = emu_step_b(emu_step_a(poked))
    P.check_finish(P.Report(str(case)), a, emu_finish(a))
    with pytest.raises(AssertionError) as e:
        P.check_finish(P.Report(str(case)), a, emu_finish(a, wrong=True))
    assert 'not bit for bit' in str(e.value)


def test_lazy_scale_is_recovered_from_h_alone():
    """the run's last hscale is observable only through H: lazy_scale_of finds it bit for bit, and not when one file was scaled differently"""
    case = P.RUN_CASES[0]
    _, _, poked = _protocol(case)
    a = emu_step_b(emu_step_a(poked))
    fin = emu_finish(a)
    was, now = sum((sh['H'] for sh in a['shards']), []), sum((sh['H'] for sh in fin['shards']), [])
    rep = P.Report(str(case))
    s = P.lazy_scale_of(rep, 'hscale', was, now, S.stage5(poked['W'], a['num'], a['den'])[1], S.bar_s(case.F))
    assert s.tobytes() == a['hscale'].tobytes()
    with pytest.raises(AssertionError):
        P.lazy_scale_of(rep, 'hscale', was, now[:-1] + [was[-1]], a['hscale'], S.bar_s(case.F))


def test_layout_totals_are_the_library_size_functions():
    from gcc_nmf_amd import _hip
    lib = _hip.lib()
    seen = set()
    for case in P.ALL_CASES + [P.CROSS_CHECK]:
        assert lib.gccnmf_klnmf_shared_partial_floats(case.F, case.K) == P.partial_floats(case.F, case.K)
        for sh, four in zip(case.shards(), case.shards(vectors=True)):
            assert lib.gccnmf_klnmf_shared_shard_workspace_floats(sh.F, sh.N, sh.K, sh.batch, sh.ld) == sh.floats, str(case)
            if not sh.ld:
                assert lib.gccnmf_klnmf_shared_workspace_floats(sh.F, sh.N, sh.K, sh.batch) == four.floats == sh.floats + 2 * sh.Kp, str(case)
                at, shape = four.blocks['hscale']
                assert at + shape[0] == four.floats and four.blocks['colsumW'][0] == at - sh.Kp      # the two vectors are the workspace's end
            seen.add((sh.single, bool(sh.ld)))
    assert seen == {(True, False), (False, False), (True, True), (False, True)}
    # the workload's own sizes, written out in tests/test_host.py, through the same class
    assert P.Shard(513, 1024, 640, 31, 20032).floats == 528 * 20032 + 31 * (528 * 1024 + 1024)
    assert P.Shard(513, 1024, 1244, 1, 0, vectors=True).floats == lib.gccnmf_klnmf_shared_workspace_floats(513, 1244, 1024, 1)


def test_case_table_reaches_what_it_claims():
    reached = set()
    for case in P.ALL_CASES:
        shards = case.shards()
        for claim, value in case.claims.items():
            if claim == 'direct':
                assert [sh.direct(case.keys) for sh in shards] == [value] * len(shards), str(case)
            elif claim == 'groups':
                assert [sh.groups(case.keys) for sh in shards] == [value], str(case)
                (sh,) = shards
                assert sh.group_files(case.keys)[0][0] == 0 and sh.group_files(case.keys)[-1][1] == sh.batch
            elif claim == 'ld_batch':
                assert any(sh.ld and sh.batch > 1 for sh in shards)
            elif claim == 'ragged_ld':
                assert any(sh.ld and sh.batch == 1 and sh.N % 64 and sh.ld > sh.Np and not sh.single for sh in shards)
            elif claim == 'two_widths':
                assert len({sh.N for sh in shards}) == 2 and not case.ld
            reached.add((claim, value))
    assert reached >= {('direct', True), ('direct', False), ('groups', 1), ('groups', 2), ('groups', 3), ('ld_batch', True), ('ragged_ld', True),
                       ('two_widths', True)}
    # the group rule at its edges: 63 tiles -> 1 group, 64 -> 1, 128 -> 2, 192 -> 3 (key 8), 256 -> 3, 512 -> 1
    assert [P.Shard(145, 20, 64, b).groups() for b in (63, 64, 128, 192, 256, 511, 512)] == [1, 1, 2, 3, 3, 3, 1]
    assert P.Shard(145, 20, 64 * 100, 2).groups() == 2 and P.Shard(145, 20, 1024, 12).groups({8: 4}) == 3
    assert P.Shard(145, 20, 1024, 12).group_files() == [(0, 4), (4, 8), (8, 12)] and P.Shard(145, 20, 512, 16).group_files() == [(0, 8), (8, 16)]


@pytest.mark.parametrize('case', P.ALL_CASES + [P.CROSS_CHECK], ids=[c.id for c in P.ALL_CASES + [P.CROSS_CHECK]])
def test_every_case_keeps_the_silent_bin_unless_one_file_runs_twice(case):
    """Every file of every case has its silent bin -- the run's column blocks, ragged remainder, shard-order sums and file groups meet an
    exactly-zero row of V, R and Upart -- and, the files' bins being different rows, the shared W keeps every row after step B.  The one
    case without: a single file in total that runs a second iteration, where W's row WOULD become exactly 0 (shown here on the same
    problem with the bin put back) and the second step A 0 / 0."""
    _, _, poked = _protocol(case)
    one_file_twice = case.files == 1 and case.iterations == 2
    assert one_file_twice == (case.name == 'one column block of pitch Np')
    for sh, (N, batch, _) in zip(poked['shards'], case.spec):
        for b, V in enumerate(sh['V']):
            assert (not V[S.zero_lines(case.F, N, b)[0]].any()) == (not one_file_twice) and (V > 0).any(0).all()
    if case.files > 1 and case.iterations == 2:
        W = emu_step_b(emu_step_a(poked))['W']
        assert (W > 0).any(1).all() and np.isfinite(W).all()
        assert len({S.zero_lines(case.F, N, b)[0] for N, batch, _ in case.spec for b in range(batch)}) > 1
    elif one_file_twice:
        (N, _, _), = case.spec
        f0 = S.zero_lines(case.F, N, 0)[0]
        V = np.array(poked['shards'][0]['V'][0])
        V[f0] = 0
        with_bin = _copy(poked, shards=[dict(poked['shards'][0], V=[V])])
        after = emu_step_b(emu_step_a(with_bin))
        assert not after['W'][f0].any()
        with np.errstate(invalid='ignore'):
            assert np.isnan(emu_step_a(after)['shards'][0]['H'][0]).all()


def test_problem_without_the_silent_frame_keeps_the_silent_bin():
    F, N, K = 513, 70, 65
    with_frame, without = S.problem(F, N, K, 2), S.problem(F, N, K, 2, frames=False)
    for b in range(2):
        f0, n0 = S.zero_lines(F, N, b)
        assert not without[0][b, f0].any() and without[0][b, :, n0].any() and not with_frame[0][b, :, n0].any()
        assert (without[0][b] > 0).sum(0).min() > 0                                        # no column of V is all zero
        rest = np.arange(N) != n0
        assert np.array_equal(without[0][b][:, rest], with_frame[0][b][:, rest])
    for a, c in zip(with_frame[1:], without[1:]):
        assert np.array_equal(a, c)
