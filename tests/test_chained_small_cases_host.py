"""tests/chained_small_cases.py checked without a device: gccnmf_klnmf_plan, gccnmf_set_tuning and the workspace-size functions are host code, so
every call of the table is shown here to take the launch form tests/test_gpu_chained_small_shapes.py means it to take, and the table to reach
every form it claims.  A later change to plan_klnmf that moves a case off the chain fails here, on any machine."""
import contextlib

import numpy as np
import pytest

import chained_small_cases as C
import klnmf_stages_restatement as S


def _lib():
    from gcc_nmf_amd import _hip
    return _hip.lib()


@contextlib.contextmanager
def _tuning(*keys):
    lib, merged = _lib(), {}
    for k in keys:
        merged.update(k)
    assert set(merged) <= set(C.DEFAULTS) and not set(merged) & {22, 25}
    try:
        for k, v in merged.items():
            assert lib.gccnmf_set_tuning(k, v) == 0, 'gccnmf_set_tuning(%d, %d) was refused: a product key, which every build accepts' % (k, v)
        yield lib
    finally:
        for k in merged:
            lib.gccnmf_set_tuning(k, C.DEFAULTS[k])


def _plan(case, call, base):
    with _tuning(base, call.keys) as lib:
        return lib.gccnmf_klnmf_plan(case.F, case.N, case.K, case.B, 0)


def _workspace_ok(lib, F, N, K, B):
    """Positive and whole 128-byte lines.  (Every block in front of the ready counters is a multiple of 64 floats; the counters are rounded up to 32
    words and 32 status words follow -- csrc/nmf.hip: carve; tests/test_host.py pins the sizes exactly -- so 32 floats is what holds at every
    shape, e.g. (257, 32, 256) x 9: 790368 = 64 * 12349 + 32.)"""
    n = lib.gccnmf_klnmf_workspace_floats(F, N, K, B)
    assert n > 0 and n % 32 == 0, 'workspace of (%d, %d, %d) x %d: %d floats' % (F, N, K, B, n)


def test_the_defaults_are_the_library_s():
    """every key a case sets is a product key, and DEFAULTS restores what the library starts with: the plan of a workload shape under DEFAULTS is
    the plan of an untouched library"""
    lib = _lib()
    shapes = [(513, 1244, 1024, 64), (513, 1244, 128, 64), (513, 1244, 1024, 16), (513, 200, 64, 2), (257, 130, 256, 9)]
    before = [lib.gccnmf_klnmf_plan(F, N, K, B, 0) for F, N, K, B in shapes]
    assert before[:2] == [C.CHAINED, C.K1K2 | C.K3K4A | C.CHAINED]
    with _tuning(C.DEFAULTS):
        assert [lib.gccnmf_klnmf_plan(F, N, K, B, 0) for F, N, K, B in shapes] == before
    assert [lib.gccnmf_klnmf_plan(F, N, K, B, 0) for F, N, K, B in shapes] == before
    assert lib.gccnmf_set_tuning(21, 3) != 0 and lib.gccnmf_set_tuning(23, 4) != 0 and lib.gccnmf_set_tuning(24, 0) != 0


# ---- B -----------------------------------------------------------------------------------------------------------------------------------------------
def test_throughput_chain_plans():
    cases = C.throughput_cases()
    assert len(cases) == len(C.THROUGHPUT_FK) * len(C.THROUGHPUT_N)
    for case in cases:
        assert case.K >= 256 and case.K % 128 == 0 and case.F in (257, 385, 513)
        for call in case.calls:
            plan = _plan(case, call, C.THROUGHPUT_KEYS)
            assert plan & 15 == call.plan, '%s %s: gccnmf_klnmf_plan says %d' % (case[:6], call.name, plan)
            assert call.compared == bool(plan & C.CHAINED)
        # where the forced form is not available the case says so and is not compared -- it is never silently dropped
        lists0 = [c for c in case.calls if c.keys.get(23) == 0]
        assert len(lists0) == 1 and lists0[0].compared == (case.B % 8 == 0)
        assert case.calls[0] == C.PLAIN and sum(c.keys == {21: 8} for c in case.calls) == 2
        with _tuning(C.THROUGHPUT_KEYS) as lib:
            _workspace_ok(lib, case.F, case.N, case.K, case.B)


def test_throughput_chain_cases_reach_every_form():
    cases = C.throughput_cases()
    calls_per_shape = {fk: sum(len(c.calls) for c in cases if (c.F, c.K) == fk) for fk in C.THROUGHPUT_FK}
    print('calls per (F, K):', calls_per_shape)
    assert all(32 <= n <= 56 for n in calls_per_shape.values())                     # "about 40"
    for fk in C.THROUGHPUT_FK:
        mine = [c for c in cases if (c.F, c.K) == fk]
        assert sorted(c.N for c in mine) == C.THROUGHPUT_N and {c.B for c in mine} == set(C.THROUGHPUT_B)
        assert {c.iterations for c in mine} == {1, 5} and sum(c.oracle for c in mine) == 1
        assert all(c.iterations == 5 and c.N >= 97 for c in mine if c.oracle)
    for N in C.THROUGHPUT_N:
        reached = set()
        for c in cases:
            if c.N == N:
                reached |= {(call.keys[21], call.keys.get(23, 1)) for call in c.calls if call.compared}
        assert reached == set(C.CHAIN_PAIRS), (N, reached)
    for B in C.THROUGHPUT_B:
        assert {c.iterations for c in cases if c.B == B} == {1, 5}
    assert {C.n_class(N) for N in C.THROUGHPUT_N} == {(1, '1'), (1, 'narrow'), (1, 'wide'), (1, 'full'), (2, '1'), (2, 'narrow'), (2, 'wide'), (3, 'narrow')}
    chunks = {call.keys[24] for c in cases for call in c.calls if 24 in call.keys}
    assert chunks == {1, 3} and all(c.iterations == 5 for c in cases for call in c.calls if 24 in call.keys)
    assert [c.alpha for c in cases].count(0.2) == len(C.THROUGHPUT_FK) and all(c.alpha == 0.2 for c in cases if c.N == 65)
    # the list forms by rule (chain_list_mode: whole files when 1000 * 8 * ceil(B / 8) <= 1027 * B)
    assert [1000 * 8 * -(-B // 8) <= 1027 * B for B in C.THROUGHPUT_B] == [True, False, False, True, True]


# ---- C -----------------------------------------------------------------------------------------------------------------------------------------------
def test_short_chain_plans():
    for case in C.short_cases():
        Kp = -(-case.K // 64) * 64
        assert case.B >= 8 and case.B * Kp // 64 < 256 and case.K <= 128
        for call in case.calls:
            plan = _plan(case, call, C.SHORT_KEYS)
            assert plan & 15 == call.plan, '%s %s: gccnmf_klnmf_plan says %d' % (case[:6], call.name, plan)
        refused = (case.F, case.N, case.K, case.B) == C.SHORT_REFUSED
        assert all(bool(call.plan & C.CHAINED) == (call.compared and not refused) for call in case.calls)
        with _tuning(C.SHORT_KEYS) as lib:
            _workspace_ok(lib, case.F, case.N, case.K, case.B)


def test_short_chain_cases_reach_all_eight_instantiations():
    cases = C.short_cases()
    for iterations in (1, 4):
        reached = {(c.KB, c.group) for c in cases if c.group and c.iterations == iterations}
        assert reached == {(kb, g) for kb in (1, 2, 3, 4) for g in (16, 32)}
    table = {(c.F, c.N, c.K, c.B): (c.KB, c.group) for c in cases}
    assert table == {(129, 65, 20, 8): (1, 16), (129, 65, 20, 130): (1, 32), (257, 64, 33, 13): (2, 16), (257, 64, 33, 128): (2, 32),
                     (385, 130, 96, 24): (3, 16), (385, 130, 96, 64): (3, 32), (385, 1, 65, 9): (3, 16), (513, 130, 128, 9): (4, 16),
                     (513, 130, 128, 70): (4, 32), (513, 1, 100, 8): (4, 16), C.SHORT_REFUSED: (2, 0)}
    assert {call.keys.get(24, 2048) for c in cases for call in c.calls} == {2048, 1}
    assert sum(c.alpha == 0.2 for c in cases) == 2 and {c.iterations for c in cases if c.alpha == 0.2} == {1, 4}


# ---- D -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,K', C.RAGGED_FK)
@pytest.mark.parametrize('lengths', C.RAGGED_LENGTHS, ids=['16 files', '9 files'])
def test_ragged_cases(F, K, lengths):
    B, Nmax = len(lengths), C.RAGGED_NMAX
    assert max(lengths) == Nmax and {C.n_class(n) for n in lengths} == {C.n_class(n) for n in C.THROUGHPUT_N}
    lists = C.ragged_lists(lengths)
    assert sorted(f for l in lists for f in l) == list(range(B)) and all(l for l in lists)
    if B == 16:
        assert sorted(lengths) == sorted(2 * C.THROUGHPUT_N)
        # every list holds two files of different lengths, and in some lists one file's last tile is narrow and the other's is not
        assert all(len(l) == 2 and lengths[l[0]] != lengths[l[1]] for l in lists)
        assert any(len({C.n_class(lengths[f])[1] in ('1', 'narrow') and lengths[f] > 64 for f in l}) == 2 for l in lists)
    else:
        assert sorted(len(l) for l in lists) == [1] * 7 + [2]
    with _tuning(C.RAGGED_KEYS) as lib:
        # the ragged call asks chain_capable alone; of gccnmf_klnmf_plan it takes the direct bit (clear) for stages 0 and 6
        assert lib.gccnmf_klnmf_plan(F, Nmax, K, B, 0) & C.DIRECT == 0
        n = lib.gccnmf_klnmf_ragged_workspace_floats(F, Nmax, K, B)
        assert n > 0 and n % 4 == 0 and n > lib.gccnmf_klnmf_workspace_floats(F, Nmax, K, B)
    with _tuning(C.RAGGED_KEYS, {21: 0}) as lib:
        for n in set(lengths):
            files = max(lengths.count(n), 1)
            assert lib.gccnmf_klnmf_plan(F, n, K, files, 0) & 15 == 0            # the reference batch: the four plain throughput-tile launches
            _workspace_ok(lib, F, n, K, files)


# ---- the problems ---------------------------------------------------------------------------------------------------------------------------------------
def _klnmf_float64(V, W, H, iterations, alpha):
    V, W, H = (np.array(a, np.float64) for a in (V, W, H))
    with np.errstate(invalid='ignore', divide='ignore'):
        for _ in range(iterations):
            H *= np.dot(W.T, V / np.dot(W, H)) / (np.sum(W, axis=0)[:, np.newaxis] + alpha + C.EPS)
            W *= np.dot(V / np.dot(W, H), H.T) / np.sum(H, axis=1)
            norms = np.sqrt(np.sum(W ** 2, 0))
            W /= norms
            H *= norms[:, np.newaxis]
    return W, H


def test_a_silent_bin_does_not_survive_a_second_iteration():
    """Why only the one-iteration calls keep the silent bin: after one iteration its row of W is exactly 0 and everything else finite; after two,
    the reference algorithm in float64 is NaN throughout."""
    F, N, K = 257, 33, 256
    V, W, H = (a[0] for a in C.problem(F, N, K, 2, 1))
    f0 = S.zero_lines(F, N, 0)[0]
    assert not V[f0].any() and V.any(axis=0).all()
    W1, H1 = _klnmf_float64(V, W, H, 1, 0.0)
    assert not W1[f0].any() and np.isfinite(W1).all() and np.isfinite(H1).all() and np.delete(W1, f0, 0).all()
    W2, H2 = _klnmf_float64(V, W, H, 2, 0.0)
    assert np.isnan(W2).all() and np.isnan(H2).all()


@pytest.mark.parametrize('F,N,K', [(257, 1, 256), (385, 33, 384), (513, 130, 128)])
def test_problems_of_several_iterations_stay_finite(F, N, K):
    """... and what those calls get instead: isolated exact zeros, no zero row or column, finite positive factors after 5 iterations in float64"""
    V, W, H = C.problem(F, N, K, 2, 5)
    for b in range(2):
        assert np.count_nonzero(V[b] == 0) >= (5 if N > 1 else 0) and V[b].any(axis=1).all() and V[b].any(axis=0).all()
        Wn, Hn = _klnmf_float64(V[b], W[b], H[b], 5, 0.0)
        assert np.isfinite(Wn).all() and np.isfinite(Hn).all() and (Wn > 0).all()
    assert not np.array_equal(W[0], W[1]) and not np.array_equal(H[0], H[1]) and not np.array_equal(V[0], V[1])
    files, by_length = C.ragged_problem(F, K, [N, 7, N])
    assert list(by_length.items()) == [(N, [0, 2]), (7, [1])] and files[1][0].shape == (F, 7) and files[2][2].shape == (K, N)
    assert np.array_equal(files[0][0], V[0]) and np.array_equal(files[2][1], W[1])


def test_oracle_factors_are_the_oracle_s():
    from oracle import gccnmf_oracle as O
    for seed in (0, 7):
        W, H = C.oracle_factors(257, 33, 256, seed)
        Wo, Ho = O.initKLNMF(257, 33, 256, C.EPS, seed)
        assert W.dtype == H.dtype == np.float32 and np.array_equal(W, Wo) and np.array_equal(H, Ho)
    case = [c for c in C.throughput_cases() if c.oracle][0]
    V, W, H = C.throughput_problem(case)
    assert np.array_equal(W[case.B - 1], C.oracle_factors(case.F, case.N, case.K, case.B - 1)[0]) and V.shape == (case.B, case.F, case.N)
