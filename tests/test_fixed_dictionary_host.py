"""Argument rules of the fixed-dictionary KL-NMF call (GCCNMF_FLAG_FIXED_W / GCCNMF_FLAG_H_ONES) and the engine's dictionary checks:
all decided before anything reaches a device."""
import numpy as np
import pytest

FIXED_W, H_ONES = 1 << 16, 1 << 17
ERR_ARG, ERR_UNSUPPORTED = 1, 3
P = 4096        # a non-null stand-in pointer: every call below returns before it touches memory


def _lib():
    from gcc_nmf_amd import _hip
    return _hip.lib()


def _klnmf(flags, F=513, N=100, K=128, batch=2):
    return _lib().gccnmf_klnmf(P, P, P, P, F, N, K, batch, 10, 0.0, 1e-16, flags, None)


@pytest.mark.parametrize('extra', [1, 2, 4, 4 | (2 << 8), 1 << 15, 1 << 18])
def test_fixed_w_with_other_bits_is_an_argument_error(extra):
    assert _klnmf(FIXED_W | extra) == ERR_ARG
    assert _klnmf(FIXED_W | H_ONES | extra) == ERR_ARG


def test_h_ones_alone_is_an_argument_error():
    assert _klnmf(H_ONES) == ERR_ARG


@pytest.mark.parametrize('bit', [FIXED_W, H_ONES, FIXED_W | H_ONES])
def test_stage_and_ragged_reject_the_new_bits(bit):
    import ctypes
    lib = _lib()
    assert lib.gccnmf_klnmf_stage(P, P, P, P, 513, 100, 128, 2, 0.0, 1e-16, bit, 1, None) == ERR_ARG
    n = (ctypes.c_int * 2)(100, 80)
    assert lib.gccnmf_klnmf_ragged(P, P, P, P, 513, n, 100, 128, 2, 10, 0.0, 1e-16, bit, None) == ERR_ARG


def test_outside_the_envelope_is_unsupported():
    assert _klnmf(FIXED_W, K=1025) == ERR_UNSUPPORTED
    assert _klnmf(FIXED_W, F=2050) == ERR_UNSUPPORTED


def test_plan_bit_4_only_with_the_flag():
    lib = _lib()
    for F, N, K, B in [(513, 1244, 128, 64), (513, 1244, 1024, 64), (129, 77, 1, 1), (2049, 1, 1024, 3)]:
        assert lib.gccnmf_klnmf_plan(F, N, K, B, FIXED_W) == 16
        assert lib.gccnmf_klnmf_plan(F, N, K, B, FIXED_W | H_ONES) == 16
        plain = lib.gccnmf_klnmf_plan(F, N, K, B, 0)
        assert plain >= 0 and not plain & 16
    assert lib.gccnmf_klnmf_plan(513, 100, 1025, 2, FIXED_W) == -1
    assert lib.gccnmf_klnmf_plan(513, 100, 128, 2, FIXED_W | 1) == -1


def test_engine_rejects_bad_dictionaries():
    from gcc_nmf_amd.engine import check_dictionary
    W = np.random.RandomState(0).rand(513, 64).astype(np.float32)
    assert check_dictionary(W, 513).dtype == np.float32
    with pytest.raises(ValueError):
        check_dictionary(W[:512], 513)
    with pytest.raises(ValueError):
        check_dictionary(W[:, 0], 513)
    with pytest.raises(ValueError):
        check_dictionary(np.zeros((513, 1025), np.float32), 513)
    bad = W.copy()
    bad[3, 4] = -1
    with pytest.raises(ValueError):
        check_dictionary(bad, 513)
    bad[3, 4] = np.nan
    with pytest.raises(ValueError):
        check_dictionary(bad, 513)


# ---- the restatement of the fused launch (tests/fixed_dictionary_restatement.py): its shape table and its bars have teeth ---------------------
import fixed_dictionary_restatement as R          # noqa: E402
import klnmf_stages_restatement as S              # noqa: E402

f32 = np.float32


def test_fixed_shape_is_the_launchers():
    """hand values of csrc/nmf_fixed.hip's fixed_shape: Kb = ceil(K / 32), KB = ceil(Kb / 8), nw = ceil(Kb / KB)"""
    for K, want in ((1, (1, 1, 1)), (32, (1, 1, 1)), (33, (2, 1, 2)), (256, (8, 1, 8)), (257, (9, 2, 5)), (300, (10, 2, 5)), (512, (16, 2, 8)),
                    (513, (17, 3, 6)), (600, (19, 3, 7)), (768, (24, 3, 8)), (769, (25, 4, 7)), (1000, (32, 4, 8)), (1024, (32, 4, 8))):
        assert R.fixed_shape(K) == want
    for K in range(1, 1025):
        Kb, KB, nw = R.fixed_shape(K)
        assert 1 <= KB <= 4 and 1 <= nw <= 8 and (nw - 1) * KB < Kb <= nw * KB and 32 * (Kb - 1) < K <= 32 * Kb
        assert 1 <= R.last_wave_blocks(K) <= KB and 1 <= R.last_block_atoms(K) <= 32


def test_the_shape_table_reaches_every_launch_form():
    shapes = [R.fixed_shape(K) for _, K, _, _ in R.SHAPES]
    assert len(set(R.SHAPES)) == len(R.SHAPES)
    assert {KB for _, KB, _ in shapes} == {1, 2, 3, 4}                                  # every template instance
    assert {nw for _, _, nw in shapes} == set(range(1, 9))                              # every workgroup size
    for KB in (2, 3, 4):                                                                # a partial last wave in each instance that can have one
        assert any(R.fixed_shape(K)[1] == KB and R.last_wave_blocks(K) < KB for _, K, _, _ in R.SHAPES), KB
        assert any(R.fixed_shape(K)[1] == KB and R.last_wave_blocks(K) == KB for _, K, _, _ in R.SHAPES), KB      # ... and a full one
    for KB in (1, 2, 3, 4):
        assert any(R.fixed_shape(K)[1:] == (KB, 8) and K % 32 == 0 for _, K, _, _ in R.SHAPES), KB                  # eight full waves
    # a last block whose lane half 1 holds no atom (K % 32 in 1 .. 4), with and without prefetch
    assert any(R.last_block_atoms(K) <= 4 and R.fixed_shape(K)[1] < 4 for _, K, _, _ in R.SHAPES)
    assert any(R.last_block_atoms(K) <= 4 and R.fixed_shape(K)[1] == 4 for _, K, _, _ in R.SHAPES)
    assert {0, 1, 31} <= {F % 32 for F, _, _, _ in R.SHAPES} and any(F < 32 for F, _, _, _ in R.SHAPES)
    assert any(N % 32 == 0 and N % 64 != 0 for _, _, N, _ in R.SHAPES)                   # a pure padding tile
    assert any(N % 32 not in (0, 1) for _, _, N, _ in R.SHAPES) and any(N > 64 for _, _, N, _ in R.SHAPES)
    assert any(files >= 3 for _, _, _, files in R.SHAPES)
    assert max(F for F, _, _, _ in R.SHAPES) == 513 and all(K * N <= 1024 * 64 for _, K, N, _ in R.SHAPES)      # every case is milliseconds
    # the batch-independence cases: multi-file shapes at KB = 2, 3 and 4
    assert {R.fixed_shape(K)[1] for _, K, _, files in R.SHAPES if files >= 2} >= {2, 3, 4}


def test_the_library_accepts_every_shape_of_the_table():
    lib = _lib()
    for F, K, N, files in R.SHAPES:
        assert lib.gccnmf_klnmf_plan(F, N, K, files, FIXED_W) == 16
        # den [Kp] | Wt [Kp][round_up(F, 32)] ends in front of the status words (the last 32 floats of the workspace)
        Kp, Fq = -(-K // 64) * 64, -(-F // 32) * 32
        assert Kp * (1 + Fq) <= lib.gccnmf_klnmf_workspace_floats(F, N, K, files) - 32


@pytest.mark.parametrize('F,K,N,files', R.SHAPES)
def test_problem_is_what_it_says(F, K, N, files):
    V, W, H0 = R.problem(F, N, K, files)
    Vf, Wf, Hf = R.problem(F, N, K, files, frame=True)
    assert V.dtype == W.dtype == H0.dtype == f32 and V.shape == (files, F, N) and W.shape == (F, K) and H0.shape == (files, K, N)
    assert np.array_equal(W, Wf) and np.array_equal(H0, Hf)
    more = R.problem(F, N, K, files + 2)
    assert np.array_equal(more[0][:files], V) and np.array_equal(more[1], W) and np.array_equal(more[2][:files], H0)      # one pool
    dead = R.dead_atom(K)
    assert (dead is None) == (K < 3) and dead != K - 1
    live = np.ones(K, bool)
    if dead is not None:
        live[dead] = False
        assert not W[:, dead].any()
    assert (W[:, live] > 0).all() and (V >= 0).all() and (H0 >= 0).all()
    for b in range(files):
        f0, n0 = S.zero_lines(F, N, b)
        assert f0 < F - 1 and not V[b, f0].any() and V[b].any(0).all()                  # a silent bin, no silent frame
        assert (n0 is None) == (N < 8)
        if n0 is not None:
            assert n0 < N - 1 and not Vf[b, :, n0].any() and np.count_nonzero(~Vf[b].any(0)) == 1
        zeros = R.h_zeros(K, N, b)
        assert np.count_nonzero(H0[b] == 0) == len(set(zeros)) and all(H0[b, k, n] == 0 for k, n in zeros)
        assert (np.asarray(W, np.float64) @ H0[b] > 0).all()                             # P > 0: every quotient is finite
        # one iteration: the dead atom, the zeros of H0 and (frame=True) the silent frame are exactly 0, everything else positive
        for Vb, frame in ((V[b], None), (Vf[b], n0)):
            ref = R.iteration(Vb, W, H0[b])
            want = H0[b] == 0
            if dead is not None:
                want[dead] = True
            if frame is not None:
                want[:, frame] = True
            assert np.isfinite(ref).all() and np.array_equal(ref == 0, want)
        # three iterations without the silent frame stay finite and positive where they started so
        ref3 = R.iterate(V[b], W, H0[b], S.ALPHA, S.EPS, 3)
        assert np.isfinite(ref3).all() and np.array_equal(ref3 == 0, R.iteration(V[b], W, H0[b]) == 0)


def test_a_silent_frame_divides_zero_by_zero_in_the_second_iteration():
    """why multi-iteration cases take frame=False"""
    F, K, N, files = R.SHAPES[1]
    V, W, H0 = R.problem(F, N, K, 1, frame=True)
    n0 = S.zero_lines(F, N, 0)[1]
    H1 = R.iteration(V[0], W, H0[0])
    assert not H1[:, n0].any()
    with np.errstate(invalid='ignore', divide='ignore'):
        assert np.isnan(R.iteration(V[0], W, H1)[:, n0]).all()


def _emulate(V, W, H, alpha, eps, variant=None):
    """One iteration in float32 NumPy as the launch orders it: K-ordered products, the float32 quotient V / P, an F-ordered sum,
    den = (colsum + alpha) + eps, h * (u / d).  `variant` names one deliberate fault."""
    F, K = W.shape
    N = H.shape[1]
    Kb, KB, nw = R.fixed_shape(K)
    P = np.zeros((F, N), f32)
    for k in range(K - 1 if variant == 'last atom dropped from P' else K):
        P += W[:, k:k + 1] * H[k:k + 1, :]
    if variant == "one wave's block counted twice":
        k0 = 32 * KB * (nw - 1)                                  # the first block of the last wave
        for k in range(k0, min(k0 + 32, K)):
            P += W[:, k:k + 1] * H[k:k + 1, :]
    with np.errstate(divide='ignore', invalid='ignore'):
        Rq = V / P
    U = np.zeros((K, N), f32)
    for f in range(F - 1 if variant == 'last bin dropped from U' else F):
        U += W[f, :, None] * Rq[f:f + 1, :]
    cs = np.zeros(K, f32)
    for f in range(F):
        cs += W[f]
    d = cs + eps if variant == 'den without alpha' else (cs + alpha) + eps
    out = H * (U / d[:, None])
    assert P.dtype == Rq.dtype == U.dtype == d.dtype == out.dtype == f32
    if variant == 'frame N - 1 left unchanged':
        out[:, N - 1] = H[:, N - 1]
    if variant == 'last atom of H taken from the previous atom':
        out[K - 1] = out[K - 2]
    return out, d


VARIANTS = ['last atom dropped from P', 'last bin dropped from U', 'den without alpha', "one wave's block counted twice",
            'frame N - 1 left unchanged', 'last atom of H taken from the previous atom']


@pytest.mark.parametrize('F,K,N,files', R.SHAPES)
def test_float32_numpy_passes_the_bars(F, K, N, files):
    V, W, H0 = R.problem(F, N, K, files)
    Vf = R.problem(F, N, K, files, frame=True)[0]
    worst_h = worst_d = 0.0
    for alpha in (S.ALPHA, f32(0)):
        den, Wt = R.prepare(W, alpha, S.EPS)
        assert Wt.shape == (K, F) and Wt.dtype == f32 and Wt.flags.c_contiguous and np.array_equal(Wt, W.T)
        for Vs in (V, Vf):
            for b in range(files):
                got, d = _emulate(Vs[b], W, H0[b], alpha, S.EPS)
                w, miss = S.share(d, den, R.bar_den(F))
                worst_d = max(worst_d, w)
                assert miss is None, ('den', miss, d[miss], den[miss])
                ref = R.iteration(Vs[b], W, H0[b], alpha, S.EPS)
                w, miss = S.share(got, ref, R.bar_iteration(F, K))
                worst_h = max(worst_h, w)
                assert miss is None, ('H', alpha, b, miss, got[miss], ref[miss])
    print('float32 NumPy, (F, K, N) = (%d, %d, %d): worst share of the bar: den (%.0f * 2^-24) %.3f, H (%.0f * 2^-24) %.3f'
          % (F, K, N, R.bar_den(F) / S.U24, worst_d, R.bar_iteration(F, K) / S.U24, worst_h))
    assert worst_h < 1 and worst_d < 1


def test_the_bars_are_the_stated_counts():
    for F, K, _, _ in R.SHAPES:
        assert R.bar_den(F) == (F + 3) * S.U24 and R.bar_iteration(F, K) == (2 * F + K + 13) * S.U24
        assert R.bar_iteration(F, K) == S.bar_H(F, K) + S.bar_colsum0(F)


@pytest.mark.parametrize('F,K,N,files', R.SHAPES)
def test_every_wrong_variant_misses_the_bar(F, K, N, files):
    V, W, H0 = R.problem(F, N, K, files)
    b = files - 1
    ref = R.iteration(V[b], W, H0[b], S.ALPHA, S.EPS)
    assert S.share(_emulate(V[b], W, H0[b], S.ALPHA, S.EPS)[0], ref, R.bar_iteration(F, K))[1] is None
    assert len(VARIANTS) >= 6
    for variant in VARIANTS:
        if variant == 'last atom of H taken from the previous atom' and K == 1:
            continue                                             # (one atom has no previous one: the other shapes carry this variant)
        got, _ = _emulate(V[b], W, H0[b], S.ALPHA, S.EPS, variant)
        worst, miss = S.share(got, ref, R.bar_iteration(F, K))
        print('(%d, %d, %d) %s: worst share of the bar %.3g, first miss at %s' % (F, K, N, variant, worst, miss))
        assert miss is not None, variant
    assert sum(K > 1 for _, K, _, _ in R.SHAPES) >= len(R.SHAPES) - 1
