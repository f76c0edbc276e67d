"""tests/klnmf_stages_restatement.py checked on the host: its stages chained are the reference's algorithm, a plain float32 NumPy evaluation
of every stage stays inside the bars at every shape tests/test_gpu_klnmf_stages.py uses (so a correct float32 implementation passes them;
the share of each bar it uses is printed), and the exact zeros a silent bin and a silent frame of V must produce are in the restatement."""
import numpy as np
import pytest

import klnmf_stages_restatement as S

f32 = np.float32


def _performKLNMF_float64(V, W, H, iterations, alpha, eps):
    """oracle.gccnmf_oracle.performKLNMF's loop, line by line, in float64 from the given initial factors."""
    V, W, H = (np.array(a, np.float64) for a in (V, W, H))
    for _ in range(iterations):
        H *= np.dot(W.T, V / np.dot(W, H)) / (np.sum(W, axis=0)[:, np.newaxis] + alpha + eps)
        W *= np.dot(V / np.dot(W, H), H.T) / np.sum(H, axis=1)
        norms = np.sqrt(np.sum(W ** 2, 0))
        W /= norms
        H *= norms[:, np.newaxis]
    return W, H


@pytest.mark.parametrize('F,N,K', [(70, 50, 12), (145, 33, 65)])
def test_chained_stages_are_the_reference_algorithm(F, N, K):
    V, W, H, _ = (a[0] for a in S.problem(F, N, K, 1, lines=False))
    alpha, eps = float(S.ALPHA), float(S.EPS)
    want_W, want_H = _performKLNMF_float64(V, W, H, 4, alpha, eps)
    W, H = np.array(W, np.float64), np.array(H, np.float64)
    colsumW, s = S.stage0(W)
    for _ in range(4):
        R = S.stage1(V, W, H, s)
        H = S.stage2(W, H, s, R, colsumW, alpha, eps)
        R = S.stage3(V, W, H)
        U, rowsumH = S.stage4(R, H)
        W, s, colsumW = S.stage5(W, U, rowsumH)
    H = S.stage6(H, s, np.float64)
    dW, dH = np.abs(W / want_W - 1).max(), np.abs(H / want_H - 1).max()
    print('chained stages against performKLNMF in float64, (%d, %d, %d): W %.3g, H %.3g relative' % (F, N, K, dW, dH))
    assert dW < 1e-12 and dH < 1e-12


def test_throughput_cases_cover_every_knob_with_every_shape():
    """Key 9 acts on the LDS-DMA launcher only: its four values are required among the key 3 = 1 cases of each shape."""
    cases = S.throughput_cases()
    assert len(set(cases)) == len(cases) == 5 * len(S.THROUGHPUT_SHAPES)
    for shape in S.THROUGHPUT_SHAPES:
        mine = [c[3:] for c in cases if c[:3] == shape]
        assert sorted(split for _, _, dma, split in mine if dma == 1) == [0, 1, 2, 3]
        assert [dma for _, _, dma, _ in mine].count(0) == 1
        assert {B for B, _, _, _ in mine} == {2, 9} and {flags for _, flags, _, _ in mine} == {0, S.NO_XCD_AFFINITY, S.UNFUSED_W_UPDATE}
        assert any(flags == 0 and dma == 1 for _, flags, dma, _ in mine)            # the default form of a batch at scale


def _within(what, got, ref, bar, shares):
    worst, miss = S.share(got, ref, bar)
    shares[what] = max(shares.get(what, 0.0), worst)
    assert miss is None, '%s: element %s is %r, reference %r, bar %.3g relative' % (what, miss, got[miss], ref[miss], bar)


@pytest.mark.parametrize('F,N,K', S.ALL_SHAPES)
def test_float32_numpy_passes_every_bar(F, N, K):
    """Each stage in float32 NumPy from the float32 state before it, the order the GPU helper follows (the silent frame's column of H is
    restored after stage 2, as there)."""
    shares = {}
    for b, (V, W, H, s) in enumerate(zip(*S.problem(F, N, K, 2))):
        n0 = S.zero_lines(F, N, b)[1]
        alpha, eps = S.ALPHA, S.EPS
        cs = W.sum(0, dtype=f32)
        _within('0 colsumW', cs, S.stage0(W)[0], S.bar_colsum0(F), shares)
        R = V / np.dot(W, s[:, None] * H)
        assert R.dtype == f32
        _within('1 R', R, S.stage1(V, W, H, s), S.bar_R(K), shares)
        H2 = (s[:, None] * H) * np.dot(W.T, R) / (cs + alpha + eps)[:, None]
        assert H2.dtype == f32
        _within('2 H', H2, S.stage2(W, H, s, R, cs), S.bar_H(F), shares)
        _within('1 H (K1 + K2 fused)', H2, S.fused12(V, W, H, s, cs), S.bar_H(F, K), shares)
        if n0 is not None:
            assert not H2[:, n0].any()
            H2[:, n0] = H[:, n0]
        R3 = V / np.dot(W, H2)
        _within('3 R', R3, S.stage3(V, W, H2), S.bar_R(K), shares)
        U, rs = np.dot(R3, H2.T), H2.sum(1, dtype=f32)
        assert U.dtype == f32
        _within('4 U', U, S.stage4(R3, H2)[0], S.bar_U(N), shares)
        _within('4 rowsumH', rs, S.stage4(R3, H2)[1], S.bar_rowsumH(N), shares)
        _within('3 U (K3 + K4a fused)', U, S.fused34(V, W, H2)[0], S.bar_U(N, K), shares)
        Wt = W * (U / rs)
        s5 = np.sqrt((Wt * Wt).sum(0, dtype=f32))
        W5 = Wt / s5
        cs5 = W5.sum(0, dtype=f32)
        assert W5.dtype == f32 and s5.dtype == f32
        for tag, ref, n in (('5', S.stage5(W, U, rs), None), ('4 (W update fused)', S.fused_w(W, R3, H2), N)):
            _within(tag + ' W', W5, ref[0], S.bar_W(F, n), shares)
            _within(tag + ' s', s5, ref[1], S.bar_s(F, n), shares)
            _within(tag + ' colsumW', cs5, ref[2], S.bar_colsumW(F, n), shares)
        assert S.stage6(H2, s5).tobytes() == (H2 * s5[:, None]).tobytes()
    print('float32 NumPy, (%d, %d, %d), largest share of each bar: ' % (F, N, K) + ', '.join('%s %.3f' % kv for kv in sorted(shares.items())))
    assert max(shares.values()) < 1


@pytest.mark.parametrize('F,N,K', [(513, 70, 65), (40, 65, 17)])
def test_exact_zeros_of_a_silent_bin_and_a_silent_frame(F, N, K):
    for b, (V, W, H, s) in enumerate(zip(*S.problem(F, N, K, 2))):
        f0, n0 = S.zero_lines(F, N, b)
        assert f0 < F - 1 and n0 < N - 1 and not V[f0].any() and not V[:, n0].any()
        assert np.count_nonzero(V == 0) > F + N - 1                   # ... and isolated zeros beside them
        cs, _ = S.stage0(W)
        R = S.stage1(V, W, H, s)
        assert not R[f0].any() and not R[:, n0].any() and np.isfinite(R).all()
        H2 = S.stage2(W, H, s, R, cs)
        assert not H2[:, n0].any() and np.count_nonzero(H2 == 0) == K
        # (stage 3 on this H2 divides 0 by 0 in the silent frame -- as the reference does; the helpers restore the column first)
        with np.errstate(invalid='ignore'):
            assert np.isnan(S.stage3(V, W, H2)[:, n0]).all()
        H2[:, n0] = H[:, n0]
        R3 = S.stage3(V, W, H2)
        assert not R3[f0].any() and not R3[:, n0].any() and np.isfinite(R3).all()
        U, rs = S.stage4(R3, H2)
        assert not U[f0].any() and np.count_nonzero(U == 0) == K
        W5, s5, cs5 = S.stage5(W, U, rs)
        assert not W5[f0].any() and np.count_nonzero(W5 == 0) == K and np.isfinite(W5).all() and (s5 > 0).all()
