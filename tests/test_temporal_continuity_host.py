"""Temporal-continuity KL-NMF, everything that needs no device: the float64 restatement (tests/temporal_continuity_restatement.py) against
a finite difference of its own cost, against the KL restatement and against its own objective, the keyword rules of _hip, the named
functions and the engines, the words that reach the library, the header macros, and the library's argument errors (all decided before any
HIP call)."""
import ctypes
import inspect
import os
import re
import struct

import numpy as np
import pytest
import torch

import klnmf_stages_restatement as S
import temporal_continuity_restatement as C
from gcc_nmf_amd import _hip

OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'gccnmf_hip.h')
P = 4096      # a 16-byte aligned non-null "pointer": every call below is rejected before it is used


def bits_of(weight):
    return struct.unpack('<I', struct.pack('<f', weight))[0]


def signed(v):
    return ctypes.c_int32(v & 0xffffffff).value


def words(K, batch, weight):
    """GCCNMF_CONTINUITY_K / _BATCH, restated"""
    b = bits_of(weight)
    return signed(K | (b & 0xffff0000)), signed(batch | ((b & 0xffff) << 16))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,segments', [(40, 2), (25, 1), (2, 2), (1, 2), (1, 1), (2, 1), (3, 2)])
def test_gp_minus_gm_is_the_gradient_of_the_cost(T, segments):
    """Gp - Gm against a central finite difference of c = T D / E in float64, at EVERY column: interior columns, both ends, both segments,
    T = 1 (the cost is 0 whatever h: the gradient is 0) and T = 2.  Step 1e-5 h: the truncation error is of the order (1e-5)^2 and the
    round-off 1e-16 / 1e-5 of the two terms' size Gp + Gm, so 1e-6 of that size is orders of magnitude above both."""
    rng = np.random.RandomState(T + segments)
    K, N = 3, T * segments
    H = np.abs(np.cumsum(rng.randn(K, N), axis=1)) * 0.2 + 0.05
    s = 0.5 + rng.rand(K)
    _, _, Gm, Gp = C.terms(H, s, segments)
    h = s[:, None] * H
    for k in range(K):
        for t in range(N):
            d = 1e-5 * h[k, t]
            up, down = h.copy(), h.copy()
            up[k, t] += d
            down[k, t] -= d
            fd = (C.cost(up, segments) - C.cost(down, segments)) / (2 * d)
            assert abs(fd - (Gp[k, t] - Gm[k, t])) <= 1e-6 * (Gp[k, t] + Gm[k, t]) + (0 if T > 1 else 1e-300), (k, t, fd, Gp[k, t], Gm[k, t])
    if T == 1:
        assert not Gp.any() and not Gm.any()


def test_terms_at_the_ends_and_on_a_dead_row():
    H = np.array([[1.0, 2.0, 4.0, 3.0, 5.0, 6.0], [0.0] * 6])
    E, D, Gm, Gp = C.terms(H, None, 2)
    assert E[0].tolist() == [21.0, 70.0] and D[0].tolist() == [5.0, 5.0]
    # segment 0 = (1, 2, 4): T = 3; the last column of a segment has no right neighbour, the first no left one
    np.testing.assert_allclose(Gp[0, :3], 2 * 3 * np.array([1 * 1.0, 2 * 2.0, 1 * 4.0]) / 21, rtol=1e-15)
    np.testing.assert_allclose(Gm[0, :3], 2 * 3 * np.array([2.0, 5.0, 2.0]) / 21 + 2 * 3 * np.array([1.0, 2.0, 4.0]) * 5 / 21 ** 2, rtol=1e-15)
    np.testing.assert_allclose(Gm[0, 3:], 2 * 3 * np.array([5.0, 9.0, 5.0]) / 70 + 2 * 3 * np.array([3.0, 5.0, 6.0]) * 5 / 70 ** 2, rtol=1e-15)
    assert not Gm[1].any() and not Gp[1].any() and not E[1].any()
    assert C.cost(H, 2) == 3 * 5.0 / 21 + 3 * 5.0 / 70
    assert C.cost(3.0 * H, 2) == pytest.approx(C.cost(H, 2), rel=1e-15)          # scale invariant


def test_weight_0_is_the_kl_stage_2_exactly():
    for F, T, K, segments in ((33, 40, 5, 2), (17, 25, 3, 1)):
        V, W, H, s = (a[0] for a in C.problem(F, T, K, segments, 1))
        colsumW, _ = S.stage0(W)
        R = S.stage1(V, W, H, s)
        assert np.array_equal(C.stage2(W, H, s, R, colsumW, 0.0, segments), S.stage2(W, H, s, R, colsumW))
        assert not np.array_equal(C.stage2(W, H, s, R, colsumW, 0.1, segments), S.stage2(W, H, s, R, colsumW))


def descent_data(F, T, K, segments, zeros):
    """the issue's data, drawn from RandomState(0) in its order (the zero mask is drawn either way, so W0 and H0 are the same with and
    without the zeros)"""
    rng = np.random.RandomState(0)
    N = T * segments
    Wt = rng.rand(F, K + 2)
    Ht = np.abs(np.cumsum(rng.randn(K + 2, N), axis=1)) * 0.2 + 0.05
    V = Wt @ Ht * (1 + 0.3 * rng.rand(F, N))
    mask = rng.rand(F, N) < 0.05
    if zeros:
        V[mask] = 0
    return V, rng.rand(F, K) + 1e-16, rng.rand(K, N) + 1e-16


@pytest.mark.parametrize('F,T,K,segments', [(33, 40, 5, 2), (17, 25, 3, 1), (65, 60, 8, 2), (9, 12, 2, 2)])
@pytest.mark.parametrize('beta', [0, 0.01, 0.1, 1, 10, 100])
@pytest.mark.parametrize('alpha', [0.0, 0.05])
@pytest.mark.parametrize('zeros', [False, True])
def test_forty_float64_iterations_never_raise_the_objective(F, T, K, segments, beta, alpha, zeros):
    """D_KL(V || W.H) + alpha sum(H) + beta sum(c), evaluated after every whole iteration: never above the value before by more than 1e-9
    of it, and finite throughout.  An empirical claim, not a theorem (the term's majoriser is Virtanen's heuristic split of the gradient)."""
    V, W, H = descent_data(F, T, K, segments, zeros)
    prev = C.objective(V, W, H, alpha, beta, segments)
    for it in range(40):
        W, H = C.iterate(V, W, H, beta, segments, alpha, 1e-16, 1)
        cur = C.objective(V, W, H, alpha, beta, segments)
        assert np.isfinite(cur) and np.isfinite(W).all() and np.isfinite(H).all(), it
        assert cur <= prev * (1 + 1e-9), (it, prev, cur)
        prev = cur


def test_the_term_smooths():
    """what the term is for: at the same iteration count a weight above 0 leaves a lower continuity cost than weight 0"""
    V, W, H = descent_data(33, 40, 5, 2, False)
    costs = [C.cost(C.iterate(V, W, H, beta, 2, 0.0, 1e-16, 40)[1], 2) for beta in (0, 1, 10)]
    assert costs[0] > costs[1] > costs[2]


@pytest.mark.parametrize('F,T,K,segments,files', C.SHAPES)
def test_float32_numpy_passes_the_stage_2_bars(F, T, K, segments, files):
    """the arithmetic csrc/nmf_smooth.hip states -- the terms in float64 rounded once, the epilogue in float32 operation by operation --
    restated in NumPy passes bar_G and bar_H at every GPU shape and weight 10: the bars are reachable, before any device is asked"""
    f32, w = np.float32, np.float32(10.0)
    for V, W, H, s in zip(*C.problem(F, T, K, segments, files)):
        colsumW, R = W.sum(0, dtype=f32), S.stage1(V, W, H, s).astype(f32)
        E, D, Gm, Gp = C.terms(H, s, segments)
        Gm32, Gp32 = Gm.astype(f32), Gp.astype(f32)
        num = (W.T @ R).astype(f32) + w * Gm32
        den = ((colsumW + S.ALPHA)[:, None] + w * Gp32) + S.EPS
        got = (H * s[:, None]) * (num / den)
        assert got.dtype == f32
        assert C.share(Gm32, Gm, C.bar_G())[1] is None and C.share(Gp32, Gp, C.bar_G())[1] is None
        worst, miss = C.share(got, C.stage2(W, H, s, R, colsumW, w, segments), C.bar_H(F))
        assert miss is None and worst < 1, (worst, miss)


def test_conditioning_bounds_the_error_of_D_and_the_trajectory_bars_grow():
    rng = np.random.RandomState(5)
    H = np.abs(np.cumsum(rng.randn(6, 80), axis=1)) * 0.2 + 0.05
    kappa = C.conditioning(H, 2)
    assert kappa > 1
    e = 1e-6
    for _ in range(20):
        Hp = H * (1 + e * (2 * rng.rand(*H.shape) - 1))
        D, Dp = C.terms(H, None, 2)[1], C.terms(Hp, None, 2)[1]
        assert (np.abs(Dp - D) <= 4 * kappa * e * D * (1 + 1e-3)).all()
    assert C.conditioning(np.ones((2, 8)), 2) == 0.0          # D = 0 everywhere: nothing to amplify
    last = (0.0, 0.0)
    for n in (1, 2, 3):
        bars = C.trajectory_bars(33, 70, 16, n, 2.0)
        assert bars[0] > last[0] and bars[1] > last[1] and max(bars) < 1.0
        last = bars
    assert C.trajectory_bars(33, 70, 16, 1, 2.0)[1] > C.bar_H(33) and C.trajectory_bars(33, 70, 16, 3, 20.0)[1] > last[1]


def test_shapes_reach_what_they_are_for():
    Ts = set(T for _, T, _, _, _ in C.SHAPES)
    assert {40, 64, C.ROW_PASS + 1, 1, 2} <= Ts
    assert set(K for _, _, K, _, _ in C.SHAPES) == {1, 33, 100, 130} and set(F for F, _, _, _, _ in C.SHAPES) == {2, 33, 513}
    assert any(seg == 1 and T % 2 for _, T, _, seg, _ in C.SHAPES)
    V, W, H, s = C.problem(33, 40, 33, 2, 2)
    assert not H[0, 1].any() and H[1, 1].all() and C.terms(H[0], s[0], 2)[0][1].tolist() == [0, 0]


# ---- keywords, decided before a device is looked for ---------------------------------------------------------------------------------------
def test_check_continuity():
    assert _hip.check_continuity(0) == (0.0, 1) and _hip.check_continuity(0.5, 2) == (0.5, 2) and _hip.check_continuity(np.float32(2), np.int64(1)) == (2.0, 1)
    for bad in (-1, -0.001, float('nan'), float('inf'), None, True, '1', [1.0], 1j):
        with pytest.raises(ValueError):
            _hip.check_continuity(bad)
    for bad in (0, 3, 1.0, True, None, '2'):
        with pytest.raises(ValueError):
            _hip.check_continuity(1.0, bad)


def test_keyword_rejections_before_any_device(monkeypatch):
    import gcc_nmf_amd.gccNMFFunctions as G
    from gcc_nmf_amd import engine, dropin
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(_hip, 'lib', lambda: pytest.fail('a rejected call reached the library'))
    assert list(inspect.signature(G.performTemporalKLNMF).parameters) == ['V', 'dictionarySize', 'numIterations', 'sparsityAlpha', 'temporalContinuity',
                                                                          'numSegments', 'epsilon', 'seedValue']
    d = dict((k, p.default) for k, p in inspect.signature(G.performTemporalKLNMF).parameters.items())
    assert (d['numSegments'], d['epsilon'], d['seedValue']) == (1, 1e-16, 0)
    assert list(inspect.signature(G.getTemporalContinuity).parameters) == ['H', 'numSegments']
    assert inspect.signature(G.getTemporalContinuity).parameters['numSegments'].default == 1
    V = np.ones((4, 6), np.float32)
    for bad in (-1.0, float('nan'), float('inf'), None, True):
        with pytest.raises(ValueError):
            G.performTemporalKLNMF(V, 2, 10, 0, bad)
    for bad in (0, 3, 1.5, True):
        with pytest.raises(ValueError):
            G.performTemporalKLNMF(V, 2, 10, 0, 1.0, bad)
        with pytest.raises(ValueError):
            G.getTemporalContinuity(np.ones((2, 6)), bad)
    with pytest.raises(NotImplementedError):
        G.performTemporalKLNMF(np.ones((4, G.LARGE_N_COLUMNS + 1), np.float32), 2, 10, 0, 1.0)
    with pytest.raises(ValueError):
        G.performTemporalKLNMF(V, 1025, 10, 0, 1.0)
    with pytest.raises(ValueError):
        G.performTemporalKLNMF(np.ones((2050, 6), np.float32), 2, 10, 0, 1.0)
    with pytest.raises(ValueError):
        G.performTemporalKLNMF(np.ones((4, 7), np.float32), 2, 10, 0, 1.0, 2)          # two segments, N odd
    with pytest.raises(ValueError):
        G.getTemporalContinuity(np.ones((2, 7)), 2)
    H = np.abs(np.cumsum(np.random.RandomState(3).randn(4, 30), axis=1)) + 0.1
    for segments in (1, 2):
        assert G.getTemporalContinuity(H, segments) == C.cost(H, segments) > 0
    assert G.getTemporalContinuity(np.zeros((2, 6))) == 0.0
    mod = dropin.install()
    try:
        for name in ('performTemporalKLNMF', 'getTemporalContinuity'):
            assert getattr(mod, name) is getattr(G, name)
    finally:
        dropin.uninstall()
    Wd = np.ones((513, 16), np.float32)
    for cls in (engine.GCCNMFEngine, engine.RaggedGCCNMFEngine, engine.GCCNMFEnhancementEngine):
        first = [16000, 20000] if cls is engine.RaggedGCCNMFEngine else 16000
        if cls is not engine.GCCNMFEnhancementEngine:
            params = inspect.signature(cls.__init__).parameters
            assert list(params)[-1] == 'temporalContinuity' and params['temporalContinuity'].default == 0.0
        for bad in (-1.0, float('nan'), None, True):
            with pytest.raises(ValueError):
                cls(first, temporalContinuity=bad)
        with pytest.raises(ValueError):
            cls(first, temporalContinuity=0.1, dictionaryW=Wd)
        with pytest.raises(ValueError):
            cls(first, temporalContinuity=0.1, divergence='is')
        with pytest.raises(ValueError):
            cls(first, temporalContinuity=0.1, tolerance=1e-4)
        with pytest.raises(ValueError):
            cls(first, temporalContinuity=0.1, klnmf_flags=2)
        with pytest.raises(ValueError):
            cls(first, temporalContinuity=0.1, klnmf_flags=4)
        with pytest.raises(ValueError):
            cls(first, temporalContinuity=0.1, dictionarySize=1025)
        with pytest.raises(_hip.HipLibraryError):              # a valid choice gets as far as the device lookup
            cls(first, temporalContinuity=0.1)
    with pytest.raises(ValueError):
        engine.GCCNMFEngine(16000, temporalContinuity=0.1, dictionaryW=Wd, numFreeAtoms=8)
    with pytest.raises(ValueError):
        engine.GCCNMFEngine(16000, temporalContinuity=0.1, nmf_groups=2, batch=2)
    for kw in (dict(fixed_w=True), dict(fixed_w=True, h_ones=True), dict(free_atoms=16), dict(groups=2), dict(flags=2), dict(flags=4),
               dict(divergence='is'), dict(divergence=2)):
        with pytest.raises(ValueError):
            _hip.klnmf(1, 2, 3, 4, 513, 100, 128, 2, 5, 0.0, 1e-16, continuity=0.5, **kw)
    for kw in (dict(free_atoms=16), dict(divergence='euclidean'), dict(flags=2)):
        with pytest.raises(ValueError):
            _hip.klnmf_stage(1, 2, 3, 4, 513, 100, 128, 2, 0.0, 1e-16, 1, continuity=0.5, **kw)
    for kw in (dict(continuity=-1.0), dict(continuity=float('inf')), dict(continuity=True), dict(continuity=1.0, segments=3),
               dict(continuity=1.0, segments=2, N=101), dict(continuity=1.0, K=1025), dict(continuity=1.0, F=2050), dict(continuity=1.0, batch=65536),
               dict(continuity=1e-60)):
        shape = dict(F=513, N=100, K=128, batch=2)
        shape.update((k, kw.pop(k)) for k in list(kw) if k in shape)
        with pytest.raises(ValueError):
            _hip.klnmf(1, 2, 3, 4, shape['F'], shape['N'], shape['K'], shape['batch'], 5, 0.0, 1e-16, **kw)


# ---- the words that reach the library -------------------------------------------------------------------------------------------------------
class StubLibrary(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 4321 if name.endswith('_workspace_floats') else 0
        return entry


@pytest.fixture
def stub(monkeypatch):
    lib = StubLibrary()
    monkeypatch.setattr(_hip, '_lib', lib)
    return lib


def test_words(stub):
    S_ = 0x5eed
    # weight 0: exactly the words of a call without the keywords
    for kw in (dict(), dict(continuity=0), dict(continuity=0.0, segments=2)):
        _hip.klnmf(1, 2, 3, 4, 513, 100, 128, 2, 5, 0.5, 1e-16, stream=S_, **kw)
        assert stub.calls[-1] == ('gccnmf_klnmf', (1, 2, 3, 4, 513, 100, 128, 2, 5, 0.5, 1e-16, 0, S_))
        _hip.klnmf(1, 2, 3, 4, 513, 100, 128, 2, 5, 0.5, 1e-16, groups=2, stream=S_, **kw)
        assert stub.calls[-1][1][6:8] == (128, 2) and stub.calls[-1][1][11] == 4 | 2 << 8
        _hip.klnmf(1, 2, 3, 4, 513, 100, 128, 2, 5, 0.5, 1e-16, divergence='is', stream=S_, **kw)
        assert stub.calls[-1][1][6:8] == (128, 2) and stub.calls[-1][1][11] == 1 << 26
        _hip.klnmf_stage(1, 2, 3, 4, 513, 100, 128, 2, 0.5, 1e-16, 2, stream=S_, **kw)
        assert stub.calls[-1] == ('gccnmf_klnmf_stage', (1, 2, 3, 4, 513, 100, 128, 2, 0.5, 1e-16, 0, 2, S_))
    for weight in (10.0, 0.01, 1.0, 3.4e38, 1e-40):
        for segments, fl in ((1, C.CONTINUITY), (2, C.CONTINUITY | C.STEREO)):
            Kw, Bw = words(128, 2, weight)
            _hip.klnmf(1, 2, 3, 4, 513, 100, 128, 2, 5, 0.5, 1e-16, continuity=weight, segments=segments, stream=S_)
            assert stub.calls[-1] == ('gccnmf_klnmf', (1, 2, 3, 4, 513, 100, Kw, Bw, 5, 0.5, 1e-16, fl, S_))
            _hip.klnmf(1, 2, 3, 4, 513, 100, 128, 2, 5, 0.5, 1e-16, flags=1, continuity=weight, segments=segments, stream=S_)
            assert stub.calls[-1][1][11] == fl | 1                                                # (no XCD affinity: accepted and ignored)
            for stage in range(8):
                _hip.klnmf_stage(1, 2, 3, 4, 513, 100, 128, 2, 0.5, 1e-16, stage, continuity=weight, segments=segments, stream=S_)
                assert stub.calls[-1] == ('gccnmf_klnmf_stage', (1, 2, 3, 4, 513, 100, Kw, Bw, 0.5, 1e-16, fl, stage, S_))
            # the words unpack to what went in
            b = ((Kw & 0xffffffff) & 0xffff0000) | ((Bw & 0xffffffff) >> 16)
            assert (Kw & 0xffff, Bw & 0xffff, b) == (128, 2, bits_of(weight))
    assert _hip.continuity_words(1024, 65535, 10.0) == words(1024, 65535, 10.0)
    assert (_hip.GCCNMF_FLAG_CONTINUITY, _hip.GCCNMF_FLAG_CONTINUITY_STEREO) == (C.CONTINUITY, C.STEREO) == (1 << 28, 1 << 29)
    assert C.flags(1) == 1 << 28 and C.flags(2) == 3 << 28


def test_header_macros_against_their_mirrors(stub):
    text = open(HEADER).read()
    assert re.search(r'#define\s+GCCNMF_FLAG_CONTINUITY\s+\(1 << 28\)', text) and re.search(r'#define\s+GCCNMF_FLAG_CONTINUITY_STEREO\s+\(1 << 29\)', text)
    m = re.search(r'#define\s+GCCNMF_KLNMF_CONTINUITY_WORKSPACE_FLOATS\(Kp, Np, batch\)\s+(.*)', text)
    assert m
    expr = m.group(1).replace('(long)', '')
    for Kp, Np, batch in ((1024, 2496, 64), (64, 128, 1), (192, 192, 3), (1024, 64, 5)):
        want = eval(expr, {}, dict(Kp=Kp, Np=Np, batch=batch))
        assert want == _hip.klnmf_continuity_extra_floats(Kp, Np, batch) == 2 * batch * Kp * Np + 4 * batch * Kp and want % 4 == 0
    # the packing macros, evaluated as C evaluates them on 32-bit words
    mk = re.search(r'#define\s+GCCNMF_CONTINUITY_K\(K, weight_bits\)\s+(.*)', text).group(1)
    mb = re.search(r'#define\s+GCCNMF_CONTINUITY_BATCH\(batch, weight_bits\)\s+(.*)', text).group(1)
    assert mk == '((int)((unsigned)(K) | ((unsigned)(weight_bits) & 0xffff0000u)))' and mb == '((int)((unsigned)(batch) | ((unsigned)(weight_bits) << 16)))'
    for K, batch, weight in ((128, 2, 10.0), (1024, 65535, 0.01), (1, 1, 3.4e38)):
        b = bits_of(weight)
        assert _hip.continuity_words(K, batch, weight) == (signed(K | (b & 0xffff0000)), signed((batch | (b << 16)) & 0xffffffff))
    # the whole workspace: the KL layout (the stub's 4321 floats) followed by the extra blocks
    assert _hip.klnmf_continuity_workspace_floats(513, 2488, 1024, 64) == 4321 + 64 * 1024 * (2 * 2496 + 4)
    assert _hip.klnmf_continuity_workspace_floats(33, 70, 16, 1) == 4321 + 64 * (2 * 128 + 4)


# ---- the library's argument errors (decided before any HIP call: no device needed) ---------------------------------------------------------
def _calls(lib, flags, weight=1.0, F=513, N=100, K=128, batch=2, ws=P):
    Kw, Bw = words(K, batch, weight) if flags & C.CONTINUITY else (K, batch)
    return (lib.gccnmf_klnmf(P, P, P, ws, F, N, Kw, Bw, 3, 0.0, 1e-16, flags, None),
            lib.gccnmf_klnmf_stage(P, P, P, ws, F, N, Kw, Bw, 0.0, 1e-16, flags, 2, None),
            lib.gccnmf_klnmf_stage(P, P, P, ws, F, N, Kw, Bw, 0.0, 1e-16, flags, 7, None),
            lib.gccnmf_klnmf_plan(F, N, Kw, Bw, flags))


def test_library_argument_errors():
    lib = _hip.lib()
    assert len(_hip.SIGNATURES) == 46
    assert _calls(lib, C.STEREO) == (ERR_ARG, ERR_ARG, ERR_ARG, -1)                                # bit 29 without bit 28
    for bit in (C.CONTINUITY, C.CONTINUITY | C.STEREO):
        for other in (bit | (1 << 16), bit | (1 << 16) | (1 << 17), bit | (1 << 17), bit | (16 << 18), bit | (1 << 26), bit | (2 << 26), bit | 4,
                      bit | 4 | (3 << 8), bit | 2):
            assert _calls(lib, other) == (ERR_ARG, ERR_ARG, ERR_ARG, -1), hex(other)
        for weight in (-1.0, float('nan'), float('inf'), -float('inf')):
            assert _calls(lib, bit, weight) == (ERR_ARG, ERR_ARG, ERR_ARG, -1), weight
        assert _calls(lib, bit, F=2050) == (ERR_UNSUPPORTED,) * 3 + (-1,)
        assert _calls(lib, bit, K=1025) == (ERR_UNSUPPORTED,) * 3 + (-1,)
        assert _calls(lib, bit, K=0) == (ERR_ARG,) * 3 + (-1,)
        assert _calls(lib, bit, ws=P + 8)[:3] == (ERR_ARG,) * 3                                   # a workspace that is not 16-byte aligned
        Kw, Bw = words(128, 2, 1.0)
        assert lib.gccnmf_klnmf_stage(P, P, P, P, 513, 100, Kw, Bw, 0.0, 1e-16, bit, 8, None) == ERR_ARG      # an unknown stage
        assert lib.gccnmf_klnmf_stage(0, P, P, P, 513, 100, Kw, Bw, 0.0, 1e-16, bit, 2, None) == ERR_ARG      # a null pointer
        n = (ctypes.c_int * 8)(*([100] * 8))
        assert lib.gccnmf_klnmf_ragged(P, P, P, P, 513, n, 100, 256, 8, 3, 0.0, 1e-16, bit, None) == ERR_ARG
        for weight in (0.0, 1e-3, 10.0, 3.4e38):
            for F, N, K, batch in ((513, 2488, 1024, 64), (2049, 2, 1, 1), (2, 6, 1024, 3), (33, 70, 16, 1), (33, 70, 16, 65535)):
                Kw, Bw = words(K, batch, weight)
                assert lib.gccnmf_klnmf_plan(F, N, Kw, Bw, bit) == C.PLAN_BIT                     # bit 7 alone
                assert lib.gccnmf_klnmf_plan(F, N, Kw, Bw, bit | 1) == C.PLAN_BIT
    assert _calls(lib, C.CONTINUITY | C.STEREO, N=101) == (ERR_ARG, ERR_ARG, ERR_ARG, -1)          # two segments, N odd
    assert lib.gccnmf_klnmf_plan(513, 101, *words(128, 2, 1.0), C.CONTINUITY) == C.PLAN_BIT       # one segment takes any N
    assert lib.gccnmf_klnmf_plan(513, 1244, 1024, 64, 0) & C.PLAN_BIT == 0
    # a call without bit 28 reads K and batch as they are: batch = 65536 + 2 is a batch, not a weight
    assert lib.gccnmf_klnmf_plan(513, 100, 128, 65538, 0) >= 0
    for F, T, K, segments, batch in C.SHAPES:
        assert lib.gccnmf_klnmf_workspace_floats(F, T * segments, K, batch) % 32 == 0             # Gm starts 16-byte aligned behind it
