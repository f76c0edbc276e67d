"""Itakura-Saito / Euclidean NMF beside KL-NMF, everything that needs no device: the float64 restatement (tests/beta_nmf_restatement.py)
against the KL restatement and against its own objective, the keyword rules of _hip, the named functions and the engines, the flag words
that reach the library, the workspace macro, and the library's argument errors (all decided before any HIP call)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import beta_nmf_restatement as B
import klnmf_stages_restatement as S
from gcc_nmf_amd import _hip

IS_BIT, EU_BIT = 1 << 26, 2 << 26
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'gccnmf_hip.h')
P = 4096      # a 16-byte aligned non-null "pointer": every call below is rejected before it is used


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def test_beta_1_is_the_kl_restatement_stage_by_stage():
    F, N, K = 33, 70, 16
    V, W, H, s = (a[0] for a in S.problem(F, N, K, 2, lines=False))
    colsumW, _ = S.stage0(W)
    R, Q = B.stage13(V, W, H, s, B.KL)
    assert np.array_equal(R, S.stage1(V, W, H, s)) and (Q == 1).all()
    H2 = B.stage2(W, H, s, R, Q)
    np.testing.assert_allclose(H2, S.stage2(W, H, s, R, colsumW), rtol=1e-13, atol=0)      # (W^T . 1 against sum_f W: the order of a float64 sum)
    R3, Q3 = B.stage13(V, W, H2, None, B.KL)
    assert np.array_equal(R3, S.stage3(V, W, H2)) and (Q3 == 1).all()
    Un, Ud = B.stage4(R3, Q3, H2)
    U, rowsumH = S.stage4(R3, H2)
    assert np.array_equal(Un, U)
    np.testing.assert_allclose(Ud, np.broadcast_to(rowsumH, Ud.shape), rtol=1e-13, atol=0)
    for got, want in zip(B.stage5(W, Un, Ud), S.stage5(W, U, rowsumH)):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize('F,N,K', [(33, 70, 16), (129, 130, 40), (130, 70, 136)])
@pytest.mark.parametrize('alpha', [0.0, 0.05])
@pytest.mark.parametrize('beta', [0, 1, 2])
@pytest.mark.parametrize('zeros', [0, 5])
def test_forty_float64_iterations_never_raise_the_objective(F, N, K, alpha, beta, zeros):
    """D_beta(V || W.H) + alpha sum(H) of the reference iteration, evaluated after every whole iteration: never above the value before
    (beyond 1e-12 relative: float64 round-off of a stalled run), and finite throughout."""
    V = B.low_rank_plus_noise(F, N, 6, 0.3, 3, zeros)
    rng = np.random.RandomState(F + N + K)
    W, H = rng.rand(F, K) + 1e-3, rng.rand(K, N) + 1e-3
    prev = B.divergence(V, W, H, beta) + alpha * H.sum()
    for it in range(40):
        W, H = B.iterate(V, W, H, beta, alpha, 1e-16, 1)
        cur = B.divergence(V, W, H, beta) + alpha * H.sum()
        assert np.isfinite(cur) and np.isfinite(W).all() and np.isfinite(H).all(), it
        assert cur <= prev * (1 + 1e-12), (it, prev, cur)
        prev = cur


def test_a_silent_frame_is_a_division_by_zero_in_the_reference_too():
    """why beta_nmf_restatement.problem carries no all-zero frame: H's column is exactly 0 after the H update, and IS's 1 / P is 1 / 0"""
    V, W, H, s = (a[0].copy() for a in S.problem(33, 70, 16, 2, lines=False))
    V[:, 5] = 0
    R, Q = B.stage13(V, W, H, s, B.IS)
    H2 = B.stage2(W, H, s, R, Q)
    assert not H2[:, 5].any()
    with np.errstate(divide='ignore', invalid='ignore'):
        R3, Q3 = B.stage13(V, W, H2, None, B.IS)
    assert np.isinf(Q3[:, 5]).all() and np.isnan(R3[:, 5]).all()


def test_trajectory_bars_grow_with_every_iteration():
    """the worst case compounds fast (every operand of a quotient is taken to err the wrong way): about 80 x per IS iteration, 30 x per
    Euclidean one -- three iterations of the smallest shape are what the GPU trajectory test can still use"""
    for beta in (B.IS, B.EUCLIDEAN):
        last = (0.0, 0.0)
        for n in (1, 2, 3):
            bars = B.trajectory_bars(beta, 33, 70, 16, n)
            assert bars[0] > last[0] and bars[1] > last[1] and max(bars) < 1.0
            last = bars
        one = B.trajectory_bars(beta, 513, 140, 128, 1)
        assert B.bar_W(513) < one[0] < 1e-3 and B.bar_H(513) < one[1] < 1e-3


# ---- keywords, decided before a device is looked for ---------------------------------------------------------------------------------------
def test_check_divergence():
    for given, want in (('kl', 'kl'), ('is', 'is'), ('euclidean', 'euclidean'), (0, 'is'), (1, 'kl'), (2, 'euclidean'), (2.0, 'euclidean'),
                        (np.int64(0), 'is')):
        assert _hip.check_divergence(given) == want
    for bad in ('IS', 'euclid', 0.5, 3, -1, None, True, False, [0], float('nan')):
        with pytest.raises(ValueError):
            _hip.check_divergence(bad)
    assert _hip.check_divergence('kl', 5000, 5000) == 'kl'          # the envelope is the IS / Euclidean call's alone
    assert _hip.check_divergence('is', 2049, 1024) == 'is'
    for F, K in ((2050, 16), (1, 16), (513, 1025), (513, 0)):
        with pytest.raises(ValueError):
            _hip.check_divergence('euclidean', F, K)


def test_keyword_rejections_before_any_device(monkeypatch):
    import gcc_nmf_amd.gccNMFFunctions as G
    from gcc_nmf_amd import engine, dropin
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(_hip, 'lib', lambda: pytest.fail('a rejected call reached the library'))
    assert list(inspect.signature(G.performBetaNMF).parameters) == ['V', 'dictionarySize', 'numIterations', 'beta', 'sparsityAlpha', 'epsilon', 'seedValue']
    d = dict((k, p.default) for k, p in inspect.signature(G.performBetaNMF).parameters.items())
    assert (d['sparsityAlpha'], d['epsilon'], d['seedValue']) == (0, 1e-16, 0)
    assert list(inspect.signature(G.getBetaDivergence).parameters) == ['V', 'W', 'H', 'beta']
    V = np.ones((4, 6), np.float32)
    for beta in (0.5, 'itakura', None, True):
        with pytest.raises(ValueError):
            G.performBetaNMF(V, 2, 10, beta)
        with pytest.raises(ValueError):
            G.getBetaDivergence(V, np.ones((4, 2)), np.ones((2, 6)), beta)
        with pytest.raises(ValueError):
            G.performBetaNMFUntilConverged(V, 2, 10, beta)
    with pytest.raises(ValueError):
        G.performBetaNMF(np.ones((4, G.LARGE_N_COLUMNS + 1), np.float32), 2, 10, 'is')        # the column-block path stays KL
    with pytest.raises(ValueError):
        G.performBetaNMF(V, 1025, 10, 2)
    with pytest.raises(ValueError):
        G.performBetaNMF(np.ones((2050, 6), np.float32), 2, 10, 0)
    with pytest.raises(ValueError):
        G.getBetaDivergence(V, np.ones((4, 2)), np.ones((3, 6)), 'is')
    with pytest.raises(ValueError):
        G.performBetaNMFUntilConverged(V, 2, 10, 'is', tolerance=2.0)
    mod = dropin.install()
    try:
        for name in ('performBetaNMF', 'getBetaDivergence', 'performBetaNMFUntilConverged', 'performKLNMFUntilConverged'):
            assert getattr(mod, name) is getattr(G, name)
    finally:
        dropin.uninstall()
    Wd = np.ones((513, 16), np.float32)
    for cls in (engine.GCCNMFEngine, engine.RaggedGCCNMFEngine, engine.GCCNMFEnhancementEngine):
        first = [16000, 20000] if cls is engine.RaggedGCCNMFEngine else 16000
        if cls is not engine.GCCNMFEnhancementEngine:
            assert inspect.signature(cls.__init__).parameters['divergence'].default == 'kl'
        for bad in ('IS', 0.5, None):
            with pytest.raises(ValueError):
                cls(first, divergence=bad)
        with pytest.raises(ValueError):
            cls(first, divergence='is', dictionaryW=Wd)
        with pytest.raises(ValueError):
            cls(first, divergence='euclidean', dictionarySize=1025)
        with pytest.raises(ValueError):
            cls(first, divergence='is', klnmf_flags=2)
        with pytest.raises(_hip.HipLibraryError):              # a valid choice gets as far as the device lookup
            cls(first, divergence='is')
    with pytest.raises(ValueError):
        engine.GCCNMFEngine(16000, divergence='is', dictionaryW=Wd, numFreeAtoms=8)
    with pytest.raises(ValueError):
        engine.GCCNMFEngine(16000, divergence='is', nmf_groups=2, batch=2)
    with pytest.raises(ValueError):
        engine.GCCNMFEngine(lengths=[16000, 20000], divergence='is', dictionaryW=Wd)
    for kw in (dict(fixed_w=True), dict(fixed_w=True, h_ones=True), dict(free_atoms=16), dict(groups=2), dict(flags=2), dict(flags=4)):
        with pytest.raises(ValueError):
            _hip.klnmf(1, 2, 3, 4, 513, 100, 128, 2, 5, 0.0, 1e-16, divergence='is', **kw)
    with pytest.raises(ValueError):
        _hip.klnmf_stage(1, 2, 3, 4, 513, 100, 128, 2, 0.0, 1e-16, 1, free_atoms=16, divergence='euclidean')
    with pytest.raises(ValueError):
        _hip.klnmf_divergence(1, 2, 3, 4, 513, 100, 128, 2, fixed=True, divergence='is')
    with pytest.raises(ValueError):
        _hip.klnmf(1, 2, 3, 4, 513, 100, 128, 2, 5, 0.0, 1e-16, divergence='beta')


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


def test_flag_words(stub):
    S_ = 0x5eed
    for name, bits in (('kl', 0), ('is', IS_BIT), ('euclidean', EU_BIT), (0, IS_BIT), (1, 0), (2, EU_BIT)):
        _hip.klnmf(1, 2, 3, 4, 513, 100, 128, 2, 5, 0.5, 1e-16, divergence=name, stream=S_)
        assert stub.calls[-1] == ('gccnmf_klnmf', (1, 2, 3, 4, 513, 100, 128, 2, 5, 0.5, 1e-16, bits, S_))
        _hip.klnmf(1, 2, 3, 4, 513, 100, 128, 2, 5, 0.5, 1e-16, flags=1, divergence=name, stream=S_)      # (no XCD affinity: accepted and ignored)
        assert stub.calls[-1][1][11] == bits | 1
        for stage in range(8):
            _hip.klnmf_stage(1, 2, 3, 4, 513, 100, 128, 2, 0.5, 1e-16, stage, divergence=name, stream=S_)
            assert stub.calls[-1] == ('gccnmf_klnmf_stage', (1, 2, 3, 4, 513, 100, 128, 2, 0.5, 1e-16, bits, stage, S_))
        ws = torch.zeros(2 * 528 * 128 + 8)
        out = _hip.klnmf_divergence(1, 2, 3, ws, 513, 100, 128, 2, divergence=name, stream=S_)
        assert stub.calls[-1] == ('gccnmf_klnmf_stage', (1, 2, 3, ws.data_ptr(), 513, 100, 128, 2, 0.0, 0.0, bits, 7, S_))
        assert out.dtype == torch.float64 and out.data_ptr() == ws.data_ptr() + 4 * 2 * 528 * 128 and out.numel() == 2
    _hip.klnmf_stage(1, 2, 3, 4, 513, 100, 144, 2, 0.5, 1e-16, 4, free_atoms=16, stream=S_)
    assert stub.calls[-1][1][10] == 16 << 18
    _hip.klnmf(1, 2, 3, 4, 513, 100, 128, 2, 5, 0.5, 1e-16, groups=2, stream=S_)                          # KL keeps every word it had
    assert stub.calls[-1][1][11] == 4 | 2 << 8
    assert (_hip.GCCNMF_FLAG_DIVERGENCE_IS, _hip.GCCNMF_FLAG_DIVERGENCE_EUCLIDEAN) == (IS_BIT, EU_BIT)
    assert B.FLAGS == {0: IS_BIT, 1: 0, 2: EU_BIT}


def test_workspace_macro_against_its_mirror(stub):
    text = open(HEADER).read()
    assert re.search(r'#define\s+GCCNMF_FLAG_DIVERGENCE_IS\s+\(1 << 26\)', text) and re.search(r'#define\s+GCCNMF_FLAG_DIVERGENCE_EUCLIDEAN\s+\(2 << 26\)', text)
    m = re.search(r'#define\s+GCCNMF_KLNMF_DIVERGENCE_WORKSPACE_FLOATS\(Fp, Kp, Np, batch\)\s+(.*)', text)
    assert m
    expr = m.group(1).replace('(long)', '')
    for Fp, Kp, Np, batch in ((528, 1024, 1280, 64), (48, 64, 128, 1), (144, 192, 192, 3), (2064, 1024, 64, 5)):
        want = eval(expr, {}, dict(Fp=Fp, Kp=Kp, Np=Np, batch=batch))
        assert want == _hip.klnmf_divergence_extra_floats(Fp, Kp, Np, batch) == batch * (Fp * Np + Fp * Kp) and want % 64 == 0
    # the whole workspace: the KL layout (the stub's 4321 floats), for IS / Euclid followed by the extra blocks
    assert _hip.klnmf_divergence_workspace_floats(513, 1244, 1024, 64) == 4321
    for d in ('is', 'euclidean', 0, 2):
        assert _hip.klnmf_divergence_workspace_floats(513, 1244, 1024, 64, d) == 4321 + 64 * 528 * (1280 + 1024)
        assert _hip.klnmf_divergence_workspace_floats(33, 70, 16, 1, d) == 4321 + 48 * (128 + 64)


# ---- the library's argument errors (decided before any HIP call: no device needed) ---------------------------------------------------------
def _lib():
    return _hip.lib()


def _calls(lib, flags, F=513, N=100, K=128, batch=2, ws=P):
    return (lib.gccnmf_klnmf(P, P, P, ws, F, N, K, batch, 3, 0.0, 1e-16, flags, None),
            lib.gccnmf_klnmf_stage(P, P, P, ws, F, N, K, batch, 0.0, 1e-16, flags, 1, None),
            lib.gccnmf_klnmf_stage(P, P, P, ws, F, N, K, batch, 0.0, 1e-16, flags, 7, None),
            lib.gccnmf_klnmf_plan(F, N, K, batch, flags))


def test_library_argument_errors():
    lib = _lib()
    assert len(_hip.SIGNATURES) == 46
    for bit in (IS_BIT, EU_BIT):
        for other in (IS_BIT | EU_BIT, bit | (1 << 16), bit | (1 << 16) | (1 << 17), bit | (1 << 17), bit | (16 << 18), bit | 4, bit | 4 | (3 << 8), bit | 2):
            assert _calls(lib, other) == (ERR_ARG, ERR_ARG, ERR_ARG, -1), hex(other)
        assert _calls(lib, bit, F=2050) == (ERR_UNSUPPORTED,) * 3 + (-1,)
        assert _calls(lib, bit, K=1025) == (ERR_UNSUPPORTED,) * 3 + (-1,)
        assert _calls(lib, bit, ws=P + 8)[:3] == (ERR_ARG,) * 3                                   # a workspace that is not 16-byte aligned
        assert lib.gccnmf_klnmf_stage(P, P, P, P, 513, 100, 128, 2, 0.0, 1e-16, bit, 8, None) == ERR_ARG      # an unknown stage
        n = (ctypes.c_int * 8)(*([100] * 8))
        assert lib.gccnmf_klnmf_ragged(P, P, P, P, 513, n, 100, 256, 8, 3, 0.0, 1e-16, bit, None) == ERR_ARG
        for F, N, K, batch in ((513, 1244, 1024, 64), (2049, 1, 1, 1), (2, 5, 1024, 3), (33, 70, 16, 1)) + tuple(B.SHAPES):
            assert lib.gccnmf_klnmf_plan(F, N, K, batch, bit) == 64                               # bit 6 alone
            assert lib.gccnmf_klnmf_plan(F, N, K, batch, bit | 1) == 64
    assert lib.gccnmf_klnmf_plan(513, 1244, 1024, 64, 0) & 64 == 0
    # the pinned KL workspace sizes do not move
    assert lib.gccnmf_klnmf_workspace_floats(513, 1244, 128, 64) % 32 == 0
    for F, N, K, batch in B.SHAPES:
        assert lib.gccnmf_klnmf_workspace_floats(F, N, K, batch) % 32 == 0                        # Q starts 16-byte aligned behind it
