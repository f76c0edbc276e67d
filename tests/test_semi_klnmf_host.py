"""Semi-supervised KL-NMF (GCCNMF_FLAG_FREE_ATOMS) without a device: every argument rule through the C ABI (rejected calls only: they
return before touching memory), the plan bit, the Python checkers and the word klnmf() packs; that float32 NumPy passes the bars of the
GPU test at every shape of its table (the bars are attainable); and the properties of the float64 restatement that make the feature
worth having (tests/semi_klnmf_restatement.py)."""
import ctypes

import numpy as np
import pytest

import klnmf_stages_restatement as S
import semi_klnmf_restatement as M

FIXED_W, H_ONES, FREE = 1 << 16, 1 << 17, M.FREE_ATOMS
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
P = 4096        # a non-null, 16-byte aligned stand-in pointer: every call below returns before it touches memory


def _lib():
    from gcc_nmf_amd import _hip
    return _hip.lib()


def _klnmf(flags, F=513, N=100, K=144, batch=2):
    return _lib().gccnmf_klnmf(P, P, P, P, F, N, K, batch, 10, 0.0, 1e-16, flags, None)


def _stage(flags, stage, F=513, N=100, K=144, batch=2):
    return _lib().gccnmf_klnmf_stage(P, P, P, P, F, N, K, batch, 0.0, 1e-16, flags, stage, None)


# (flags, keywords) -> status: every rule of the header, each for gccnmf_klnmf, gccnmf_klnmf_stage (stages 1 and 4) and gccnmf_klnmf_plan
REJECTED = [
    (FREE(16) | FIXED_W, {}, ERR_ARG), (FREE(16) | H_ONES, {}, ERR_ARG), (FREE(16) | FIXED_W | H_ONES, {}, ERR_ARG),
    (FREE(16) | 4, {}, ERR_ARG), (FREE(16) | 4 | (3 << 8), {}, ERR_ARG), (FREE(16) | 2, {}, ERR_ARG),
    (FREE(129), dict(K=128 + 129), ERR_ARG), (FREE(255), dict(K=512), ERR_ARG),
    (FREE(16), dict(K=16), ERR_ARG), (FREE(16), dict(K=7), ERR_ARG),
    (FREE(16), dict(K=16 + 8), ERR_UNSUPPORTED), (FREE(1), dict(K=64), ERR_UNSUPPORTED), (FREE(17), dict(K=128), ERR_UNSUPPORTED),
    (FREE(16), dict(K=1024 + 16), ERR_UNSUPPORTED), (FREE(128), dict(K=1040), ERR_UNSUPPORTED),
    (FREE(16), dict(F=2050), ERR_UNSUPPORTED),
]


@pytest.mark.parametrize('flags,kw,status', REJECTED)
def test_rejected_calls(flags, kw, status):
    assert _klnmf(flags, **kw) == status
    fixed_bits = flags & (FIXED_W | H_ONES)
    for stage in (1, 4, 5):
        assert _stage(flags, stage, **kw) == (ERR_ARG if fixed_bits else status)      # (the stage call rejects the fixed bits on its own)
    a = dict(F=513, N=100, K=144, batch=2)
    a.update(kw)
    assert _lib().gccnmf_klnmf_plan(a['F'], a['N'], a['K'], a['batch'], flags) == -1


def test_a_misaligned_workspace_is_still_an_argument_error():
    assert _lib().gccnmf_klnmf(P, P, P, P + 4, 513, 100, 144, 2, 10, 0.0, 1e-16, FREE(16), None) == ERR_ARG
    assert _lib().gccnmf_klnmf_stage(P, P, P, P + 4, 513, 100, 144, 2, 0.0, 1e-16, FREE(16), 4, None) == ERR_ARG


def test_plan_bit_5_only_with_the_bits():
    lib = _lib()
    for F, N, Kf, n, B in M.SHAPES + [(513, 1244, 128, 16, 64), (513, 1244, 1008, 16, 64), (513, 1244, 896, 128, 64), (513, 1244, 64, 64, 1)]:
        assert lib.gccnmf_klnmf_plan(F, N, Kf + n, B, FREE(n)) == 32
        assert lib.gccnmf_klnmf_plan(F, N, Kf + n, B, FREE(n) | 1) == 32          # (the XCD block map of the blind GEMMs stays selectable)
        plain = lib.gccnmf_klnmf_plan(F, N, Kf + n, B, 0)
        assert plain >= 0 and not plain & 32
        assert not lib.gccnmf_klnmf_plan(F, N, Kf + n, B, FIXED_W) & 32


@pytest.mark.parametrize('n', [1, 16, 128])
def test_the_ragged_call_rejects_the_bits(n):
    lengths = (ctypes.c_int * 8)(*([100] * 8))
    assert _lib().gccnmf_klnmf_ragged(P, P, P, P, 513, lengths, 100, 256, 8, 10, 0.0, 1e-16, FREE(n), None) == ERR_ARG


def test_the_header_states_the_flag():
    import os
    text = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'gccnmf_hip.h')).read()
    assert '#define GCCNMF_FLAG_FREE_ATOMS(n) ((n) << 18)' in text
    from gcc_nmf_amd import _hip
    assert _hip.GCCNMF_FLAG_FREE_ATOMS(16) == 16 << 18 and _hip.GCCNMF_FLAG_FREE_ATOMS(128) == 128 << 18


def test_check_free_atoms():
    from gcc_nmf_amd._hip import check_free_atoms
    assert check_free_atoms(0, 100) == 0 and check_free_atoms(16, 128) == 16 and check_free_atoms(128, 896) == 128
    assert check_free_atoms(np.int64(1), 1008, 2049) == 1
    for n, Kf in [(-1, 128), (129, 128), (1.5, 128), (True, 128), ('4', 128), (None, 128),      # not a whole number in [0, 128]
                  (16, 0), (16, None),                                                          # no dictionary: n >= K
                  (16, 100), (1, 8),                                                            # (K - n) % 16
                  (16, 1024), (128, 912)]:                                                      # K > 1024
        with pytest.raises(ValueError):
            check_free_atoms(n, Kf)
    with pytest.raises(ValueError):
        check_free_atoms(16, 128, 2050)                                                         # F > 2049


def test_klnmf_packs_the_word(monkeypatch):
    from gcc_nmf_amd import _hip
    from test_stage_words_host import StubLibrary, last, STREAM
    stub = StubLibrary()
    monkeypatch.setattr(_hip, '_lib', stub)
    _hip.klnmf(1, 2, 3, 4, 513, 100, 144, 2, 10, 0.5, 1e-16, free_atoms=16, stream=STREAM)
    assert last(stub, 'gccnmf_klnmf') == (1, 2, 3, 4, 513, 100, 144, 2, 10, 0.5, 1e-16, 16 << 18, STREAM)
    _hip.klnmf(1, 2, 3, 4, 513, 100, 1024, 2, 10, 0.5, 1e-16, free_atoms=128, flags=1, stream=STREAM)
    assert last(stub, 'gccnmf_klnmf')[11] == (128 << 18) | 1
    _hip.klnmf(1, 2, 3, 4, 513, 100, 144, 2, 10, 0.5, 1e-16, stream=STREAM)
    assert last(stub, 'gccnmf_klnmf')[11] == 0
    calls = len(stub.calls)
    for kw in (dict(fixed_w=True), dict(h_ones=True, fixed_w=True), dict(groups=2), dict(flags=2), dict(flags=4)):
        with pytest.raises(ValueError):
            _hip.klnmf(1, 2, 3, 4, 513, 100, 144, 2, 10, 0.5, 1e-16, free_atoms=16, stream=STREAM, **kw)
    for K, n in ((144, 129), (16, 16), (140, 16), (1040, 16)):
        with pytest.raises(ValueError):
            _hip.klnmf(1, 2, 3, 4, 513, 100, K, 2, 10, 0.5, 1e-16, free_atoms=n, stream=STREAM)
    assert len(stub.calls) == calls          # nothing reached the library


def test_engine_argument_rules():
    """decided in front of the first device call (no device here)"""
    from gcc_nmf_amd.engine import GCCNMFEngine
    W = np.random.RandomState(0).rand(513, 64).astype(np.float32)
    for kw in (dict(numFreeAtoms=16), dict(dictionaryW=W, numFreeAtoms=16, initialH='ones'), dict(dictionaryW=W, numFreeAtoms=129),
               dict(dictionaryW=W[:, :60], numFreeAtoms=16), dict(dictionaryW=W, numFreeAtoms=16, dictionarySize=64),
               dict(dictionaryW=W, numFreeAtoms=16, lengths=[16000, 20000])):
        with pytest.raises(ValueError):
            GCCNMFEngine(None if 'lengths' in kw else 16000, **kw)


def test_initial_factors_are_the_drawn_ones():
    from gcc_nmf_amd.engine import klnmf_initial_factors, semi_supervised_initial_factors
    W = np.random.RandomState(1).rand(40, 16).astype(np.float32)
    W0, H0 = semi_supervised_initial_factors(W, 5, 30, 1e-16, 3)
    Wd, Hd = klnmf_initial_factors(40, 30, 21, 1e-16, 3)
    assert W0.dtype == np.float32 and np.array_equal(W0[:, :16], W) and np.array_equal(W0[:, 16:], Wd[:, 16:]) and np.array_equal(H0, Hd)


# ---- float32 NumPy passes the bars of the GPU test ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,N,Kf,n,B', M.SHAPES)
def test_float32_numpy_passes_the_stage_bars(F, N, Kf, n, B):
    V, W, H, _ = M.problem(F, N, Kf, n, min(B, 2))
    for b in range(V.shape[0]):
        R = np.asarray(S.stage3(V[b], W[b], H[b]), np.float32)              # the float32 R the device would hold before stage 4
        U, rs = M.stage4_free(R, H[b], n)
        U32, rs32 = M.stage4_free(R, H[b], n, np.float32)
        for got, ref, bar in ((U32, U, S.bar_U(N)), (rs32, rs, S.bar_rowsumH(N))):
            worst, miss = S.share(got, ref, bar)
            assert miss is None and worst <= 1, (worst, miss)
        f0 = S.zero_lines(F, N, b)[0]
        assert not U32[f0].any()                                           # the silent bin
        refs = M.stage5_free(W[b], U32, rs32, n)
        gots = M.stage5_free(W[b], U32, rs32, n, np.float32)
        for got, ref, bar in zip(gots, refs, (S.bar_W(F), S.bar_s(F), S.bar_colsumW(F))):
            worst, miss = S.share(got, ref, bar)
            assert miss is None and worst <= 1, (worst, miss)


@pytest.mark.parametrize('F,N,Kf,n,B', M.SHAPES)
def test_float32_numpy_passes_the_iteration_bars(F, N, Kf, n, B):
    V, W, H, _ = M.problem(F, N, Kf, n, 2, silent_frame=False)
    bars = M.iteration_bars(F, N, Kf + n)
    for b in range(2):
        Wr, Hr = M.iteration(V[b], W[b], H[b], n)
        Wg, Hg = M.iteration(V[b], W[b], H[b], n, dtype=np.float32)
        assert np.array_equal(Wg[:, :Kf], W[b][:, :Kf])
        for got, ref, bar in ((Wg[:, Kf:], Wr[:, Kf:], bars['W_free']), (Hg[:Kf], Hr[:Kf], bars['H_fixed']), (Hg[Kf:], Hr[Kf:], bars['H_free'])):
            worst, miss = S.share(got, ref, bar)
            assert miss is None and worst <= 1, (worst, miss)
        assert not Wg[S.zero_lines(F, N, b)[0], Kf:].any()


def test_problem_makes_the_edges_large():
    V, W, H, _ = M.problem(40, 65, 16, 33, 2)
    base = S.problem(40, 65, 49, 2)
    assert np.array_equal(V, base[0])
    assert (W[:, 39, :15] == base[1][:, 39, :15] * 4).all() and (W[:, :39, 15] == base[1][:, :39, 15] * 4).all()
    assert (H[:, 48] == base[2][:, 48] * 4).all() and (H[:, 15] == base[2][:, 15] * 4).all() and (H[:, 14] == base[2][:, 14]).all()


# ---- what the restatement says about the feature ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def unseen():
    from gcc_nmf_amd.engine import semi_supervised_initial_factors, klnmf_initial_factors
    V, Wfix = M.unseen_noise_problem()
    W0, H0 = semi_supervised_initial_factors(Wfix.astype(np.float32), 16, V.shape[1], 1e-16, 0)
    Hf0 = klnmf_initial_factors(V.shape[0], V.shape[1], 64, 1e-16, 0)[1]
    return V, Wfix, W0, H0, Hf0


@pytest.mark.parametrize('alpha', [0.0, 0.1])
def test_restatement_descends_and_keeps_the_dictionary(unseen, alpha):
    V, Wfix, W0, H0, _ = unseen
    trace = [M.divergence(V, W0, H0)]
    W, H = M.run(V, W0, H0, 16, 100, alpha, 1e-16, np.float64, trace)
    assert np.array_equal(W[:, :64], np.asarray(W0, np.float64)[:, :64])          # bit for bit
    assert all(b <= a for a, b in zip(trace, trace[1:])), 'the divergence rose'
    W32, H32 = M.run(V.astype(np.float32), W0, H0, 16, 100, alpha, 1e-16, np.float32)
    assert np.array_equal(W32[:, :64], W0[:, :64])
    W64, H64 = M.run(V.astype(np.float32), W0, H0, 16, 100, alpha, 1e-16, np.float64)
    for a, b in ((W32[:, 64:], W64[:, 64:]), (H32, H64)):
        assert np.linalg.norm(a - b) / np.linalg.norm(b) < 1e-4


def test_free_atoms_take_what_the_dictionary_cannot(unseen):
    V, Wfix, W0, H0, Hf0 = unseen
    W, H = M.run(V, W0, H0, 16, 100, 0.0, 1e-16)
    semi = M.divergence(V, W, H)
    fixed = M.divergence(V, Wfix, M.run_fixed(V, Wfix, Hf0, 100, 0.0, 1e-16))
    print('D after 100 iterations: dictionary alone %.1f, with 16 free atoms %.1f (%.4f of it)' % (fixed, semi, semi / fixed))
    assert semi < 0.5 * fixed
