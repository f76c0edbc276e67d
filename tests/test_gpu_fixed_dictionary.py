"""KL-NMF coefficients against a fixed, pre-trained dictionary (gccnmf_klnmf with GCCNMF_FLAG_FIXED_W, csrc/nmf_fixed.hip).

The references are float64 / NumPy restatements of performKLNMF's H update (gccNMF/gccNMFFunctions.py:76) with W never updated."""
import numpy as np
import pytest
import torch

import gcc_checks as C
from oracle.rt_oracle import make_rt_dictionary

pytestmark = pytest.mark.gpu

FIXED_W, H_ONES = 1 << 16, 1 << 17


def _lib():
    from gcc_nmf_amd import _hip
    return _hip.lib()


def _geom(F, N, K):
    Fp, Kp, Np = -(-F // 16) * 16, -(-K // 64) * 64, -(-N // 64) * 64
    return Fp, Kp, Np


def _run(V, W, H0, iters, alpha=0.0, eps=1e-16, ones=False, nan_fill=True):
    """V (B, F, N), W (F, K), H0 (B, K, N) or None (ones) -> H (B, Kp, Np) full padded result, W after the call (Fp, Kp)."""
    lib = _lib()
    B, F, N = V.shape
    K = W.shape[1]
    Fp, Kp, Np = _geom(F, N, K)
    dev = 'cuda'
    Vd = torch.zeros((B, Fp, Np), dtype=torch.float32, device=dev)
    Vd[:, :F, :N] = torch.from_numpy(V).to(dev)
    Wd = torch.zeros((Fp, Kp), dtype=torch.float32, device=dev)
    Wd[:F, :K] = torch.from_numpy(W).to(dev)
    Hd = torch.full((B, Kp, Np), float('nan') if nan_fill else 0.0, dtype=torch.float32, device=dev)
    if H0 is not None:
        Hd[:, :K, :N] = torch.from_numpy(H0).to(dev)
    ws = torch.full((lib.gccnmf_klnmf_workspace_floats(F, N, K, B),), float('nan'), dtype=torch.float32, device=dev)
    flags = FIXED_W | (H_ONES if ones else 0)
    rc = lib.gccnmf_klnmf(Vd.data_ptr(), Wd.data_ptr(), Hd.data_ptr(), ws.data_ptr(), F, N, K, B, iters, alpha, eps, flags,
                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    import ctypes
    st = ctypes.c_int(-1)
    assert lib.gccnmf_klnmf_chain_status(ws.data_ptr(), F, N, K, B, ctypes.byref(st)) == 0
    assert st.value == 0
    return Hd.cpu().numpy(), Wd.cpu().numpy()


def _inputs(B, F, N, K, seed):
    rng = np.random.RandomState(seed)
    V = (rng.rand(B, F, N).astype(np.float32) + np.float32(0.01))
    W = make_rt_dictionary(seed + 1, F, K)
    H0 = rng.rand(B, K, N).astype(np.float32) + np.float32(0.01)
    V[:, -1, :] *= 100          # a dropped tail row / atom shows
    W[-1, :] *= 100
    W[:, -1] *= 100
    return V, W, H0


def _one_iteration_f64(V, W, H, alpha, eps):
    V, W, H = V.astype(np.float64), W.astype(np.float64), H.astype(np.float64)
    P = W @ H
    R = V / P
    U = W.T @ R
    den = (W.astype(np.float32).sum(0).astype(np.float64) + alpha + eps)[:, None]
    return H * U / den, R


SHAPES = [(129, 1, 1, 1), (129, 64, 77, 3), (257, 96, 1244, 1), (513, 128, 77, 3), (513, 200, 1244, 1), (2049, 1024, 77, 1),
          (257, 1024, 1, 1), (129, 200, 77, 64)]


@pytest.mark.parametrize('F,K,N,B', SHAPES)
def test_one_iteration_elementwise(F, K, N, B):
    V, W, H0 = _inputs(B, F, N, K, F + K + N)
    Hd, Wout = _run(V, W, H0, 1, alpha=0.1)
    Fp, Kp, Np = _geom(F, N, K)
    for b in range(B):
        ref, R = _one_iteration_f64(V[b], W, H0[b], 0.1, 1e-16)
        # bound: the P error (F x K products) carried through R, plus the U reduction over F
        P_abs = W.astype(np.float64) @ H0[b].astype(np.float64)
        relP = C.gemm_bound(P_abs, K) / P_abs + 2 ** -23
        absU = W.T.astype(np.float64) @ (np.abs(R) * (1 + relP))
        bound = H0[b] * (C.gemm_bound(absU, F) + W.T.astype(np.float64) @ (np.abs(R) * relP)) / \
            (W.astype(np.float32).sum(0).astype(np.float64) + 0.1)[:, None] + 4 * 2 ** -24 * np.abs(ref)
        got = Hd[b, :K, :N].astype(np.float64)
        assert np.isfinite(got).all()
        assert (np.abs(got - ref) <= bound * 2).all(), np.abs(got - ref).max()
        C.check_zero(Hd[b, K:, :], 'H padding rows')
        C.check_zero(Hd[b, :, N:], 'H padding columns')
    assert np.array_equal(Wout[:F, :K], W)


def _numpy_fixed(V, W, H, iters, alpha, eps=1e-16):
    H = H.copy()
    for _ in range(iters):
        H *= np.dot(W.T, V / np.dot(W, H)) / (np.sum(W, axis=0)[:, np.newaxis] + alpha + eps)
    return H


@pytest.mark.parametrize('alpha', [0.0, 0.1])
@pytest.mark.parametrize('init', ['random', 'ones'])
def test_hundred_iterations_against_numpy(alpha, init):
    from gcc_nmf_amd.engine import klnmf_initial_factors
    F, K, N, B = 513, 128, 1244, 2
    rng = np.random.RandomState(5)
    V = rng.rand(B, F, N).astype(np.float32) + np.float32(0.01)
    W = make_rt_dictionary(3, F, K)
    H0 = klnmf_initial_factors(F, N, K)[1] if init == 'random' else np.ones((K, N), np.float32)
    Hd, Wout = _run(V, W, None if init == 'ones' else np.broadcast_to(H0, (B, K, N)).copy(), 100, alpha=alpha, ones=init == 'ones')
    assert np.array_equal(Wout[:F, :K], W), 'W changed'
    for b in range(B):
        ref = _numpy_fixed(V[b], W, H0, 100, alpha)
        assert np.abs(Hd[b, :K, :N] - ref).max() <= 1e-4 * np.abs(ref).max()


def test_descent():
    F, K, N, B = 257, 64, 500, 2
    V, W, H0 = _inputs(B, F, N, K, 11)
    prev = None
    for it in [0, 1, 2, 5, 20, 100]:
        Hd, _ = _run(V, W, H0, it)
        H = Hd[:, :K, :N].astype(np.float64)
        WH = np.einsum('fk,bkn->bfn', W.astype(np.float64), H)
        Vd = V.astype(np.float64)
        D = (Vd * np.log(Vd / WH) - Vd + WH).sum()
        if prev is not None:
            assert D <= prev * (1 + 1e-6), (it, D, prev)
        prev = D


def test_bitwise_batch_independence():
    F, K, N, B = 513, 1024, 1244, 64
    V, W, H0 = _inputs(B, F, N, K, 21)
    whole, _ = _run(V, W, H0, 3)
    alone, _ = _run(V[37:38], W, H0[37:38], 3)
    assert np.array_equal(whole[37], alone[0])
    perm = np.random.RandomState(0).permutation(B)
    permuted, _ = _run(V[perm], W, H0[perm], 3)
    assert np.array_equal(permuted, whole[perm])


@pytest.mark.parametrize('K', [128, 1024])
def test_engine_with_dictionary_on_dev1(dev1, K):
    from gcc_nmf_amd.engine import GCCNMFEngine, inferKLNMFCoefficients
    x, sr = dev1
    x = np.asarray(x, np.float32)
    W = make_rt_dictionary(7, 513, K)
    blind = GCCNMFEngine(x.shape[-1], sampleRate=sr, dictionarySize=K, numIterations=2)
    fixed = GCCNMFEngine(x.shape[-1], sampleRate=sr, dictionaryW=W, numIterations=100)
    yb = blind.separate(x)
    y = fixed.separate(x)
    assert not fixed.chain_failed()
    assert np.array_equal(blind.get_tdoa_indexes(), fixed.get_tdoa_indexes())
    Wg, Hg = fixed.get_WH()
    assert np.array_equal(Wg[0], W)
    V = fixed.get_V()
    assert np.array_equal(Hg[0], inferKLNMFCoefficients(V[0], W, 100))
    assert np.isfinite(y).all() and y.shape == yb.shape
    y2 = list(fixed.separate_batches([x[None], x[None]]))
    assert np.array_equal(y2[0], y) and np.array_equal(y2[1], y)
    pcm = (np.clip(x.T, -1, 1) * 32767).astype(np.int16)
    out = fixed.separate_pcm16(pcm)
    assert out.shape[:2] == (1, fixed.g.S)


def test_ragged_with_dictionary():
    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_mixture
    W = make_rt_dictionary(9, 513, 128)
    lengths = [16000, 24000, 16000, 40000]
    xs = [synthetic_mixture(i, n) for i, n in enumerate(lengths)]
    rag = GCCNMFEngine(lengths=lengths, dictionaryW=W, numIterations=20)
    out = rag.separate(xs)
    for n in sorted(set(lengths)):
        idx = [i for i, m in enumerate(lengths) if m == n]
        e = GCCNMFEngine(n, batch=len(idx), dictionaryW=W, numIterations=20)
        y = e.separate(np.stack([xs[i] for i in idx]))
        for k, i in enumerate(idx):
            assert np.array_equal(out[i], y[k])
