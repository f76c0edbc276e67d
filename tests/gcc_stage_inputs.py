"""Built inputs of the GCC stage tests (tests/test_gpu_gcc_stages.py, tests/test_gpu_tracks_stages.py): one file's float32 arrays, the
launch cells they are run at, and the padded device images.  The host half (host_file, CELLS) is plain NumPy, so that the CPU suite can
evaluate float64 scores of the same inputs (tests/test_tracks_stage_cases_host.py); torch is imported only where a device image is made.
Test infrastructure, not the product (never imported by the package)."""
import contextlib

import numpy as np

from oracle import gccnmf_oracle as O

# (F, D, S, K, T, batch, key 2, key 3) -> kernel per stage (angular | scores | reconstruction), from the launch rules of gcc.hip.
# k-tail = F % 16 == 1 (the scores' last bin as a rank-1 epilogue term); TAIL = F % 128 == 1 (the reconstruction's last row on the VALU).
CELLS = {
    (33, 3, 1, 16, 1, 1, 2, 1): 'ring | ring k-tail | ring',
    (65, 33, 2, 96, 5, 1, 1, 0): 'gemm<1,4> | gemm<1,4> k-tail | gemm<1,4>',
    (129, 129, 3, 129, 63, 1, 1, 1): 'gemm<4,1> | dma k-tail | gemm<1,4> TAIL',
    (201, 200, 4, 200, 65, 1, 1, 0): 'gemm<4,1> | gemm<4,1> | gemm<4,1>',
    (201, 64, 7, 1024, 3, 1, 1, 1): 'gemm<1,4> | dma | dma',
    (257, 128, 2, 128, 64, 1, 1, 0): 'gemm<1,4> | gemm<1,4> k-tail | gemm<4,1> TAIL',
    (513, 200, 3, 200, 130, 1, 1, 1): 'gemm<4,1> | dma k-tail | dma TAIL',
    (513, 33, 2, 1024, 5, 1, 1, 0): 'gemm<1,4> | gemm<4,1> k-tail | gemm<4,1> TAIL',
    (200, 128, 2, 16, 2, 1, 2, 1): 'ring | ring | ring',
    (257, 129, 4, 200, 5, 1, 2, 0): 'ring | ring k-tail | ring TAIL',
    (2049, 64, 3, 64, 3, 1, 2, 1): 'gemm<1,4> (n_fft 4096: no ring) | ring k-tail | ring TAIL',
    (2049, 200, 2, 129, 2, 1, 0, 1): 'gemm<4,1> (n_fft 4096: no ring) | ring k-tail | ring TAIL',
    (1025, 4096, 2, 128, 5, 1, 1, 1): 'gemm<4,1> | gemm<1,4> k-tail | dma TAIL',
    (201, 33, 3, 96, 65, 1, 0, 0): 'ring | ring | ring',
    (257, 128, 3, 200, 65, 9, 1, 1): 'gemm<1,4> | dma k-tail | dma TAIL',
    (513, 64, 2, 129, 5, 3, 2, 0): 'ring | ring k-tail | ring TAIL',
    (129, 33, 2, 96, 3, 64, 0, 1): 'ring | ring k-tail | ring TAIL',
}
CELL_IDS = ['F%d-D%d-S%d-K%d-T%d-b%d-tile%d-dma%d' % c for c in CELLS]


def cell_seed(F, K, b):
    """The seed of file b of a cell, as test_gcc_stages_against_float64 has always drawn it."""
    return 1000 * F + 10 * b + K


def host_file(F, T, K, D, S, seed):
    """One file's float32 inputs.  |X| in [0.5, 2]; C = its PHAT coherence with the Nyquist row x100; W, H in [0.01, 1] with W's
    Nyquist row and last atom x100 (the last reduction index of the scores and of the reconstruction); S distinct TDOA indexes."""
    rng = np.random.RandomState(seed)
    X = (rng.uniform(0.5, 2.0, (2, F, T)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (2, F, T)))).astype(np.complex64)
    Cc = O.spectralCoherence(X).astype(np.complex64)
    Cc[F - 1] *= np.float32(100)
    W = rng.uniform(0.01, 1.0, (F, K)).astype(np.float32)
    W[F - 1] *= np.float32(100)
    W[:, K - 1] *= np.float32(100)
    H = rng.uniform(0.01, 1.0, (K, 2 * T)).astype(np.float32)
    tdoa = np.sort(rng.choice(D, S, replace=False)).astype(np.int32)
    masks = rng.uniform(0.0, 1.0, (S, K, T)).astype(np.float32)
    return dict(X=X, V=np.abs(X).astype(np.float32), C=Cc, W=W, H=H, tdoa=tdoa, masks=masks)


@contextlib.contextmanager
def tuning(lib, tile_policy, dma):
    try:
        assert lib.gccnmf_set_tuning(2, tile_policy) == 0 and lib.gccnmf_set_tuning(3, dma) == 0
        yield
    finally:
        lib.gccnmf_set_tuning(2, 0)
        lib.gccnmf_set_tuning(3, 1)


def geometry(F, T, K, D):
    from gcc_nmf_amd.engine import Geometry
    return Geometry(F, T, K, D)


def upload(files, g, S):
    """Padded device images (zero padding, as the geometry requires) of a batch of host_file() dicts."""
    import torch
    B, F, T, K = len(files), g.F, g.T, g.K
    CC = np.zeros((B, 2, g.Fp, g.Tp), np.float32)
    W = np.zeros((B, g.Fp, g.Kp), np.float32)
    H = np.zeros((B, g.Kp, g.Np), np.float32)
    X = np.zeros((B, 2, g.Fp, g.Tp, 2), np.float32)
    V = np.zeros((B, g.Fp, g.Np), np.float32)
    M = np.zeros((B, S, g.Kp, g.Tp), np.float32)
    for b, f in enumerate(files):
        CC[b, 0, :F, :T], CC[b, 1, :F, :T] = f['C'].real, f['C'].imag
        W[b, :F, :K] = f['W']
        H[b, :K, :2 * T] = f['H']
        X[b, :, :F, :T, 0], X[b, :, :F, :T, 1] = f['X'].real, f['X'].imag
        V[b, :F, :T], V[b, :F, T:2 * T] = f['V'][0], f['V'][1]
        M[b, :, :K, :T] = f['masks']
    d = lambda a: torch.from_numpy(a).cuda()
    return dict(CC=d(CC), W=d(W), H=d(H), X=d(X), V=d(V), masks=d(M),
                tdoa=d(np.stack([f['tdoa'] for f in files]).astype(np.int32)))
