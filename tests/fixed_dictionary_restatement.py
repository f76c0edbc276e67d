"""NumPy float64 restatement of the fixed-dictionary KL-NMF call (gccnmf_klnmf with GCCNMF_FLAG_FIXED_W, csrc/nmf_fixed.hip), with a derived
per-element bar for every output: the reference for tests/test_fixed_dictionary_host.py and tests/test_gpu_fixed_dictionary.py.  Same
contract as klnmf_stages_restatement.py (S below), whose helpers this file uses: every function takes the float32 values the device held
BEFORE the call, widened to float64, and returns what the call must leave; a reference of exactly 0 demands exactly 0; S.share judges.

    prepare     den = colsum_f W + alpha + eps  (K,),   Wt = W^T            (the head of the workspace, written once per call)
    iteration   H <- H * (W^T (V / (W H))) / den                             (every iteration of the call inside ONE launch)

The launch shape follows from K alone (fixed_shape): the atoms are cut in Kb blocks of 32, a wave owns KB consecutive blocks, nw waves make
the workgroup.  The last wave may own fewer than KB blocks and the last block fewer than 32 atoms -- with at most 4 atoms, lane half 1 of the
block holds none.  SHAPES is the smallest table that reaches every such form.

THE BARS follow S's rule: u = 2^-24; every reduction is a sum of NON-NEGATIVE float32 terms, so a sum of m terms that each carry a relative
error of at most a u is within (a + m - 1) u of the exact sum relative to the sum itself, IN ANY ORDER, fused or not.  The per-wave partial
products of P, added in wave order, are still one sum of K non-negative terms: the argument holds unchanged.  Nothing here was fitted to a
device result."""
import numpy as np

import klnmf_stages_restatement as S
from klnmf_stages_restatement import low_rank_plus_noise, share, U24, ALPHA, EPS      # noqa: F401  (re-exported for the tests)

FIXED_W, H_ONES = 1 << 16, 1 << 17                          # GCCNMF_FLAG_* of include/gccnmf_hip.h
MAX_WAVES = 8


def _f64(*a):
    return [np.asarray(x, np.float64) for x in a]


# ---- the launch shape -------------------------------------------------------------------------------------------------------------------------
def fixed_shape(K):
    """-> (Kb, KB, nw): 32-atom blocks, blocks per wave, waves per workgroup."""
    Kb = (K + 31) // 32
    KB = (Kb + MAX_WAVES - 1) // MAX_WAVES
    nw = (Kb + KB - 1) // KB
    return Kb, KB, nw


def last_wave_blocks(K):
    """blocks the last wave owns (nblk of wave nw - 1): 1 ... KB"""
    Kb, KB, nw = fixed_shape(K)
    return Kb - (nw - 1) * KB


def last_block_atoms(K):
    """valid atoms of the last 32-atom block: 1 ... 32"""
    return K - 32 * (fixed_shape(K)[0] - 1)


# ---- the call ---------------------------------------------------------------------------------------------------------------------------------
def prepare(W, alpha=ALPHA, eps=EPS):
    """-> den (K,) float64, Wt (K, F) float32: the transposed copy is the dictionary's own bits."""
    W64, alpha, eps = _f64(W, alpha, eps)
    return W64.sum(0) + alpha + eps, np.ascontiguousarray(np.asarray(W, np.float32).T)


def iteration(V, W, H, alpha=ALPHA, eps=EPS):
    V, W, H = _f64(V, W, H)
    den, _ = prepare(W, alpha, eps)
    return H * (W.T @ (V / (W @ H))) / den[:, None]


def iterate(V, W, H, alpha, eps, iterations):
    for _ in range(iterations):
        H = iteration(V, W, H, alpha, eps)
    return np.asarray(H, np.float64)


# ---- the bars (each: a multiple of u, relative to the element's own reference) ---------------------------------------------------------------
def bar_den(F):
    """den: the column sum's F - 1 additions, + alpha (1), + eps (1) = F + 1 (alpha, eps >= 0: still a sum of non-negative terms);
    + 2 spare = S.bar_colsum0(F) + 2."""
    return S.bar_colsum0(F) + 2 * U24


def bar_iteration(F, K):
    """H after one iteration.  P = W.H: K products (1 each, or 0 fused) and K - 1 additions, the division v / p (1) = K + 1 on every r
    (S.bar_R's K + 4 covers it: there is no lazy scale here, that rounding is one more spare).  U = W^T.r: F products and F - 1 additions
    = F, on terms that carry r's error alike: F + K + 4.  den: F - 1 additions of exact terms and 2 spare (S.bar_colsum0 = F + 1), then
    + alpha, + eps (2).  h * (u / den): the division and the product (2; S.bar_H counts 3 and the unused s * h 1: 2 more spare).
    In all S.bar_H(F, K) + S.bar_colsum0(F) = (F + 8 + K + 4) + (F + 1) = 2 F + K + 13: the fused composition's count is fused12's, plus
    the column sum, which is formed inside the call here and not read from memory.  Dividing by a den that is e off moves the quotient by
    e (1 + O(e))."""
    return S.bar_H(F, K) + S.bar_colsum0(F)


# ---- the shapes (F, K, N, files): tests/test_fixed_dictionary_host.py shows what the table reaches --------------------------------------------
SHAPES = [
    (2, 1, 1, 1),          # the smallest call: one atom, one frame, one wave
    (33, 33, 32, 2),       # Np = 64: the second column tile is a pure padding tile; the last block holds one atom
    (34, 70, 35, 1),       # nw = 3
    (17, 100, 9, 2),       # nw = 4, the last block 4 atoms at KB = 1: lane half 1 empty
    (31, 256, 33, 1),      # KB = 1 at its largest: eight full waves
    (65, 257, 77, 3),      # KB = 2, last wave nblk = 1, one atom
    (64, 300, 70, 2),      # KB = 2, full waves
    (33, 512, 65, 1),      # KB = 2 at its largest
    (65, 516, 40, 2),      # KB = 3, nw = 6, last wave nblk = 2, last block 4 atoms: lane half 1 empty
    (40, 600, 64, 1),      # KB = 3, nw = 7, last wave nblk = 1
    (33, 768, 33, 1),      # KB = 3 at its largest
    (65, 770, 70, 2),      # KB = 4 (no prefetch), nw = 7, last wave nblk = 1, two atoms
    (33, 1000, 40, 1),     # KB = 4, eight waves, the last block 8 atoms
    (129, 1024, 33, 1),    # the largest dictionary
    (513, 64, 77, 3),      # the workload's F
]


# ---- the problems ---------------------------------------------------------------------------------------------------------------------------
def dead_atom(K):
    """the all-zero atom of the dictionary (its row of H comes out exactly 0), never atom K - 1; None for K < 3"""
    return K // 2 if K >= 3 else None


def h_zeros(K, N, b):
    """(atom, frame) of the exact zeros of file b's H0; none for K < 8 (every column of W.H0 keeps positive terms)"""
    return [((5 + 11 * i) % K, (3 + 7 * i + b) % N) for i in range(3)] if K >= 8 else []


def problem(F, N, K, files, frame=False):
    """-> V (files, F, N), W (F, K), H0 (files, K, N): float32, read-only.  File b is the same problem whatever `files` is.
    V: low rank plus noise with isolated exact zeros (none where F < 8: they would be most of a frame) and one silent bin per file
    at S.zero_lines' row; frame=True adds S.zero_lines' silent frame (N >= 8) -- for ONE iteration only: that column of H is exactly 0
    afterwards and a second iteration divides 0 by 0 there, in the reference too.
    W: ONE positive dictionary, row F - 1 and atom K - 1 scaled by 100 (a dropped tail shows), atom dead_atom(K) all zero.
    H0: positive with the exact zeros of h_zeros."""
    rng = np.random.RandomState(F * 7 + N * 3 + K)
    W = (rng.rand(F, K) + 0.01).astype(np.float32)
    W[F - 1, :] *= 100
    W[:, K - 1] *= 100
    if dead_atom(K) is not None:
        W[:, dead_atom(K)] = 0
    V = np.stack([low_rank_plus_noise(F, N, 5, 0.3, F + N + 17 * b, 5 if F >= 8 else 0) for b in range(files)])
    H0 = np.stack([(np.random.RandomState(1000 + F + N + K + 31 * b).rand(K, N) + 0.01).astype(np.float32) for b in range(files)])
    for b in range(files):
        f0, n0 = S.zero_lines(F, N, b)
        V[b, f0, :] = 0
        if frame and n0 is not None:
            V[b, :, n0] = 0
        for k, n in h_zeros(K, N, b):
            H0[b, k, n] = 0
    for a in (V, W, H0):
        a.flags.writeable = False
    return V, W, H0
