"""NumPy float64 restatement of ONE KL-NMF iteration, stage by stage as gccnmf_klnmf_stage cuts it (include/gccnmf_hip.h), with a derived
per-element bar for every output: the reference for tests/test_klnmf_stages_host.py and tests/test_gpu_klnmf_stages.py.

State of one file: V (F, N), W (F, K), H (K, N), the lazy atom scale s (K,) -- `hscale`: the H the algorithm means is s * H until stage 6
materialises it --, R (F, N), U (F, K), rowsumH (K,), colsumW (K,).  Every function takes the float32 values the device held BEFORE the
stage (they are widened to float64 here) and returns what the stage must leave, so a comparison never sees rounding of an earlier stage.

    stage 0   colsumW = sum_f W,  s = 1,  R = 0
    stage 1   R = V / (W . (s * H))
    stage 2   H <- (s * H) * (W^T . R) / (colsumW + alpha + eps)
    stage 3   R = V / (W . H)
    stage 4   U = R . H^T,  rowsumH = sum_n H
    stage 5   Wt = W * (U / rowsumH),  s = sqrt(sum_f Wt^2),  W = Wt / s,  colsumW = sum_f W
    stage 6   H *= s                                   (float32: the one stage whose result is exact)

Launch forms that do not materialise an intermediate are compositions: fused12 = stage 2 o stage 1, fused34 = stage 4 o stage 3,
fused_w = stage 5 o stage 4.

THE BARS.  u = 2^-24 is the unit round-off of float32.  Every reduction here is a sum of NON-NEGATIVE float32 terms, so there is no
cancellation: if each term carries a relative error of at most a * u and m - 1 additions follow, the float32 sum -- in any order, with
products fused into the additions or not -- is within (a + m - 1) * u (1 + O(m u)) of the exact sum, RELATIVE TO THE SUM ITSELF.  A bar is
therefore `roundings on the longest path to the element` + a constant for the element-wise operations behind it, times u, times the
element's own float64 reference; a reference of exactly 0 (a silent bin or frame of V) demands exactly 0.  The O(m u) second-order term is
below 1e-4 of the bar at every size in use and is covered by the constant (each constant holds 2 spare roundings).  The counts are stated at
each bar function."""
import numpy as np

from kl_divergence_restatement import low_rank_plus_noise

U24 = 2.0 ** -24
ALPHA, EPS = np.float32(0.05), np.float32(1e-16)


def _f64(*a):
    return [np.asarray(x, np.float64) for x in a]


# ---- the stages ---------------------------------------------------------------------------------------------------------------------------
def stage0(W):
    """-> colsumW, s (R, all zero, is the caller's to state)."""
    W, = _f64(W)
    return W.sum(0), np.ones(W.shape[1])


def stage1(V, W, H, s):
    V, W, H, s = _f64(V, W, H, s)
    return V / (W @ (s[:, None] * H))


def stage2(W, H, s, R, colsumW, alpha=ALPHA, eps=EPS):
    W, H, s, R, colsumW, alpha, eps = _f64(W, H, s, R, colsumW, alpha, eps)
    return (s[:, None] * H) * (W.T @ R) / (colsumW + alpha + eps)[:, None]


def stage3(V, W, H):
    V, W, H = _f64(V, W, H)
    return V / (W @ H)


def stage4(R, H):
    """-> U, rowsumH"""
    R, H = _f64(R, H)
    return R @ H.T, H.sum(1)


def stage5(W, U, rowsumH):
    """-> W, s, colsumW"""
    W, U, rowsumH = _f64(W, U, rowsumH)
    Wt = W * (U / rowsumH)
    s = np.sqrt((Wt * Wt).sum(0))
    Wn = Wt / s
    return Wn, s, Wn.sum(0)


def stage6(H, s, dtype=np.float32):
    """float32 by default: H * s is one rounding per element, so the device's result is THIS array bit for bit."""
    return np.asarray(H, dtype) * np.asarray(s, dtype)[:, None]


def fused12(V, W, H, s, colsumW, alpha=ALPHA, eps=EPS):
    return stage2(W, H, s, stage1(V, W, H, s), colsumW, alpha, eps)


def fused34(V, W, H):
    return stage4(stage3(V, W, H), H)


def fused_w(W, R, H):
    return stage5(W, *stage4(R, H))


# ---- the bars (each: a multiple of u, relative to the element's own reference) ---------------------------------------------------------------
def bar_colsum0(F):
    """stage 0 colsumW: F exact terms, F - 1 additions; + 2 spare."""
    return (F + 1) * U24


def bar_R(K):
    """stages 1 and 3: s * h (1), the product with w (1, or 0 when fused into the accumulation), K - 1 additions, the division (1) = K + 2;
    + 2 spare.  Division by a denominator that is (K + 1) u off moves the quotient by the same relative amount."""
    return (K + 4) * U24


def bar_H(F, K=None):
    """stage 2: the F products w * r (1 each) and F - 1 additions = F; s * h (1); colsumW + alpha + eps (2); the reciprocal or division (1) and
    the two products that join the three factors (2) = F + 6; + 2 spare.
    fused12 (K given): r is not read from memory but carries bar_R(K) itself, on every (non-negative) term alike: + K + 4."""
    return (F + 8 + (0 if K is None else K + 4)) * U24


def bar_U(N, K=None):
    """stage 4 U: N products (1 each), N - 1 additions = N; + 2 spare.  fused34 (K given): r carries bar_R(K): + K + 4."""
    return (N + 2 + (0 if K is None else K + 4)) * U24


def bar_rowsumH(N):
    """stage 4 rowsumH: N exact terms, N - 1 additions; + 2 spare."""
    return (N + 1) * U24


def _wt_roundings(N):
    """relative error of Wt = W * (U / rowsumH) in units of u: the division and the product (2), and, where U and rowsumH are not read from
    memory (the W update in the epilogue of R.H^T, N given), their own bars on top."""
    return 2 + (0 if N is None else (N + 2) + (N + 1))


def bar_s(F, N=None):
    """stage 5 s: with e = _wt_roundings, every Wt^2 is within 2 e + 1 (its own rounding; 0 when fused), F - 1 additions: the sum is within
    2 e + F; sqrt(x (1 + d)) = sqrt(x) (1 + d / 2 + O(d^2)), so the square root halves that, and it rounds once: e + F / 2 + 1; + 1 spare."""
    return (_wt_roundings(N) + F / 2.0 + 2) * U24


def bar_W(F, N=None):
    """stage 5 W = Wt / s: e (Wt) + e + F / 2 + 1 (s) + the division (1) = 2 e + F / 2 + 2; + 2 spare."""
    return (2 * _wt_roundings(N) + F / 2.0 + 4) * U24


def bar_colsumW(F, N=None):
    """stage 5 colsumW: F terms each within bar_W, F - 1 additions: bar_W + F (3 F / 2 + 8 where U and rowsumH are read from memory)."""
    return bar_W(F, N) + F * U24


# ---- the shapes of tests/test_gpu_klnmf_stages.py (the host file shows that float32 NumPy passes the bars at every one of them) ----------------
DIRECT_SHAPES = [(513, 70, 65), (145, 1, 1), (17, 64, 64), (40, 65, 17)]
THROUGHPUT_SHAPES = [(513, 96, 65), (513, 97, 65), (641, 96, 70), (200, 130, 130)]
SHORT_SHAPES = [(129, 65, 20), (513, 1, 128), (513, 130, 128), (257, 64, 33), (129, 65, 33)]
UPDATE_W_SHAPES = [(513, 16, 50), (40, 16, 50)]
DMA_UPDW_SHAPE = (513, 96, 128)          # Fm a multiple of 128 and K of 64: the one shape class whose fused W update runs in the LDS-DMA kernel
# the smallest shapes chain_capable (csrc/nmf.hip) admits -- F in {257, 385, 513}, K a multiple of 128 from 256 on -- on the PLAIN launches the chained
# ones are pinned to bit for bit (tests/test_gpu_chained_small_shapes.py):
#   (257, 70, 256)  K2's outputs are 256 rows: half-height tiles; Fm = 256: two row blocks of the fused W update, four atom tiles
#   (385, 96, 384)  K2 of 384 rows: one full-height row tile with an idle wave; Fm = 384; the last column tile has exactly 32 columns (the narrow item)
#   (513, 33, 640)  two row tiles of K2, the second a quarter full; ten atom tiles of the W update; ONE column tile; K1 / K3 reduce over 640
CHAIN_SHAPES = [(257, 70, 256), (385, 96, 384), (513, 33, 640)]
ALL_SHAPES = DIRECT_SHAPES + THROUGHPUT_SHAPES + SHORT_SHAPES + UPDATE_W_SHAPES + [DMA_UPDW_SHAPE] + CHAIN_SHAPES
NO_XCD_AFFINITY, UNFUSED_W_UPDATE = 1, 2                    # GCCNMF_FLAG_* of include/gccnmf_hip.h


def throughput_cases():
    """(F, N, K, batch, flags, key 3, key 9) of the throughput-tile cases.  The knobs: key 3 in {1, 0} (LDS-DMA | register staging), key 9 in
    {0, 1, 2, 3} (full | by the launcher's cost model | narrow halves | half-height), the batch in {2, 9} (9: the XCD-affine block map of
    batch >= 8), flags in {0, no XCD affinity, unfused W update}.  Key 9 is read by the LDS-DMA launcher alone (gemm_dma.h), so its four
    values mean something only with key 3 = 1: every shape runs all four there, and once with key 3 = 0 (key 9 at its default).  The batch
    and the flags rotate over those five runs -- run r of shape i takes batch[(i + r) mod 2] and flags[(i + r) mod 3] -- so every value of
    either occurs with every shape; not the cross product (48 runs per shape).  tests/test_klnmf_stages_host.py checks the table."""
    cases = []
    for i, shape in enumerate(THROUGHPUT_SHAPES):
        for r, (dma, split) in enumerate([(1, 0), (1, 1), (1, 2), (1, 3), (0, 1)]):
            cases.append(shape + ((2, 9)[(i + r) % 2], (0, NO_XCD_AFFINITY, UNFUSED_W_UPDATE)[(i + r) % 3], dma, split))
    return cases


# ---- the problems --------------------------------------------------------------------------------------------------------------------------
def zero_lines(F, N, b):
    """(row, column) of file b's all-zero bin and frame: never bin F - 1 or the last frame -- those are the elements the kernels treat
    apart, and an exact zero there would hide them.  column is None for N < 8 (a zero frame would be most, or all, of V)."""
    return (F // 3 + 7 * b) % (F - 1), ((N // 2 + 3 * b) % (N - 1) if N >= 8 else None)


def problem(F, N, K, files, lines=True, frames=True):
    """`files` independent problems: V (files, F, N) low rank plus noise with isolated exact zeros and, with `lines`, one all-zero row and --
    unless `frames` is off -- one all-zero column per file (zero_lines); W (files, F, K), H (files, K, N) positive; s (files, K) in
    [0.5, 2) -- the lazy scale a stage-1 / stage-2 launch meets in every iteration but the first.  float32, read-only.
    frames=False is for callers that cannot restore H between the H update and stage 3 (the shared-dictionary step A,
    tests/shared_protocol_restatement.py): a silent frame's column of H is exactly 0 after stage 2 and stage 3 divides 0 by 0 there."""
    rng = np.random.RandomState(F * 7 + N * 3 + K)
    V = np.stack([low_rank_plus_noise(F, N, 5, 0.3, F + N + 17 * b) for b in range(files)])
    if lines:
        for b in range(files):
            f0, n0 = zero_lines(F, N, b)
            V[b, f0, :] = 0
            if frames and n0 is not None:
                V[b, :, n0] = 0
    W = (rng.rand(files, F, K) + 0.01).astype(np.float32)
    H = (rng.rand(files, K, N) + 0.01).astype(np.float32)
    s = (0.5 + 1.5 * rng.rand(files, K)).astype(np.float32)
    for a in (V, W, H, s):
        a.flags.writeable = False
    return V, W, H, s


def share(got, ref, bar):
    """(worst |got - ref| / (bar |ref|) over the elements with ref != 0, index of the first element that misses or None).  An element whose
    reference is exactly 0 must be exactly 0; NaN and Inf always miss."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err, lim = np.abs(got - ref), bar * np.abs(ref)
    bad = ~(err <= lim)
    nz = ref != 0
    worst = float((err[nz] / lim[nz]).max()) if nz.any() else 0.0
    return worst, (tuple(int(i) for i in np.argwhere(bad)[0]) if bad.any() else None)
