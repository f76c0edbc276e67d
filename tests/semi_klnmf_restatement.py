"""NumPy restatement of ONE semi-supervised KL-NMF iteration (GCCNMF_FLAG_FREE_ATOMS in include/gccnmf_hip.h), built from the stage
functions of klnmf_stages_restatement.py: stages 0-3 and 6 are the blind call's, stages 4 and 5 touch the free atoms -- the LAST n columns
of W, the last n rows of H -- alone.  The reference of tests/test_semi_klnmf_host.py and tests/test_gpu_semi_klnmf.py, with the shape
table they share.

    W = [ W_fixed (F x K_fixed) | W_free (F x n) ],  K = K_fixed + n
    stage 4   U[:, K_fixed:] = R . H[K_fixed:]^T,   rowsumH[K_fixed:] = sum_n H[K_fixed:]
    stage 5   Wt = W_free * (U_free / rowsumH_free),  s_free = sqrt(sum_f Wt^2),  W_free = Wt / s_free,  colsumW_free = sum_f W_free
    everything that belongs to a fixed atom -- its column of W and of U, rowsumH, s (1), colsumW (stage 0's) -- keeps its bits.

The bars are klnmf_stages_restatement's (bar_U, bar_rowsumH, bar_s, bar_W, bar_colsumW): the free-only stages do the same arithmetic per
element as the blind ones, on fewer columns."""
import numpy as np

import klnmf_stages_restatement as S

# (F, N, K_fixed, n, batch): the smallest shapes at which the free-atom kernels can go wrong
#   (513, 65, 64, 16, 2)     the tail bin band (F = 16 * 32 + 1), a third column chunk of one column, half an atom block
#   (513, 130, 128, 1, 3)    one free atom; five column chunks: wave 0 takes two, the last chunk has two columns
#   (129, 1, 16, 17, 1)      one column (three waves idle), n = 16 + 1 (a second W-update group with one atom), one file
#   (40, 65, 16, 33, 9)      Fp > F and F no multiple of 32, two atom blocks with one atom in the second, batch 9
#   (641, 96, 64, 128, 2)    the most free atoms (four blocks), F > 576
#   (513, 70, 1008, 16, 1)   K = Kp = 1024: the free block ends at the last padded atom (nothing to read behind it)
#   (2049, 77, 64, 32, 1)    the most bins; exactly one atom block
SHAPES = [(513, 65, 64, 16, 2), (513, 130, 128, 1, 3), (129, 1, 16, 17, 1), (40, 65, 16, 33, 9), (641, 96, 64, 128, 2),
          (513, 70, 1008, 16, 1), (2049, 77, 64, 32, 1)]


def FREE_ATOMS(n):
    """GCCNMF_FLAG_FREE_ATOMS(n) of include/gccnmf_hip.h"""
    return n << 18


def problem(F, N, Kf, n, files, silent_frame=True):
    """klnmf_stages_restatement.problem at K = Kf + n (zero row and column included), with the last bin, the last free atom and the
    last fixed atom made large so that a dropped one shows: W's last row and its columns Kf - 1 and K - 1, H's rows Kf - 1 and K - 1
    are scaled by 4.  float32, read-only.  silent_frame=False keeps the silent bin but not the silent frame: a WHOLE iteration divides
    0 by 0 in an all-zero column of V (the H update makes the column of H zero, and the reference's own second quotient is then NaN;
    tests/test_klnmf_stages_host.py shows it), so the whole-iteration checks run without one."""
    V, W, H, s = S.problem(F, N, Kf + n, files, lines=silent_frame)
    W, H = W.copy(), H.copy()
    if not silent_frame:
        V = V.copy()
        for b in range(files):
            V[b, S.zero_lines(F, N, b)[0], :] = 0
        V.flags.writeable = False
    W[:, F - 1, :] *= 4
    for k in (Kf - 1, Kf + n - 1):
        W[:, :, k] *= 4
        H[:, k, :] *= 4
    for a in (W, H):
        a.flags.writeable = False
    return V, W, H, s


def stage4_free(R, H, n, dtype=np.float64):
    """-> U_free (F, n), rowsumH_free (n,)"""
    R, H = np.asarray(R, dtype), np.asarray(H, dtype)
    return R @ H[-n:].T, H[-n:].sum(1)


def stage5_free(W, U_free, rowsum_free, n, dtype=np.float64):
    """-> W_free (F, n), s_free (n,), colsumW_free (n,)"""
    Wf, U, rs = np.asarray(W, dtype)[:, -n:], np.asarray(U_free, dtype), np.asarray(rowsum_free, dtype)
    Wt = Wf * (U / rs)
    s = np.sqrt((Wt * Wt).sum(0))
    Wn = Wt / s
    return Wn, s, Wn.sum(0)


def iteration(V, W, H, n, alpha=S.ALPHA, eps=S.EPS, dtype=np.float64):
    """One whole iteration from materialised factors (s = 1) to materialised factors: -> W, H.  In `dtype` throughout (float64: the
    reference; float32: what NumPy itself reaches in the device's precision)."""
    V, W, H = (np.asarray(a, dtype) for a in (V, W, H))
    alpha, eps = dtype(alpha), dtype(eps)
    H = H * (W.T @ (V / (W @ H))) / (W.sum(0) + alpha + eps)[:, None]
    R = V / (W @ H)
    U, rs = R @ H[-n:].T, H[-n:].sum(1)
    Wt = W[:, -n:] * (U / rs)
    s = np.sqrt((Wt * Wt).sum(0))
    W, H = W.copy(), H.copy()
    W[:, -n:] = Wt / s
    H[-n:] *= s[:, None]
    return W, H


def iteration_bars(F, N, K):
    """Per-element bars (relative, in units of 1: multiples of u) of ONE whole iteration from materialised float32 factors, compounded
    from the stage bars to first order -- every reduction is a sum of non-negative terms, so a relative error of its terms is a relative
    error of the sum.  In units of u:
        H after stage 2 (either form)      eH  = F + 8 + K + 4                               bar_H(F, K)
        R of stage 3                       eR  = eH + K + 4                                  the denominator moves by eH, + bar_R(K)
        U_free, rowsumH_free               eU  = eR + eH + N + 2,   ers = eH + N + 1         terms r * h, + bar_U(N) / bar_rowsumH(N)
        Wt = w * (u / rowsum)              eWt = eU + ers + 2
        s                                  es  = eWt + F / 2 + 2                             as bar_s
        W_free = Wt / s                    eW  = eWt + es + 1, + 2 spare
        H of a fixed atom                  eH;      H of a free atom = h * s: eH + es + 1, + 2 spare
    -> dict(W_free=, H_fixed=, H_free=).  The second-order terms are below 1e-3 of these at every shape in use."""
    eH = F + 8 + K + 4
    eR = eH + K + 4
    eU, ers = eR + eH + N + 2, eH + N + 1
    eWt = eU + ers + 2
    es = eWt + F / 2.0 + 2
    return dict(W_free=(eWt + es + 3) * S.U24, H_fixed=eH * S.U24, H_free=(eH + es + 3) * S.U24)


def run(V, W, H, n, iterations, alpha=S.ALPHA, eps=S.EPS, dtype=np.float64, trace=None):
    """`iterations` iterations; trace: a list that receives the KL divergence after each."""
    for _ in range(iterations):
        W, H = iteration(V, W, H, n, alpha, eps, dtype)
        if trace is not None:
            trace.append(divergence(V, W, H))
    return W, H


def run_fixed(V, W, H, iterations, alpha=S.ALPHA, eps=S.EPS, dtype=np.float64):
    """The fixed-dictionary iteration (H alone) for comparison."""
    V, W, H = (np.asarray(a, dtype) for a in (V, W, H))
    den = (W.sum(0) + dtype(alpha) + dtype(eps))[:, None]
    for _ in range(iterations):
        H = H * (W.T @ (V / (W @ H))) / den
    return H


def divergence(V, W, H):
    V, W, H = (np.asarray(a, np.float64) for a in (V, W, H))
    R = W @ H
    nz = V > 0
    return float((V[nz] * np.log(V[nz] / R[nz])).sum() - V.sum() + R.sum())


def unseen_noise_problem(F=129, N=200, Kf=64, outside=4, seed=3):
    """The construction of DESIGN section 2c: a 64-atom make_rt_dictionary(3, 129, 64), V = dictionary content plus `outside` spectra the
    dictionary does not hold.  -> V (F, N), Wfix (F, Kf), float64."""
    from oracle.rt_oracle import make_rt_dictionary
    Wfix = np.asarray(make_rt_dictionary(3, F, Kf), np.float64)
    rng = np.random.RandomState(seed)
    Hd = rng.rand(Kf, N) * (rng.rand(Kf, N) < 0.2)
    Wn = rng.rand(F, outside) ** 4 * 3 + 0.01
    Hn = rng.rand(outside, N) + 0.1
    return Wfix @ Hd + Wn @ Hn + 1e-3, Wfix
