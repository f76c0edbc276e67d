"""NumPy float64 restatement of ONE Itakura-Saito (beta = 0) / Kullback-Leibler (1) / Euclidean (2) NMF iteration, stage by stage as
gccnmf_klnmf_stage cuts it with GCCNMF_FLAG_DIVERGENCE_* (include/gccnmf_hip.h), with a derived per-element bar for every output: the
reference for tests/test_beta_nmf_host.py and tests/test_gpu_beta_nmf.py.  Same contract as klnmf_stages_restatement.py (S below), whose
helpers this file uses: every function takes the float32 values the device held BEFORE the stage, widened to float64, and returns what the
stage must leave.

    stage 0   colsumW = sum_f W,  s = 1,  R = Q = 0                                   (S.stage0)
    stage 1   P = W . (s * H);   IS: Q = 1 / P, R = V Q Q    KL: Q = 1, R = V / P    Euclid: Q = P, R = V
    stage 2   H <- (s * H) * (W^T . R) / (W^T . Q + alpha + eps)
    stage 3   stage 1 with s = 1
    stage 4   Un = R . H^T,  Ud = Q . H^T
    stage 5   Wt = W * (Un / Ud),  s = sqrt(sum_f Wt^2),  W = Wt / s,  colsumW = sum_f W
    stage 6   H *= s                                                                  (S.stage6: float32, exact)

At beta = 1, W^T . Q = colsumW and Q . H^T = rowsumH in every row: the stages are klnmf_stages_restatement's (test_beta_nmf_host.py).

THE BARS follow S's rule: u = 2^-24; every reduction is a sum of NON-NEGATIVE float32 terms, so a sum of m terms that each carry a relative
error of at most a u is within (a + m - 1) u of the exact sum relative to the sum itself, in any order, fused or not; a bar is the roundings
on the longest path to the element plus the stated element-wise operations, times u, times the element's own float64 reference, and a
reference of exactly 0 demands exactly 0.  Each constant holds 2 spare roundings for the second-order terms.  The counts are stated at each
bar function; nothing here was fitted to a device result."""
import numpy as np

import klnmf_stages_restatement as S
from klnmf_stages_restatement import low_rank_plus_noise, share, U24, ALPHA, EPS      # noqa: F401  (re-exported for the tests)

IS, KL, EUCLIDEAN = 0, 1, 2
NAMES = {IS: 'is', KL: 'kl', EUCLIDEAN: 'euclidean'}
FLAGS = {IS: 1 << 26, KL: 0, EUCLIDEAN: 2 << 26}          # GCCNMF_FLAG_DIVERGENCE_* of include/gccnmf_hip.h


def _f64(*a):
    return [np.asarray(x, np.float64) for x in a]


# ---- the stages ---------------------------------------------------------------------------------------------------------------------------
def stage13(V, W, H, s, beta):
    """stage 1 (s = the lazy scale) and stage 3 (s = None) -> R, Q"""
    V, W, H = _f64(V, W, H)
    P = W @ (H if s is None else np.asarray(s, np.float64)[:, None] * H)
    if beta == IS:
        Q = 1.0 / P
        return V * Q * Q, Q
    if beta == KL:
        return V / P, np.ones_like(P)
    return V.copy(), P


def stage2(W, H, s, R, Q, alpha=ALPHA, eps=EPS):
    W, H, s, R, Q, alpha, eps = _f64(W, H, s, R, Q, alpha, eps)
    return (s[:, None] * H) * (W.T @ R) / (W.T @ Q + alpha + eps)


def stage4(R, Q, H):
    """-> Un, Ud"""
    R, Q, H = _f64(R, Q, H)
    return R @ H.T, Q @ H.T


def stage5(W, Un, Ud):
    """-> W, s, colsumW"""
    W, Un, Ud = _f64(W, Un, Ud)
    Wt = W * (Un / Ud)
    s = np.sqrt((Wt * Wt).sum(0))
    Wn = Wt / s
    return Wn, s, Wn.sum(0)


def iterate(V, W, H, beta, alpha, eps, iterations):
    """`iterations` whole iterations in float64 from the given factors (the H a caller sees: the scale is materialised every iteration,
    which in exact arithmetic is what the lazy scale computes)."""
    V, W, H = _f64(V, W, H)
    one = np.ones(W.shape[1])
    for _ in range(iterations):
        H = stage2(W, H, one, *stage13(V, W, H, None, beta), alpha=alpha, eps=eps)
        R, Q = stage13(V, W, H, None, beta)
        W, s, _ = stage5(W, *stage4(R, Q, H))
        H = H * s[:, None]
    return W, H


def divergence(V, W, H, beta):
    """float64 D_beta(V || W.H).  IS: sum over V > 0 of V / R - log(V / R) - 1 (a zero of V contributes nothing: IS is +infinity there);
    KL: sum V log(V / R) - V + R (a zero of V contributes R); Euclid: sum (V - R)^2 / 2."""
    V, W, H = _f64(V, W, H)
    R = W @ H
    pos = V > 0
    if beta == IS:
        q = V[pos] / R[pos]
        return float((q - np.log(q) - 1.0).sum())
    if beta == KL:
        logs = np.zeros_like(V)
        logs[pos] = V[pos] * np.log(V[pos] / R[pos])
        return float((logs - V + R).sum())
    return float((0.5 * (V - R) ** 2).sum())


def divergence_bar(V, W, H, beta):
    """The absolute bar on a float32-GEMM evaluation of D_beta against `divergence` on the same float32 factors, derived as
    kl_divergence_restatement.value_bar derives KL's (8 + K) u sum(V + R): the GEMM's worst-case error K u R in R moves a term by
    |dD/dR| K u R, and |dD/dR| R is |R - V| <= V + R for KL, |R - V| / R <= (V + R) / R for IS, R |R - V| <= (V + R)^2 for Euclid; the
    handful of element-wise float32 roundings (the 8) are each relative to a quantity of at most that size.  So the bar is
    (8 + K) u sum w (V + R) with the weight w = 1 (KL), 1 / R over V > 0 (IS), V + R (Euclid)."""
    V, W, H = _f64(V, W, H)
    R = W @ H
    if beta == IS:
        pos = V > 0
        weight = float(((V[pos] + R[pos]) / R[pos]).sum())
    elif beta == KL:
        weight = float((V + R).sum())
    else:
        weight = float(((V + R) ** 2).sum())
    return (8 + W.shape[1]) * U24 * weight


# ---- the bars (each: a multiple of u, relative to the element's own reference) ---------------------------------------------------------------
def bar_Q(K):
    """stages 1 and 3, Q: s * h (1), the product with w (1, or 0 fused), K - 1 additions = K + 1 on P; IS: the reciprocal (1) = K + 2 (Euclid:
    Q = P, one fewer); + 2 spare."""
    return (K + 4) * U24


def bar_R(K, beta):
    """stages 1 and 3, R.  IS: R = (V * Q) * Q -- Q's K + 2 twice and the two products = 2 K + 6; + 2 spare.  Euclid: R is V, exactly: 0."""
    return (2 * K + 8) * U24 if beta == IS else 0.0


def bar_H(F):
    """stage 2: the numerator's F products (1 each) and F - 1 additions = F; the denominator's likewise F, + alpha (1), + eps (1) = F + 2
    (alpha, eps >= 0: still a sum of non-negative terms); the quotient (1), s * h (1), the product of the two (1) = 2 F + 5; + 2 spare."""
    return (2 * F + 7) * U24


def bar_U(N):
    """stage 4, Un and Ud alike: N products (1 each), N - 1 additions = N; + 2 spare."""
    return S.bar_U(N)


def bar_s(F):
    """stage 5 s: Wt = W * (Un / Ud) carries 2 (the quotient, the product: Un and Ud are read from memory), then as S.bar_s."""
    return S.bar_s(F)


def bar_W(F):
    return S.bar_W(F)


def bar_colsumW(F):
    return S.bar_colsumW(F)


def trajectory_bars(beta, F, N, K, iterations):
    """(bar of W, bar of H) after `iterations` whole iterations from exact initial factors: the per-stage counts above carried along to first
    order.  e_X is the relative error of X in units of u.  A product or quotient adds its operands' errors and its own rounding; a sum of
    non-negative terms carries the largest error among its terms plus its own count; sqrt halves.  Per iteration (s = 1: H is materialised,
    which adds the rounding of stage 6 where the device's lazy scale adds the same one in s * h):
        P: e_W + e_H + K + 1     IS: Q = P + 1, R = 2 Q + 2     Euclid: Q = P, R = 0
        H' = e_H + (e_W + e_R + F) + (e_W + e_Q + F + 2) + 3
        P', Q', R' from (W, H') likewise
        Un = e_R' + e_H' + N,  Ud = e_Q' + e_H' + N,  Wt = e_W + e_Un + e_Ud + 2
        s = e_Wt + F / 2 + 1,  W' = e_Wt + e_s + 1,  H'' = e_H' + e_s + 1
    + 2 spare at the end.  Valid while the result times u stays far below 1 (the callers assert it)."""
    def pqr(eW, eH):
        eP = eW + eH + K + 1
        return (2 * (eP + 1) + 2, eP + 1) if beta == IS else (0.0, eP)
    eW = eH = 0.0
    for _ in range(iterations):
        eR, eQ = pqr(eW, eH)
        eH = eH + (eW + eR + F) + (eW + eQ + F + 2) + 3
        eR, eQ = pqr(eW, eH)
        eWt = eW + (eR + eH + N) + (eQ + eH + N) + 2
        es = eWt + F / 2.0 + 1
        eW, eH = eWt + es + 1, eH + es + 1
    return (eW + 2) * U24, (eH + 2) * U24


# ---- the shapes and problems of tests/test_gpu_beta_nmf.py ---------------------------------------------------------------------------------
SHAPES = [(33, 70, 16, 1), (129, 130, 40, 3), (130, 70, 136, 2), (513, 140, 128, 2)]      # (F, N, K, batch): the issue's table


def problem(F, N, K, files):
    """S.problem without the all-zero bin and frame (isolated exact zeros stay): a silent frame's column of H is exactly 0 after stage 2,
    and IS's 1 / P would be 1 / 0 there -- the reference iteration does the same (test_beta_nmf_host.py shows it)."""
    return S.problem(F, N, K, files, lines=False)
