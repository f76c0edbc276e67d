"""NumPy float64 restatement of the temporal-continuity KL-NMF iteration (gccnmf_klnmf / gccnmf_klnmf_stage with GCCNMF_FLAG_CONTINUITY,
include/gccnmf_hip.h; csrc/nmf_smooth.hip), with a derived per-element bar for every output of the new stage: the reference for
tests/test_temporal_continuity_host.py and tests/test_gpu_temporal_continuity.py.  Same contract as klnmf_stages_restatement.py (S below),
whose stages 0, 1, 3, 4, 5 and 6 -- and their bars -- are this iteration's: every function takes the float32 values the device held BEFORE
the stage, widened to float64, and returns what the stage must leave.

The columns are `segments` equal runs of T = N / segments frames; per atom and segment, with h = s * H:

    E = sum_t h_t^2        D = sum_{t >= 1} (h_t - h_{t-1})^2        cost c = T D / E
    Gp_t = 2 T n_t h_t / E                                   n_t = the neighbours inside the segment (2, at the ends 1, T = 1: 0)
    Gm_t = 2 T (h_{t-1} + h_{t+1}) / E + 2 T h_t D / E^2     a missing neighbour adds 0;  E = 0 -> Gp = Gm = 0
    stage 2   H <- h * (W^T . R + beta Gm) / (colsumW + alpha + beta Gp + eps)

THE BARS follow S's rule: u = 2^-24; a sum of m non-negative terms that each carry a relative error of at most a u is within (a + m - 1) u
of the exact sum relative to the sum itself, in any order; a bar is the roundings on the longest path to the element times u times the
element's own float64 reference, a reference of exactly 0 demands exactly 0, and each constant holds 2 spare roundings.  (h_t - h_{t-1})^2
is a non-negative term: the device forms h in float64 from the float32 s and H -- an exact product -- so the difference does not cancel
rounded operands, and the term carries float64 roundings alone.  E, D, Gm, Gp, the numerator and the denominator of stage 2 are sums of
non-negative terms.  The counts are stated at each bar function; nothing here was fitted to a device result."""
import numpy as np

import klnmf_stages_restatement as S
from klnmf_stages_restatement import share, U24, ALPHA, EPS      # noqa: F401  (re-exported for the tests)

CONTINUITY, STEREO = 1 << 28, 1 << 29          # GCCNMF_FLAG_CONTINUITY, GCCNMF_FLAG_CONTINUITY_STEREO of include/gccnmf_hip.h
PLAN_BIT = 128                                 # bit 7 of gccnmf_klnmf_plan


def _f64(*a):
    return [np.asarray(x, np.float64) for x in a]


def flags(segments):
    return CONTINUITY | (STEREO if segments == 2 else 0)


# ---- the term --------------------------------------------------------------------------------------------------------------------------------
def terms(H, s, segments):
    """-> E (K, segments), D (K, segments), Gm (K, N), Gp (K, N) of h = s * H (s = None: H is materialised)."""
    H, = _f64(H)
    K, N = H.shape
    T = N // segments
    assert T * segments == N
    h = (H if s is None else np.asarray(s, np.float64)[:, None] * H).reshape(K, segments, T)
    E = (h * h).sum(2)
    D = (np.diff(h, axis=2) ** 2).sum(2)
    nb = np.zeros(h.shape)                       # h_{t-1} + h_{t+1}, a missing neighbour adds 0
    nb[:, :, 1:] += h[:, :, :-1]
    nb[:, :, :-1] += h[:, :, 1:]
    n = np.full(T, 2.0)
    n[0] -= 1
    n[-1] -= 1                                   # (T = 1: 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        Gp = 2 * T * n * h / E[:, :, None]
        Gm = 2 * T * nb / E[:, :, None] + 2 * T * h * (D / (E * E))[:, :, None]
    dead = np.broadcast_to((E == 0)[:, :, None], h.shape)
    Gp[dead] = 0
    Gm[dead] = 0
    return E, D, Gm.reshape(K, N), Gp.reshape(K, N)


def cost(H, segments):
    """sum over atoms and segments of c = T D / E (an all-zero row contributes 0)."""
    E, D, _, _ = terms(H, None, segments)
    T = np.asarray(H).shape[1] // segments
    return float((T * D[E > 0] / E[E > 0]).sum())


# ---- the stages ------------------------------------------------------------------------------------------------------------------------------
def stage2(W, H, s, R, colsumW, beta, segments, alpha=ALPHA, eps=EPS):
    """At beta = 0 this is S.stage2, bit for bit (x + 0 is x)."""
    _, _, Gm, Gp = terms(H, s, segments)
    W, H, s, R, colsumW, alpha, eps, beta = _f64(W, H, s, R, colsumW, alpha, eps, beta)
    return (s[:, None] * H) * (W.T @ R + beta * Gm) / ((colsumW + alpha)[:, None] + beta * Gp + eps)


def iterate(V, W, H, beta, segments, alpha, eps, iterations):
    """`iterations` whole iterations in float64 from the given factors (the H a caller sees: the scale is materialised every iteration,
    which in exact arithmetic is what the lazy scale computes)."""
    V, W, H = _f64(V, W, H)
    one = np.ones(W.shape[1])
    for _ in range(iterations):
        H = stage2(W, H, one, S.stage1(V, W, H, one), W.sum(0), beta, segments, alpha, eps)
        W, s, _ = S.stage5(W, *S.stage4(S.stage3(V, W, H), H))
        H = H * s[:, None]
    return W, H


def kl(V, W, H):
    """float64 D_KL(V || W.H); a zero of V contributes R."""
    V, W, H = _f64(V, W, H)
    R = W @ H
    pos = V > 0
    logs = np.zeros_like(V)
    logs[pos] = V[pos] * np.log(V[pos] / R[pos])
    return float((logs - V + R).sum())


def objective(V, W, H, alpha, beta, segments):
    return kl(V, W, H) + alpha * float(np.asarray(H, np.float64).sum()) + beta * cost(H, segments)


# ---- the bars (each: a multiple of u, relative to the element's own reference) ---------------------------------------------------------------
def bar_ED():
    """E and D: every term is formed in float64 from exact operands (s * H is exact in float64) and summed in float64 -- T + 3 roundings of
    2^-53, below 1e-5 u for any T < 2^20 --, then rounded ONCE to float32 (1); + 2 spare, which cover the float64 part."""
    return 3 * U24


def bar_G():
    """Gm and Gp: float64 from the float64 E and D and exact h -- a handful of 2^-53 roundings on top of E's and D's -- rounded ONCE to
    float32 (1); + 2 spare."""
    return 3 * U24


def bar_H(F):
    """stage 2.  Numerator W^T . R + beta Gm: the GEMM element carries F (S.bar_H: F products, F - 1 additions), beta Gm carries Gm's
    rounding and the product (2); the sum of the two non-negative terms adds 1: max(F, 2) + 1 = F + 1 (F >= 2).  Denominator
    ((colsumW + alpha) + beta Gp) + eps: beta Gp carries 2, the other terms are exact; three additions: 2 + 3 = 5.  The quotient (1), s * h
    (1), their product (1).  F + 10 - 1 = F + 9; + 2 spare."""
    return (F + 11) * U24


def conditioning(H, segments):
    """max over atoms and segments of sqrt(E / D): how much a relative perturbation of H is amplified in D, a sum of squared DIFFERENCES.
    With |dh_t| <= e h_t:  |dD| <= 2 sum |d_t| e (h_t + h_{t-1}) <= 2 e sqrt(D) sqrt(4 E)  (Cauchy-Schwarz), i.e. 4 e sqrt(E / D) of D."""
    E, D, _, _ = terms(H, None, segments)
    ok = D > 0
    return float(np.sqrt(E[ok] / D[ok]).max()) if ok.any() else 0.0


def trajectory_bars(F, N, K, iterations, kappa):
    """(bar of W, bar of H) after `iterations` whole iterations from exact initial factors: the per-stage counts carried along to first
    order, by the rule of beta_nmf_restatement.trajectory_bars.  e_X is the relative error of X in units of u.  A product or quotient adds
    its operands' errors and its own rounding; a sum of non-negative terms carries the largest error among its terms plus its own count;
    sqrt halves.  D is the one quantity that is not such a sum of its inputs: an error e_H of H moves it by 4 kappa e_H (conditioning;
    kappa = the largest sqrt(E / D) the float64 trajectory meets).  Per iteration (s = 1: H is materialised):
        P: e_W + e_H + K + 1,  R = P + 1
        E = 2 e_H + 1,  D = 4 kappa e_H + 1,  Gp = e_H + E + 1,  Gm = e_H + max(E, D + 2 E) + 1
        H' = e_H + (max(e_W + R + F, Gm + 1) + 1) + (max(e_W + F, Gp + 1) + 3) + 3
        R' from (W, H') likewise;  U = R' + e_H' + N,  rowsumH = e_H' + N,  Wt = e_W + U + rowsumH + 2
        s = e_Wt + F / 2 + 1,  W' = e_Wt + e_s + 1,  H'' = e_H' + e_s + 1
    + 2 spare at the end.  Valid while the result times u stays far below 1 (the callers assert it)."""
    eW = eH = 0.0
    for _ in range(iterations):
        eR = eW + eH + K + 2
        eE, eD = 2 * eH + 1, 4 * kappa * eH + 1
        eGp, eGm = eH + eE + 1, eH + max(eE, eD + 2 * eE) + 1
        eH = eH + (max(eW + eR + F, eGm + 1) + 1) + (max(eW + F, eGp + 1) + 3) + 3
        eR = eW + eH + K + 2
        eWt = eW + (eR + eH + N) + (eH + N) + 2
        es = eWt + F / 2.0 + 1
        eW, eH = eWt + es + 1, eH + es + 1
    return (eW + 2) * U24, (eH + 2) * U24


# ---- the shapes and problems of tests/test_gpu_temporal_continuity.py -----------------------------------------------------------------------
ROW_PASS = 64          # frames one pass of the row launch's wave covers (csrc/nmf_smooth.hip: every row is read twice, whatever its length)
# (F, T, K, segments, batch): the segment boundary inside a column tile (T = 40), exactly on a tile edge (64), neighbours across a tile edge and
# a row of one more than a pass (65), T = 1 and T = 2, one segment with N odd; K in {1, 33, 100, 130}; F in {2, 33, 513}
SHAPES = [(33, 40, 33, 2, 2), (513, 64, 100, 2, 1), (33, 65, 130, 2, 2), (2, 1, 1, 2, 1), (33, 2, 33, 2, 1), (33, 71, 100, 1, 3), (2, 65, 1, 1, 1)]


def problem(F, T, K, segments, files, zero_row=True):
    """S.problem at N = segments * T without the all-zero bin and frame (isolated exact zeros stay), with smooth rows at the even atoms of H
    (a random walk: D << E, the case the term is for) and, with `zero_row` and from two atoms on, atom 1 of file 0 all zero (E = 0: the row
    stays zero, and a whole iteration would divide by its row sum).  float32, read-only."""
    N = segments * T
    V, W, H, s = S.problem(F, N, K, files, lines=False)
    H = H.copy()
    rng = np.random.RandomState(F + 5 * T + 11 * K)
    for k in range(0, K, 2):
        H[:, k, :] = (np.abs(np.cumsum(rng.randn(files, N), axis=1)) * 0.2 + 0.05).astype(np.float32)
    if zero_row and K >= 2:
        H[0, 1, :] = 0
    H.flags.writeable = False
    return V, W, H, s
