"""float64 NumPy restatement of the BSS Eval 3.0 image criteria (`bss_eval_images`: Vincent, Sawada, Bofill, Makino & Rosca 2007), written
from the published definition with explicit delayed-signal matrices -- the oracle of gcc_nmf_amd/evaluation.py (mir_eval and museval are
not available; tests/test_bss_eval_host.py pins this file by identities that hold for any correct implementation).

Layout: true images s (J, C, n), estimates e (J, C, n); everything is zero outside [0, n); L filter taps; sums over n + L - 1 samples.
Also here: the test inputs, and the two derived error bars of the device kernels, which hold for ANY summation order and are therefore
fixed, not measured:
    lag correlations   |R_dev - R_exact| <= m 2^-53 sum_n |a_n b_{n+l}|     m = non-zero terms of that lag; the products are exact in float64
    projections        |P_dev - P_ref|   <= (t + 2) 2^-53 sum |coef| |s|    t = terms of that output sample
"""
import itertools
import math

import numpy as np
import scipy.linalg

U = 2.0 ** -53


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def make_case(J, C, n, L, seed=0, artefact_db=-40.0, taps=4):
    """(s, e) float32 (J, C, n): white sources through short random FIRs, one per channel, plus an independent white component of 0.3 in
    every channel image (without it the channel images of a source are exactly linearly dependent across L lags and G is singular);
    estimates = a random, well-conditioned mix of the images (interference) filtered by a 2-tap FIR (spatial distortion) plus white
    artefacts at ``artefact_db`` relative to the image."""
    rng = np.random.default_rng(1000 * seed + 7 * J + 3 * C + n + L)
    s = np.zeros((J, C, n))
    for i in range(J):
        src = rng.standard_normal(n + taps)
        for c in range(C):
            h = rng.standard_normal(taps) * np.array([1.0, 0.5, 0.25, 0.125][:taps])
            s[i, c] = np.convolve(src, h)[taps:taps + n] + 0.3 * rng.standard_normal(n)
    e = np.zeros_like(s)
    for j in range(J):
        for c in range(C):
            mix = s[j, c] + 0.2 * np.roll(s[j, c], 1)
            for i in range(J):
                if i != j:
                    mix = mix + 0.1 * rng.standard_normal() * s[i, c]
            rms = np.sqrt(np.mean(s[j, c] ** 2))
            e[j, c] = mix + 10.0 ** (artefact_db / 20.0) * rms * rng.standard_normal(n)
    return s.astype(np.float32), e.astype(np.float32)


def case_files(shape):
    """The three files of one test shape (J, C, n, L): seeds 0, 1, 2; the third with its estimates in reverse order."""
    files = [make_case(*shape, seed=k) for k in range(3)]
    files[2] = (files[2][0], np.ascontiguousarray(files[2][1][::-1]))
    return files


# (J, C, n, L) of the GPU tests: the five of the issue; n = the correlation kernel's block length + 1; n below L; taps beyond 64 on four
# reference signals; more than 4096 output samples; more than 512 taps and 1024 lags (tests/test_gpu_bss_eval.py says what each reaches)
SHAPES = [(2, 2, 300, 5), (3, 2, 1000, 16), (3, 2, 2000, 33), (1, 2, 257, 8), (2, 1, 500, 16), (2, 2, 1025, 16), (1, 1, 20, 24),
          (2, 2, 1500, 70), (1, 2, 4200, 130), (1, 1, 1300, 520)]
CHUNKED = (3, 1, 1001, 16, 7)            # J, C, n, L and the number of files (seeds 0 .. 6) of the test that cuts a batch into chunks


def all_test_files():
    """(L, s, e) of every file the GPU tests score against this restatement."""
    for shape in SHAPES:
        for s, e in case_files(shape):
            yield shape[3], s, e
    J, C, n, L, B = CHUNKED
    for k in range(B):
        yield (L,) + make_case(J, C, n, L, seed=k)


# The dB tolerance of the device against this restatement: 10 x the largest disagreement between float64 evaluations of the restatement
# that differ only in solver (Cholesky / LU / least squares) and summation order (forward / reversed), measured over all_test_files():
# 6.82e-13 dB (tests/test_bss_eval_host.py measures it again), times 10 and rounded up to two digits.  Both the device's solver and its
# summation order differ.
DB_TOLERANCE = 6.9e-12


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def delayed(s, L):
    """s (J, C, n) -> D (J C L, n + L - 1): row (i, c, tau) is s[i][c][m - tau]."""
    J, C, n = s.shape
    D = np.zeros((J, C, L, n + L - 1))
    for tau in range(L):
        D[:, :, tau, tau:tau + n] = s
    return D.reshape(J * C * L, n + L - 1)


def pad(x, L):
    return np.concatenate([np.asarray(x, np.float64), np.zeros(x.shape[:-1] + (L - 1,))], axis=-1)


def gram(D, order='forward'):
    return D @ D.T if order == 'forward' else D[:, ::-1] @ D[:, ::-1].T


def solve(G, d, solver='lstsq'):
    if solver == 'lstsq':
        return np.linalg.lstsq(G, d, rcond=None)[0]
    if solver == 'cholesky':
        return scipy.linalg.cho_solve(scipy.linalg.cho_factor(G), d)
    if solver == 'lu':
        return np.linalg.solve(G, d)
    raise ValueError(solver)


def sumsq(x, order='forward'):
    x = np.asarray(x).reshape(-1)
    return float(np.sum((x * x)[::-1])) if order == 'reversed' else float(np.sum(x * x))


def decompose(s, e, L, solver='lstsq', order='forward'):
    """(P_all, P_i): P_all (J_est, C, M) and P_i (J_est, J_true, C, M), M = n + L - 1, the projections of every estimate channel on all
    delayed true images / on source i's alone; and cond(G)."""
    s, e = np.asarray(s, np.float64), np.asarray(e, np.float64)
    J, C, n = s.shape
    M, CL = n + L - 1, C * L
    D = delayed(s, L)
    E = pad(e, L).reshape(J * C, M)
    if order == 'reversed':
        G, d = gram(D, order), D[:, ::-1] @ E[:, ::-1].T
    else:
        G, d = gram(D), D @ E.T
    P_all = (solve(G, d, solver).T @ D).reshape(J, C, M)
    P_i = np.zeros((J, J, C, M))
    for i in range(J):
        rows = slice(i * CL, (i + 1) * CL)
        x = solve(G[rows, rows], d[rows], solver)
        P_i[:, i] = (x.T @ D[rows]).reshape(J, C, M)
    return P_all, P_i, float(np.linalg.cond(G))


def ratio_db(num, den):
    if den == 0:
        return np.inf
    with np.errstate(divide='ignore'):
        return 10.0 * np.log10(num / den)


def all_pairs(s, e, L, solver='lstsq', order='forward'):
    """The four tables (J_est, J_true) of SDR, ISR, SIR, SAR in dB, and cond(G)."""
    J = s.shape[0]
    P_all, P_i, cond = decompose(s, e, L, solver, order)
    sp, ep = pad(s, L), pad(e, L)
    out = np.zeros((4, J, J))
    for j in range(J):
        for i in range(J):
            e_spat, e_interf, e_artif = P_i[j, i] - sp[i], P_all[j] - P_i[j, i], ep[j] - P_all[j]
            out[0, j, i] = ratio_db(sumsq(sp[i], order), sumsq(ep[j] - sp[i], order))
            out[1, j, i] = ratio_db(sumsq(sp[i], order), sumsq(e_spat, order))
            out[2, j, i] = ratio_db(sumsq(sp[i] + e_spat, order), sumsq(e_interf, order))
            out[3, j, i] = ratio_db(sumsq(sp[i] + e_spat + e_interf, order), sumsq(e_artif, order))
    return out[0], out[1], out[2], out[3], cond


def best_permutation(sir):
    """perm (J,): estimate perm[i] is true source i, the assignment with the largest mean SIR."""
    J = sir.shape[0]
    best = max(itertools.permutations(range(J)), key=lambda p: np.mean([sir[p[i], i] for i in range(J)]))
    return np.asarray(best)


def bss_eval_images(s, e, L, computePermutation=True, solver='lstsq', order='forward'):
    """(sdr, isr, sir, sar, perm), each (J,) indexed by true source."""
    sdr, isr, sir, sar, _ = all_pairs(s, e, L, solver, order)
    J = s.shape[0]
    perm = best_permutation(sir) if computePermutation else np.arange(J)
    true = np.arange(J)
    return sdr[perm, true], isr[perm, true], sir[perm, true], sar[perm, true], perm


# ---- the bars -------------------------------------------------------------------------------------------------------------------------
def lag_correlations_exact(A, B, L):
    """A (Ma, n), B (Mb, n) float32 -> (R, bar), both (Ma, Mb, 2L - 1): R[a][b][l + L - 1] = sum_n A_a[n] B_b[n + l] summed exactly
    (math.fsum of the products, which are exact in float64), and the kernel's bar m 2^-53 sum |a_n b_{n+l}|."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    n = A.shape[1]
    R = np.zeros((A.shape[0], B.shape[0], 2 * L - 1))
    bar = np.zeros_like(R)
    for a in range(A.shape[0]):
        for b in range(B.shape[0]):
            for l in range(-(L - 1), L):
                lo, hi = max(0, -l), min(n, n - l)
                if hi <= lo:
                    continue
                prod = A[a, lo:hi] * B[b, lo + l:hi + l]
                R[a, b, l + L - 1] = math.fsum(prod)
                bar[a, b, l + L - 1] = np.count_nonzero(prod) * U * math.fsum(np.abs(prod))
    return R, bar


def projections_reference(A, coef, ranges):
    """A (Ma, n) float32, coef (Q, Ma, L) float64, ranges (Q, 2) -> (P, bar), both (Q, n + L - 1): P[q][m] = sum_{a in refs(q)} sum_tau
    coef[q][a][tau] A_a[m - tau], accumulated in extended precision (its own error is below 2^-10 of the bar), and the kernel's bar
    (t + 2) 2^-53 sum |coef| |A|."""
    A = np.asarray(A, np.float64)
    Ma, n = A.shape
    Q, _, L = coef.shape
    M = n + L - 1
    P = np.zeros((Q, M), np.longdouble)
    mag = np.zeros((Q, M), np.longdouble)
    terms = np.zeros((Q, M))
    Al, Cl = A.astype(np.longdouble), np.asarray(coef).astype(np.longdouble)
    for q in range(Q):
        for a in range(ranges[q][0], ranges[q][0] + ranges[q][1]):
            for tau in range(L):
                P[q, tau:tau + n] += Cl[q, a, tau] * Al[a]
                mag[q, tau:tau + n] += np.abs(Cl[q, a, tau]) * np.abs(Al[a])
                terms[q, tau:tau + n] += 1
    return P, (terms + 2) * U * mag.astype(np.float64)
