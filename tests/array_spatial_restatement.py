"""NumPy restatement of the M x M spatial (multichannel Wiener) filter of the microphone-array path (include/gccnmf_array_spatial.h,
csrc/array_spatial.hip).  Per file, with E[i, c] the ratio-mode estimate of target i, channel c (S, M, F, T) and X (M, F, T):

    v_i[f,t]  = (sum_c |E_i,c|^2) / M
    R_i[f]    = sum_t E_i E_i^H / n,  n = (sum_c p_c) / M,  p_c = sum_t |E_i,c|^2  (float64; tr R_i = M);  R_i = I when n = 0
    R~_i[f]   = R_i[f] + LOADING I, rounded to float32 once
    Sigma_w   = sum_j w_j R~_j,  w_j = v_j 2^-e (e the binary exponent of sum_j v_j);  y = Sigma_w^-1 X;  E'_i = w_i R~_i y
    E'_i = 0 for every i where sum_j v_j = 0;  NaN / Inf propagate

A covariance is kept as the device keeps it: a row of M M float32 -- the M diagonal entries, then (Re, Im) of the entries (a, b), a < b, in
lexicographic order (``pairs``); ``hermitian`` expands a row to the full matrix.

``spatial_filter(E, X)`` evaluates this in float64 with numpy.linalg.solve (the contract); ``spatial_filter(E, X, np.float32)`` runs the
header's order operation by operation -- the square-root-free LDL^H factorisation without pivoting, the two substitutions and the
output products, every product and sum its own float32 rounding -- and is meant to equal the device bit for bit.  At M = 2 the device
runs the stereo filter's closed 2 x 2 inverse, and so does this file: both precisions are tests/spatial_restatement.py's there
(spatial_filter hands M = 2 over to it, so its equality with the stereo restatement holds by construction; covariances and powers
are this file's own code at every M).  The
keywords ``trace``, ``divisor`` and ``without`` plant mistakes (tests/test_array_spatial_host.py).  Nothing here knows about the device."""
import numpy as np

import spatial_restatement as SR

LOADING = 1e-3              # GCCNMF_ARRAY_SPATIAL_LOADING (include/gccnmf_array_spatial.h)


def pairs(M):
    return [(a, b) for a in range(M) for b in range(a + 1, M)]


def pair_index(M, a, b):
    return a * M - a * (a + 1) // 2 + (b - a - 1)


def covariances(E, loading=LOADING, frame_sum=None, trace=None):
    """E (S, M, F, T) complex -> R~ as (S, F, M M) float32 rows.  The sums run over the frames in ascending order in float64
    (np.cumsum adds sequentially); ``frame_sum`` (float64 (..., T) -> (...)) adds them in another order (tests/spatial_checks.py:
    the device's).  trace: the trace R is normalised to (default M)."""
    E = np.asarray(E).astype(np.complex64).astype(np.complex128)
    S, M, F, T = E.shape
    re, im = E.real, E.imag
    with np.errstate(invalid='ignore', over='ignore'):
        last = frame_sum or (lambda a: np.cumsum(a, axis=-1)[..., -1])
        p = [last(re[:, c] * re[:, c] + im[:, c] * im[:, c]) for c in range(M)]
        qr = [last(re[:, a] * re[:, b] + im[:, a] * im[:, b]) for a, b in pairs(M)]
        qi = [last(im[:, a] * re[:, b] - re[:, a] * im[:, b]) for a, b in pairs(M)]
        tr = p[0]
        for c in range(1, M):
            tr = tr + p[c]
        n = tr / float(M if trace is None else trace)
    zero = n == 0
    with np.errstate(divide='ignore', invalid='ignore'):
        d = np.where(zero, 1.0, n)
        cols = [np.where(zero, 1.0, p[c] / d) + loading for c in range(M)]
        for k in range(len(qr)):
            cols += [np.where(zero, 0.0, qr[k] / d), np.where(zero, 0.0, qi[k] / d)]
    return np.stack(cols, axis=-1).astype(np.float32)


def hermitian(R, M):
    """(..., M M) rows -> (..., M, M) complex: the full Hermitian matrices (complex64 for float32 rows)."""
    R = np.asarray(R)
    out = np.zeros(R.shape[:-1] + (M, M), np.complex64 if R.dtype == np.float32 else np.complex128)
    for a in range(M):
        out[..., a, a] = R[..., a]
    for k, (a, b) in enumerate(pairs(M)):
        out[..., a, b] = R[..., M + 2 * k] + 1j * R[..., M + 2 * k + 1]
        out[..., b, a] = R[..., M + 2 * k] - 1j * R[..., M + 2 * k + 1]
    return out


def powers(E, dtype=np.float64, divisor=None):
    """v (S, F, T) in ``dtype`` from inputs rounded to float32 once: channels ascending, then the quotient by M."""
    E = np.asarray(E).astype(np.complex64)
    M = E.shape[1]
    with np.errstate(invalid='ignore', over='ignore'):
        s = None
        for c in range(M):
            r, i = E[:, c].real.astype(dtype), E[:, c].imag.astype(dtype)
            term = r * r + i * i
            s = term if s is None else s + term
        return s / dtype(M if divisor is None else divisor)


def _scaled(v):
    """w_j = v_j 2^-e, e the binary exponent of sum_j v_j (ascending j) -> (w, the sum)."""
    total = v[0].copy()
    for j in range(1, v.shape[0]):
        total = total + v[j]
    fin = np.isfinite(total)
    e = np.where(fin, np.frexp(np.where(fin, total, 0))[1], 0)
    return np.ldexp(v, -e[None]).astype(v.dtype), total


def ldl_solve(sg, xr, xi, M, recip=None):
    """The header's solve on whatever its operands are: arrays of one dtype, or any objects with *, + and - and unary minus
    (tests/array_spatial_checks.py carries (value, bound) pairs through these very lines); recip(d_k) is the column's reciprocal.
    sg: the M M stored components of Sigma_w (arrays (F, T)); xr, xi: lists of M arrays -> (yr, yi, d): y = Sigma_w^-1 X and the M pivots."""
    recip = recip or (lambda x: x.dtype.type(1.0) / x)
    lr = [[None] * M for _ in range(M)]
    li = [[None] * M for _ in range(M)]
    d, rd = [None] * M, [None] * M
    for k in range(M):
        gr = [lr[k][m] * d[m] for m in range(k)]
        gi = [li[k][m] * d[m] for m in range(k)]
        dk = sg[k]
        for m in range(k):
            dk = dk - (lr[k][m] * gr[m] + li[k][m] * gi[m])
        d[k] = dk
        rd[k] = recip(dk)
        for i in range(k + 1, M):
            q = M + 2 * pair_index(M, k, i)
            cr, ci = sg[q], -sg[q + 1]
            for m in range(k):
                cr = cr - (lr[i][m] * gr[m] + li[i][m] * gi[m])
                ci = ci - (li[i][m] * gr[m] - lr[i][m] * gi[m])
            lr[i][k] = cr * rd[k]
            li[i][k] = ci * rd[k]
    zr, zi = [None] * M, [None] * M
    for i in range(M):
        ar, ai = xr[i], xi[i]
        for k in range(i):
            ar = ar - (lr[i][k] * zr[k] - li[i][k] * zi[k])
            ai = ai - (lr[i][k] * zi[k] + li[i][k] * zr[k])
        zr[i], zi[i] = ar, ai
    for k in range(M):
        zr[k], zi[k] = zr[k] * rd[k], zi[k] * rd[k]
    yr, yi = [None] * M, [None] * M
    for k in range(M - 1, -1, -1):
        ar, ai = zr[k], zi[k]
        for i in range(k + 1, M):
            ar = ar - (lr[i][k] * yr[i] + li[i][k] * yi[i])
            ai = ai - (lr[i][k] * yi[i] - li[i][k] * yr[i])
        yr[k], yi[k] = ar, ai
    return yr, yi, d


def apply_row(r, a, yr, yi, M):
    """u_a = sum_b R~_ab y_b, b ascending, in the header's association.  r: the M M stored components of R~ (arrays (F, 1))."""
    ur = ui = None
    for b in range(M):
        if b == a:
            tr, ti = r[a] * yr[b], r[a] * yi[b]
        elif a < b:
            q = M + 2 * pair_index(M, a, b)
            tr, ti = r[q] * yr[b] - r[q + 1] * yi[b], r[q] * yi[b] + r[q + 1] * yr[b]
        else:
            q = M + 2 * pair_index(M, b, a)
            tr, ti = r[q] * yr[b] + r[q + 1] * yi[b], r[q] * yi[b] - r[q + 1] * yr[b]
        ur, ui = (tr, ti) if b == 0 else (ur + tr, ui + ti)
    return ur, ui


def spatial_filter(E, X, dtype=np.float64, R=None, loading=LOADING, divisor=None, without=None):
    """E (S, M, F, T), X (M, F, T) -> E' (S, M, F, T) complex128 (float64) or complex64 (float32).  R: covariance rows (S, F, M M) to
    use instead of those of E.  Planted mistakes: divisor (the powers' quotient), without (a target left out of Sigma_w)."""
    E = np.asarray(E)
    S, M = E.shape[:2]
    R = covariances(E, loading) if R is None else np.asarray(R, np.float32)
    X = np.asarray(X).astype(np.complex64)
    if M == 2 and divisor is None and without is None:
        return SR.spatial_filter(E, X, dtype, R=R)
    MM = M * M
    v = powers(E, dtype, divisor)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        w, vs = _scaled(v)
        out = np.zeros(E.shape, np.complex128 if dtype == np.float64 else np.complex64)
        used = [j for j in range(S) if j != without]
        if dtype == np.float64:
            H = hermitian(R.astype(np.float64), M)                                      # (S, F, M, M)
            sigma = sum(w[j][:, :, None, None] * H[j][:, None] for j in used)         # (F, T, M, M)
            bad = ~np.isfinite(sigma).all(axis=(-1, -2)) | ~np.isfinite(X).all(axis=0) | (vs == 0)
            sigma = np.where(bad[:, :, None, None], np.eye(M), sigma)
            rhs = np.where(bad[None], 0, X.astype(np.complex128))
            y = np.linalg.solve(sigma, np.transpose(rhs, (1, 2, 0))[..., None])        # (F, T, M, 1)
            for i in range(S):
                u = np.matmul(H[i][:, None], y)[..., 0]                                  # (F, T, M)
                out[i] = np.transpose(w[i][:, :, None] * u, (2, 0, 1))
            out[:, :, bad & ~(vs == 0)] = np.nan * (1 + 1j)
        else:
            r = [[R[j, :, g][:, None] for g in range(MM)] for j in range(S)]
            sg = []
            for g in range(MM):
                a = w[used[0]] * r[used[0]][g]
                for j in used[1:]:
                    a = a + w[j] * r[j][g]
                sg.append(a)
            xr, xi = [X[c].real.astype(dtype) for c in range(M)], [X[c].imag.astype(dtype) for c in range(M)]
            yr, yi, _ = ldl_solve(sg, xr, xi, M)
            for i in range(S):
                for a in range(M):
                    ur, ui = apply_row(r[i], a, yr, yi, M)
                    out[i, a].real, out[i, a].imag = w[i] * ur, w[i] * ui
    out[:, :, vs == 0] = 0                                # False where the sum is NaN: those propagate
    return out
