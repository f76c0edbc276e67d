"""NumPy restatement of the EM refinement of the spatial (multichannel Wiener) reconstruction (include/gccnmf_hip.h, gccnmf_reconstruct
with GCCNMF_RECONSTRUCT_SPATIAL_ITERATIONS(n) on S; csrc/spatial_em.hip): the local Gaussian model EM of Duong, Vincent & Gribonval
(2010) started from the spatial mode of tests/spatial_restatement.py (SR).  Per file, E[i, c] the ratio-mode estimates (S, 2, F, T),
X (2, F, T), lambda = SR.LOADING:

    start      v_i = SR.powers(E),  R~_i = SR.covariances(E)
    iteration  for every bin, against the OLD R~:  Sigma = sum_j v_j R~_j (ascending j),  G_i = v_i R~_i Sigma^-1,  s_i = G_i X,
               C_i = s_i s_i^H + (I - G_i) v_i R~_i,  v'_i = max(0, 1/2 Re tr(R~_i^-1 C_i)),  v'_i = 0 for every i where sum_j v_j = 0;
               then  A_i = sum over the frames with v'_i != 0 of C_i / v'_i (float32 terms, float64 sum),  n_i = their number,
               R'_i = A_i / n_i (I when n_i = 0),  R~'_i = R'_i + lambda 1/2 tr(R'_i) I, rounded to float32 once;  v <- v', R~ <- R~'
    output     v_i R~_i Sigma^-1 X, SR.spatial_filter's formulas on the final v and R~

The form that is evaluated (``em_step``; both precisions, so that their distance is what float32 costs and nothing else).  With
w_j = v_j 2^-e (e the binary exponent of sum_j v_j, SR's scaling; e = 0 in the unscaled float64 evaluation), Sigma_w = sum_j w_j R~_j,
y = Sigma_w^-1 X, u_i = R~_i y (so s_i = w_i u_i) and N_i = sum_{j != i} w_j R~_j (ascending j):

    2 - tr G_i          = tr(Sigma_w^-1 N_i) =: k_i          a sum of non-negative parts where the literal 2 - tr G_i cancels
    (I - G_i) v_i R~_i  = v_i N_i Sigma_w^-1 R~_i =: v_i P_i   (Hermitian: R~_i - w_i R~_i Sigma_w^-1 R~_i; small when N_i is, no cancellation)
    s_i^H R~_i^-1 s_i   = w_i^2 y^H R~_i y = w_i^2 Re(y^H u_i)   (no inverse of R~_i)
    v'_i = w_i v"_i,  v"_i = 1/2 (w_i Re(y^H u_i) + 2^e k_i);     C_i = w_i C"_i,  C"_i = w_i u_i u_i^H + 2^e P_i;    C_i / v'_i = C"_i / v"_i

-- v"_i and C"_i have the magnitude of |X|^2 whatever the target's share is, so the quotient keeps float32 accuracy for a target
whose own power is subnormal.  ``literal_step`` evaluates the definition as written (inverse of R~_i, 2 x 2 matrix products) in
float64; tests/test_spatial_em_host.py holds the two together.  A frame whose v'_i is NaN is counted (its term is NaN too): NaN
propagates into the bin's covariance, and stays in that bin.  A power that is exactly 0 stays 0 (w_i = 0).

``spatial_em(E, X, n)`` is the contract (float64); ``spatial_em(E, X, n, np.float32)`` rounds the inputs to float32 once and uses float64
only for the frame sums and R~, and adds the frames pairwise (np.sum) where the float64 evaluation adds them in ascending order.
``measured_bar`` is SR.BAR_FACTOR times the distance of the two, relative to max|X|.  Nothing here knows about the device."""
import numpy as np

import spatial_restatement as SR

LOADING = SR.LOADING
BAR_FACTOR = SR.BAR_FACTOR          # association order of the 2 x 2 products and the reciprocals, as in SR


def _planes(X, dtype):
    X = np.asarray(X).astype(np.complex64)
    return tuple(a.astype(dtype) for a in (X[0].real, X[0].imag, X[1].real, X[1].imag))


def _solve(v, R, x, dtype, scaled):
    """v (S, F, T), R (S, F, 4) in dtype, x the four planes of X -> (w, e, vs, (a, d, br, bi), rdet, y): SR.spatial_filter's roundings."""
    S = v.shape[0]
    r = lambda j, k: R[j, :, k][:, None]
    e = np.zeros(v.shape[1:], np.int64)
    if scaled:
        total = v[0].copy()
        for j in range(1, S):
            total = total + v[j]
        e = np.where(np.isfinite(total), np.frexp(np.where(np.isfinite(total), total, 0))[1], 0)
        v = np.ldexp(v, -e[None]).astype(dtype)
    vs = v[0].copy()
    a, d, br, bi = v[0] * r(0, 0), v[0] * r(0, 1), v[0] * r(0, 2), v[0] * r(0, 3)
    for j in range(1, S):
        vs = vs + v[j]
        a, d, br, bi = a + v[j] * r(j, 0), d + v[j] * r(j, 1), br + v[j] * r(j, 2), bi + v[j] * r(j, 3)
    det = a * d - (br * br + bi * bi)
    rdet = dtype(1.0) / det
    x0r, x0i, x1r, x1i = x
    y = ((d * x0r - (br * x1r - bi * x1i)) * rdet, (d * x0i - (br * x1i + bi * x1r)) * rdet,
         (a * x1r - (br * x0r + bi * x0i)) * rdet, (a * x1i - (br * x0i - bi * x0r)) * rdet)
    return v, e, vs, (a, d, br, bi), rdet, y


def _u(R, i, y):
    """u_i = R~_i y, the association of SR.spatial_filter's output."""
    r = lambda k: R[i, :, k][:, None]
    y0r, y0i, y1r, y1i = y
    return (r(0) * y0r + (r(2) * y1r - r(3) * y1i), r(0) * y0i + (r(2) * y1i + r(3) * y1r),
            (r(2) * y0r + r(3) * y0i) + r(1) * y1r, (r(2) * y0i - r(3) * y0r) + r(1) * y1i)


def filter_with(v, R, X, dtype=np.float64, scaled=None):
    """The output stage on given powers v (S, F, T) and covariances R (S, F, 4): SR.spatial_filter(E, X, dtype, R=R) when v = SR.powers(E)."""
    v = np.asarray(v, dtype)
    S = v.shape[0]
    R = np.asarray(R, np.float32).astype(dtype)
    if scaled is None:
        scaled = dtype == np.float32
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        w, _, vs, _, _, y = _solve(v, R, _planes(X, dtype), dtype, scaled)
        out = np.zeros((S, 2) + v.shape[1:], np.complex128 if dtype == np.float64 else np.complex64)
        for i in range(S):
            u0r, u0i, u1r, u1i = _u(R, i, y)
            out[i, 0].real, out[i, 0].imag, out[i, 1].real, out[i, 1].imag = w[i] * u0r, w[i] * u0i, w[i] * u1r, w[i] * u1i
    out[:, :, vs == 0] = 0
    return out


def em_step(v, R, X, dtype=np.float64, scaled=None, order='v_first', weighting='normalised', frame_sum=None, close=None):
    """One iteration.  v (S, F, T) in dtype, R (S, F, 4) float32 -> (v' in dtype, R~' float32).  ``order`` / ``weighting``: the two
    variants scripts/spatial_em_study.py keeps on record ('r_first': A_i = sum C_i / v_i with the OLD power, then v'_i against the NEW
    R~'_i, the same C_i; 'power': A_i = sum C_i / 1/2 sum tr C_i);
    the contract is the default of both.  ``frame_sum`` (float64 (F, T) -> (F,)) replaces the order in which the frames' terms are
    added; ``close(sums, use)`` (the four sums (F,) and the frames counted (F, T) -> R~' (F, 4) float64 before its rounding) replaces
    step 2's quotient and loading (tests/spatial_checks.py: the device's order, and planted mistakes)."""
    v = np.asarray(v, dtype)
    S, F, T = v.shape
    R32 = np.asarray(R, np.float32)
    R = R32.astype(dtype)
    if scaled is None:
        scaled = dtype == np.float32
    r = lambda j, k: R[j, :, k][:, None]
    half, two = dtype(0.5), dtype(2.0)
    vn = np.zeros_like(v)
    Rn = np.zeros((S, F, 4), np.float64)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        w, e, vs, (a, d, br, bi), rdet, y = _solve(v, R, _planes(X, dtype), dtype, scaled)
        y0r, y0i, y1r, y1i = y
        for i in range(S):
            u0r, u0i, u1r, u1i = _u(R, i, y)
            n0 = n1 = nr = ni = np.zeros((F, T), dtype)
            first = True
            for j in range(S):
                if j == i:
                    continue
                t = (w[j] * r(j, 0), w[j] * r(j, 1), w[j] * r(j, 2), w[j] * r(j, 3))
                n0, n1, nr, ni = t if first else (n0 + t[0], n1 + t[1], nr + t[2], ni + t[3])
                first = False
            k = ((d * n0 + a * n1) - two * (br * nr + bi * ni)) * rdet
            h = (y0r * u0r + y0i * u0i) + (y1r * u1r + y1i * u1i)
            v2 = half * (w[i] * h + np.ldexp(k, e).astype(dtype))
            vi = w[i] * v2
            vi = np.where(vi < 0, dtype(0), vi)
            vi[vs == 0] = 0
            vn[i] = vi
            # M = det Sigma_w^-1 R~_i,  P = N_i M / det
            x_, y_, z_, q_ = r(i, 0), r(i, 1), r(i, 2), r(i, 3)
            kk, ll = br * z_ + bi * q_, bi * z_ - br * q_
            m00r = d * x_ - kk
            m11r, m11i = a * y_ - kk, ll
            m01r, m01i = d * z_ - br * y_, d * q_ - bi * y_
            m10r, m10i = a * z_ - br * x_, bi * x_ - a * q_
            p00 = (n0 * m00r + (nr * m10r - ni * m10i)) * rdet
            p11 = ((nr * m01r + ni * m01i) + n1 * m11r) * rdet
            p01r = (n0 * m01r + (nr * m11r - ni * m11i)) * rdet
            p01i = (n0 * m01i + (nr * m11i + ni * m11r)) * rdet
            c = (w[i] * (u0r * u0r + u0i * u0i) + np.ldexp(p00, e).astype(dtype),
                 w[i] * (u1r * u1r + u1i * u1i) + np.ldexp(p11, e).astype(dtype),
                 w[i] * (u0r * u1r + u0i * u1i) + np.ldexp(p01r, e).astype(dtype),
                 w[i] * (u0i * u1r - u0r * u1i) + np.ldexp(p01i, e).astype(dtype))
            use = ~(vi == 0)                                   # NaN counts
            cnt = use.sum(axis=-1).astype(np.float64)
            if weighting == 'power':
                terms = [np.where(use, w[i] * ck, 0).astype(np.float64) for ck in c]       # C_i = w_i C"_i itself
            elif order == 'r_first':
                terms = [np.where(use, np.ldexp(ck, -e), 0).astype(np.float64) for ck in c]   # C_i / v_i, the OLD power (v_i = w_i 2^e)
            else:
                rv = dtype(1.0) / v2
                terms = [np.where(use, ck * rv, 0).astype(np.float64) for ck in c]
            if frame_sum is not None:
                sums = [frame_sum(tk) for tk in terms]
            elif dtype == np.float64:
                sums = [np.cumsum(tk, axis=-1)[..., -1] for tk in terms]                   # ascending frames
            else:
                sums = [np.sum(tk, axis=-1) for tk in terms]                               # pairwise: another order
            if weighting == 'power':
                cnt = half * (sums[0] + sums[1])
            none = cnt == 0
            den = np.where(none, 1.0, cnt)
            r00, r11 = np.where(none, 1.0, sums[0] / den), np.where(none, 1.0, sums[1] / den)
            rr, ri = np.where(none, 0.0, sums[2] / den), np.where(none, 0.0, sums[3] / den)
            load = LOADING * (0.5 * (r00 + r11))
            Rn[i] = np.stack([r00 + load, r11 + load, rr, ri], axis=-1) if close is None else close(sums, use)
            if order == 'r_first':                             # ... and v'_i = 1/2 Re tr(R~'_i^-1 C_i) against the NEW covariance
                q00, q11, qr, qi = (Rn[i, :, k].astype(np.float32).astype(dtype)[:, None] for k in range(4))
                tr = (q11 * c[0] + q00 * c[1] - two * (qr * c[2] + qi * c[3])) / (q00 * q11 - (qr * qr + qi * qi))
                vi = w[i] * (half * tr)
                vi = np.where(vi < 0, dtype(0), vi)
                vi[vs == 0] = 0
                vn[i] = np.where(use, vi, 0)
    return vn, Rn.astype(np.float32)


def literal_step(v, R, X):
    """One iteration as the definition is written, float64 with complex 2 x 2 matrices: (v', R'_i before the loading and the rounding,
    as (S, F, 2, 2) complex)."""
    v = np.asarray(v, np.float64)
    S, F, T = v.shape
    R = np.asarray(R, np.float32).astype(np.float64)
    Rm = np.empty((S, F, 2, 2), np.complex128)
    Rm[..., 0, 0], Rm[..., 1, 1] = R[..., 0], R[..., 1]
    Rm[..., 0, 1] = R[..., 2] + 1j * R[..., 3]
    Rm[..., 1, 0] = R[..., 2] - 1j * R[..., 3]
    Xv = np.moveaxis(np.asarray(X).astype(np.complex64).astype(np.complex128), 0, -1)[..., None]          # (F, T, 2, 1)
    Sigma = (v[..., None, None] * Rm[:, :, None]).sum(axis=0)                                              # (F, T, 2, 2)
    live = v.sum(axis=0) != 0
    Si = np.linalg.inv(np.where(live[..., None, None], Sigma, np.eye(2)))
    vn, Rn = np.zeros_like(v), np.zeros((S, F, 2, 2), np.complex128)
    for i in range(S):
        vR = v[i][..., None, None] * Rm[i][:, None]
        G = vR @ Si
        s = G @ Xv
        C = s @ np.conj(np.swapaxes(s, -1, -2)) + (np.eye(2) - G) @ vR
        vi = np.maximum(0.0, 0.5 * np.trace(np.linalg.inv(Rm[i])[:, None] @ C, axis1=-2, axis2=-1).real)
        vi[~live] = 0
        vn[i] = vi
        use = vi != 0
        A = np.where(use[..., None, None], C / np.where(use, vi, 1.0)[..., None, None], 0).sum(axis=1)
        cnt = use.sum(axis=1)
        Rn[i] = np.where((cnt == 0)[:, None, None], np.eye(2), A / np.maximum(cnt, 1)[:, None, None])
    return vn, Rn


def refine(E, X, n, dtype=np.float64, loading=LOADING, **variant):
    """-> (v, R~) after n iterations: (S, F, T) in dtype, (S, F, 4) float32."""
    assert loading == LOADING or not n
    v, R = SR.powers(E, dtype), SR.covariances(E, loading)
    for _ in range(int(n)):
        v, R = em_step(v, R, X, dtype, **variant)
    return v, R


def spatial_em(E, X, n, dtype=np.float64, **variant):
    """E (S, 2, F, T), X (2, F, T) -> E' (S, 2, F, T) after n iterations; n = 0 is SR.spatial_filter(E, X, dtype)."""
    if not int(n):
        return SR.spatial_filter(E, X, dtype)
    v, R = refine(E, X, n, dtype, **variant)
    return filter_with(v, R, X, dtype)


def measured_bar(E, X, n):
    """(bar, float32 error, E' float64): as SR.measured_bar.  The condition the bar rests on is asserted: the zero pattern of the powers
    and the NaN pattern are the same in the two evaluations (a frame that one of them skips and the other counts is not a rounding)."""
    X = np.asarray(X)
    v64, R64 = refine(E, X, n, np.float64)
    v32, R32 = refine(E, X, n, np.float32)
    assert np.array_equal(v64 == 0, v32 == 0), 'the zero pattern of the powers differs between float32 and float64'
    assert np.array_equal(np.isnan(v64), np.isnan(v32)) and np.array_equal(np.isnan(R64), np.isnan(R32))
    ref = filter_with(v64, R64, X, np.float64) if int(n) else SR.spatial_filter(E, X, np.float64)
    f32 = filter_with(v32, R32, X, np.float32) if int(n) else SR.spatial_filter(E, X, np.float32)
    assert np.array_equal(np.isfinite(ref), np.isfinite(f32))
    ok = np.isfinite(ref)
    scale = float(np.abs(X[np.isfinite(X)]).max())
    err = float(np.abs(f32[ok] - ref[ok]).max()) / scale if ok.any() else 0.0
    return BAR_FACTOR * err, err, ref
