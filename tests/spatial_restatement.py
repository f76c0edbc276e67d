"""NumPy restatement of the spatial (multichannel Wiener) reconstruction (include/gccnmf_hip.h, gccnmf_reconstruct with
GCCNMF_RECONSTRUCT_RATIO and GCCNMF_RECONSTRUCT_SPATIAL_BATCH; csrc/spatial.hip).  Per file, with E[i, c] the ratio-mode estimate of
target i, channel c (S, 2, F, T) and X (2, F, T):

    v_i[f,t]  = 1/2 (|E_i,0|^2 + |E_i,1|^2)
    p_c       = sum_t |E_i,c|^2,  q = sum_t E_i,0 conj(E_i,1),  n = (p_0 + p_1) / 2      frames in ascending order, float64
    R_i[f]    = [[p_0, q], [conj q, p_1]] / n;  R_i[f] = I when n = 0
    R~_i[f]   = R_i[f] + LOADING I, rounded to float32 once
    Sigma     = sum_j v_j R~_j (ascending j);  y = Sigma^-1 X (closed 2 x 2 Hermitian inverse);  E'_i = v_i R~_i y
    E'_i = 0 for every i where sum_j v_j = 0;  NaN / Inf propagate

``spatial_filter(E, X)`` evaluates this in float64 (the contract); ``spatial_filter(E, X, np.float32)`` evaluates the same formulas in
float32 with the inputs rounded to float32 once and float64 only where the definition says so (the covariance sums and R~): its distance
from the float64 evaluation is what float32 arithmetic costs on those inputs, and ``measured_bar`` is BAR_FACTOR times that.  The
float32 evaluation works on w_j = v_j 2^-e, e the binary exponent of sum_j v_j, as include/gccnmf_hip.h allows: an exact scaling that
leaves every rounding as it is while all intermediates are normal float32 numbers (``scaled=False`` evaluates the v_j themselves: the
same bits there) and keeps the determinant of a nearly silent frame out of the subnormal range, where the literal form loses the frame.
Nothing here knows about the device."""
import numpy as np

LOADING = 1e-3              # GCCNMF_SPATIAL_LOADING (include/gccnmf_hip.h)
BAR_FACTOR = 4.0            # covers the other association order of the 2 x 2 products and the reciprocal


def covariances(E, loading=LOADING, frame_sum=None):
    """E (S, 2, F, T) complex -> R~ as (S, F, 4) float32: (R~00, R~11, Re R~01, Im R~01).  The sums run over the frames in ascending
    order in float64 (np.cumsum adds sequentially); ``frame_sum`` (float64 (..., T) -> (...)) adds them in another order
    (tests/spatial_checks.py: the device's)."""
    E = np.asarray(E).astype(np.complex64).astype(np.complex128)
    S, _, F, T = E.shape
    with np.errstate(invalid='ignore', over='ignore'):
        last = frame_sum or (lambda a: np.cumsum(a, axis=-1)[..., -1])
        p0 = last(E[:, 0].real ** 2 + E[:, 0].imag ** 2)
        p1 = last(E[:, 1].real ** 2 + E[:, 1].imag ** 2)
        qr = last(E[:, 0].real * E[:, 1].real + E[:, 0].imag * E[:, 1].imag)
        qi = last(E[:, 0].imag * E[:, 1].real - E[:, 0].real * E[:, 1].imag)
    n = 0.5 * (p0 + p1)
    zero = n == 0
    with np.errstate(divide='ignore', invalid='ignore'):
        d = np.where(zero, 1.0, n)
        r00 = np.where(zero, 1.0, p0 / d)
        r11 = np.where(zero, 1.0, p1 / d)
        rr = np.where(zero, 0.0, qr / d)
        ri = np.where(zero, 0.0, qi / d)
    return np.stack([r00 + loading, r11 + loading, rr, ri], axis=-1).astype(np.float32)


def powers(E, dtype=np.float64):
    """v (S, F, T) in ``dtype`` from inputs rounded to float32 once."""
    E = np.asarray(E).astype(np.complex64)
    r0, i0, r1, i1 = (a.astype(dtype) for a in (E[:, 0].real, E[:, 0].imag, E[:, 1].real, E[:, 1].imag))
    with np.errstate(invalid='ignore', over='ignore'):
        return dtype(0.5) * ((r0 * r0 + i0 * i0) + (r1 * r1 + i1 * i1))


def spatial_filter(E, X, dtype=np.float64, R=None, loading=LOADING, scaled=None):
    """E (S, 2, F, T), X (2, F, T) -> E' (S, 2, F, T) complex128 (float64) or complex64 (float32).  R: covariances to use instead of
    those of E (tests of the rules for R).  scaled: evaluate on the v_j scaled by a power of two (default: in float32 only)."""
    E = np.asarray(E)
    S = E.shape[0]
    R = (covariances(E, loading) if R is None else np.asarray(R, np.float32)).astype(dtype)
    v = powers(E, dtype)
    X = np.asarray(X).astype(np.complex64)
    x0r, x0i, x1r, x1i = (a.astype(dtype) for a in (X[0].real, X[0].imag, X[1].real, X[1].imag))
    r = lambda j, k: R[j, :, k][:, None]
    if scaled is None:
        scaled = dtype == np.float32
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
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
        y0r = (d * x0r - (br * x1r - bi * x1i)) * rdet
        y0i = (d * x0i - (br * x1i + bi * x1r)) * rdet
        y1r = (a * x1r - (br * x0r + bi * x0i)) * rdet
        y1i = (a * x1i - (br * x0i - bi * x0r)) * rdet
        out = np.zeros(E.shape, np.complex128 if dtype == np.float64 else np.complex64)
        for i in range(S):
            out[i, 0].real = v[i] * (r(i, 0) * y0r + (r(i, 2) * y1r - r(i, 3) * y1i))
            out[i, 0].imag = v[i] * (r(i, 0) * y0i + (r(i, 2) * y1i + r(i, 3) * y1r))
            out[i, 1].real = v[i] * ((r(i, 2) * y0r + r(i, 3) * y0i) + r(i, 1) * y1r)
            out[i, 1].imag = v[i] * ((r(i, 2) * y0i - r(i, 3) * y0r) + r(i, 1) * y1i)
    out[:, :, vs == 0] = 0                                # False where the sum is NaN: those propagate
    return out


def measured_bar(E, X):
    """(bar, float32 error, E' float64): distances relative to max|X|; the bar is BAR_FACTOR x the largest distance of the float32
    evaluation from the float64 one over the elements where both are finite (a NaN must be a NaN in both)."""
    X = np.asarray(X)
    ref = spatial_filter(E, X, np.float64)
    f32 = spatial_filter(E, X, np.float32)
    assert np.array_equal(np.isfinite(ref), np.isfinite(f32))
    ok = np.isfinite(ref)
    scale = float(np.abs(X[np.isfinite(X)]).max())
    err = float(np.abs(f32[ok] - ref[ok]).max()) / scale if ok.any() else 0.0
    return BAR_FACTOR * err, err, ref


def best_assignment_sdr(estimates, images, windowSize):
    """estimates (S, 2, L), images (S, 2, n): the stereo image SDR (both channels' energies pooled) of every source under the permutation
    of the outputs that maximises the mean -> (sdr per source, permutation)."""
    import itertools
    S = len(images)
    off = windowSize // 2

    def sdr(e, s, guard=4000):
        est = np.asarray(e, np.float64)
        a, b = off + guard, off + est.shape[-1] - guard
        ref = np.asarray(s, np.float64)[:, a:b]
        return 10.0 * np.log10(np.sum(ref ** 2) / np.sum((ref - est[:, a - off:b - off]) ** 2))

    table = np.array([[sdr(estimates[j], images[i]) for j in range(len(estimates))] for i in range(S)])
    best = max(itertools.permutations(range(len(estimates)), S), key=lambda p: sum(table[i, p[i]] for i in range(S)))
    return np.array([table[i, best[i]] for i in range(S)]), best
