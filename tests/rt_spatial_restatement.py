"""NumPy restatement of the online spatial (multichannel Wiener) filter of the real-time block call (include/gccnmf_hip.h,
GCCNMF_RT_SEPARATION_SPATIAL; csrc/rt_spatial.hip).  Per stream and bin f, components j < NC, state P_j = (p0, p1, qr, qi) in float32,
frames of a call in ascending order:

    E_j,c     multiple mode: the masked spectrum Y_j,c (NC = N);  single-target modes: E_0 = Y, E_1 = X - E_0 component-wise in float32 (NC = 2)
    c_j       = (|E_j,0|^2, |E_j,1|^2, Re E_j,0 conj E_j,1, Im E_j,0 conj E_j,1),   v_j = 1/2 (c_j.p0 + c_j.p1)
    P_j      <- a P_j + b c_j,  b = 1 / tau,  a = 1 - b, BEFORE use, rounded to float32 (the state is float32); only when X and every c_j
              of the (bin, frame) are finite as float32 numbers, else the bin's state stays bit for bit
    R_j       = P_j / n_j,  n_j = 1/2 (P_j.p0 + P_j.p1);  R_j = I when n_j < 2^-126;  R~_j = R_j + LOADING I
    Y'        = spatial_restatement.spatial_filter(E[..., t], X[..., t], R=R~)      (R~ rounded to float32 once, there)
    written   multiple mode: Y_j <- Y'_j;  single-target: Y <- Y'_0

``rt_spatial(Y, X, P, tau, multi)`` evaluates this in float64 (the contract: everything but the two stated float32 roundings -- the
residual and the stored state -- is float64); with ``np.float32`` it evaluates the same formulas in float32, one rounding per operation,
1 / tau and 1 / n_j as one division each followed by products: its distance from the float64 evaluation is what float32 arithmetic costs
on those inputs, and ``measured_bar`` is BAR_FACTOR times that (the project's rule, spatial_restatement.measured_bar).  ``bug`` plants one
of four mistakes (tests/test_rt_spatial_host.py shows that the bar sees each of them).  Nothing here knows about the device."""
import numpy as np

import spatial_restatement as SR

LOADING, BAR_FACTOR = SR.LOADING, SR.BAR_FACTOR
TINY = 2.0 ** -126
BUGS = ('update_after_use', 'no_carry', 'no_residual', 'no_skip')


def components(Y, X, multi):
    """Y (NY, 2, F, T), X (2, F, T) -> E (NC, 2, F, T) complex64."""
    Y, X = np.asarray(Y).astype(np.complex64), np.asarray(X).astype(np.complex64)
    if multi:
        return Y
    assert Y.shape[0] == 1
    with np.errstate(invalid='ignore', over='ignore'):
        resid = np.empty_like(Y[0])
        resid.real, resid.imag = X.real - Y[0].real, X.imag - Y[0].imag       # one float32 rounding per component
    return np.stack([Y[0], resid])


def statistics(E, dtype):
    """E (NC, 2, F) complex64, one frame -> c (NC, F, 4) in ``dtype``."""
    r0, i0, r1, i1 = (a.astype(dtype) for a in (E[:, 0].real, E[:, 0].imag, E[:, 1].real, E[:, 1].imag))
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([r0 * r0 + i0 * i0, r1 * r1 + i1 * i1, r0 * r1 + i0 * i1, i0 * r1 - r0 * i1], axis=-1)


def loaded_covariances(P, dtype=np.float64):
    """State P (NC, F, 4) float32 -> R~ (NC, F, 4) in ``dtype`` (float64: not yet rounded to float32)."""
    P = np.asarray(P, np.float32).astype(dtype)
    one, lam = dtype(1.0), dtype(LOADING)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        n = dtype(0.5) * (P[..., 0] + P[..., 1])
        ident = n < dtype(TINY)
        if dtype == np.float32:
            R = P * (one / np.where(ident, one, n))[..., None]                  # one division, then products
        else:
            R = P / np.where(ident, one, n)[..., None]
        R = np.where(ident[..., None], np.array([1, 1, 0, 0], dtype), R)
        R[..., :2] = R[..., :2] + lam
    return R.astype(dtype)


def rt_spatial(Y, X, P, tau, multi, dtype=np.float64, bug=None):
    """Y (NY, 2, F, T) complex64 as the mask kernel wrote it (NY = N in multiple mode, 1 otherwise), X (2, F, T) complex64, P (NC, F, 4)
    float32 the state before the call, tau the time constant in frames -> (Y' (NY, 2, F, T) complex, P (NC, F, 4) float32 after)."""
    assert bug is None or bug in BUGS or bug == 'identity'
    X = np.asarray(X).astype(np.complex64)
    E = components(Y, X, multi)
    if bug == 'no_residual' and not multi:
        E = E[:1]
        P = np.asarray(P)[:1]
    NC, _, F, T = E.shape
    P0 = np.asarray(P, np.float32).copy()
    assert P0.shape == (NC, F, 4), (P0.shape, (NC, F, 4))
    tau = dtype(np.float32(tau))
    b = dtype(1.0) / tau
    a = dtype(1.0) - b
    P = P0.copy()
    out = np.zeros(E.shape, np.complex128 if dtype == np.float64 else np.complex64)
    for t in range(T):
        Et, Xt = E[..., t], X[..., t]
        c = statistics(Et, dtype)
        finite = np.isfinite(Xt.real).all(axis=0) & np.isfinite(Xt.imag).all(axis=0) & np.isfinite(c.astype(np.float32)).all(axis=(0, 2))
        if bug == 'no_skip':
            finite = np.ones_like(finite)
        prior = P0 if bug == 'no_carry' else P
        with np.errstate(invalid='ignore', over='ignore', under='ignore'):
            new = np.where(finite[None, :, None], (a * prior.astype(dtype) + b * c).astype(np.float32), prior)
        used = prior if bug == 'update_after_use' else np.zeros_like(new) if bug == 'identity' else new      # identity: R~ = (1 + LOADING) I
        P = new
        out[..., t] = SR.spatial_filter(Et[..., None], Xt[..., None], dtype, R=loaded_covariances(used, dtype))[..., 0]
    return (out if multi else out[:1]), P


def measured_bar(Y, X, P, tau, multi):
    """-> dict: Y64, P64 (the contract), Y32, P32 (its float32 evaluation), err_Y (relative to max|X|), err_P (relative to the largest state
    entry), bar_Y, bar_P = BAR_FACTOR x those.  A non-finite element must be non-finite in both evaluations."""
    Y64, P64 = rt_spatial(Y, X, P, tau, multi, np.float64)
    Y32, P32 = rt_spatial(Y, X, P, tau, multi, np.float32)
    assert np.array_equal(np.isfinite(Y64), np.isfinite(Y32))
    ok = np.isfinite(Y64)
    X = np.asarray(X)
    fin = np.abs(X[np.isfinite(X)])
    scale_Y = float(fin.max()) if fin.size and fin.max() > 0 else 1.0
    scale_P = float(np.abs(P64).max()) or 1.0
    err_Y = float(np.abs(Y32[ok] - Y64[ok]).max()) / scale_Y if ok.any() else 0.0
    err_P = float(np.abs(P32.astype(np.float64) - P64).max()) / scale_P
    return dict(Y64=Y64, P64=P64, Y32=Y32, P32=P32, scale_Y=scale_Y, scale_P=scale_P, err_Y=err_Y, err_P=err_P,
                bar_Y=BAR_FACTOR * err_Y, bar_P=BAR_FACTOR * err_P)


def distance(got_Y, got_P, m):
    """Largest distances of (got_Y, got_P) from the contract in the units of ``measured_bar``; a non-finite element of the contract must be
    non-finite in got_Y too (and only those)."""
    ok = np.isfinite(m['Y64'])
    assert np.array_equal(np.isfinite(got_Y), ok), 'non-finite elements differ from the restatement'
    dY = float(np.abs(np.asarray(got_Y).astype(np.complex128)[ok] - m['Y64'][ok]).max()) / m['scale_Y'] if ok.any() else 0.0
    dP = float(np.abs(np.asarray(got_P).astype(np.float64) - m['P64']).max()) / m['scale_P']
    return dY, dP


def random_state(NC, F, seed, scale=1.0):
    """A random positive-semidefinite state (NC, F, 4) float32: the sum of two random rank-1 outer products per (component, bin)."""
    rng = np.random.RandomState(seed)
    z = (rng.standard_normal((2, NC, F, 2)) + 1j * rng.standard_normal((2, NC, F, 2))) * scale
    p0, p1 = (np.abs(z[..., 0]) ** 2).sum(axis=0), (np.abs(z[..., 1]) ** 2).sum(axis=0)
    q = (z[..., 0] * np.conj(z[..., 1])).sum(axis=0)
    return np.stack([p0, p1, q.real, q.imag], axis=-1).astype(np.float32)
