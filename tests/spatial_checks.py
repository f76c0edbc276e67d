"""Element-wise checks of the offline spatial reconstruction and its EM refinement (csrc/spatial.hip, csrc/spatial_em.hip and the
arithmetic of csrc/spatial.h; include/gccnmf_hip.h, gccnmf_reconstruct).  Plain NumPy; nothing here knows about the device.
tests/test_spatial_checks_host.py runs it on NumPy's own float32, tests/test_gpu_spatial_stages.py on what the device returned.

Four parts.

1. Structured problems (``structured``): the inputs of the call -- W, H, an arg-max image or soft masks, X -- built so that the ratio
   stage produces estimates with spatial structure and dynamic range, where tests/test_gpu_spatial_reconstruction.py draws |X| in
   [0.5, 2] with independent phases (``uniform``: kept as one cell, so that both regimes are seen side by side).
2. The device's summation order, restated exactly (``device_sum``), and with it a float32 model of every stage that is meant to equal
   the device bit for bit (``model_stages``): SR.covariances, SR.spatial_filter, EM.em_step and EM.filter_with hold the per-element
   roundings, only the order of the float64 frame sums is the device's here.
3. A derived bar for every element of every output (``bar_filter``, ``bar_em_powers``, ``bar_em_cov``), by running error analysis on
   exact float32 inputs: no measured factor and no max|X|.
4. The cell table (``CELLS``) and the one function that checks a cell's stages (``check_cell``), whoever produced them.

The rounding model of part 3.  u = 2^-24.  A float32 product, sum, difference or quotient of float32 numbers is the exact result times
(1 + d), |d| <= u, plus, for products and quotients only, an absolute |eta| <= 2^-150 where the result is subnormal (sums of float32
numbers are exact there); a product with a power of two (ldexp, 0.5 *, 2 *) is exact, up to eta.  A quantity is carried as a pair
(x, e): x its exact value on the exact inputs, evaluated in float64, and e a bound of |float32 result - x|.  With a = (x_a, e_a),
b = (x_b, e_b):

    a * b    x = x_a x_b,   e = t + u (|x| + t) + eta,   t = |x_a| e_b + |x_b| e_a + e_a e_b
    a +- b   x = x_a +- x_b,  e = t + u (|x| + t),       t = e_a + e_b
    2^k a    x = 2^k x_a,   e = 2^k e_a + eta
    1 / a    only where |x_a| > 2 e_a (the guard; an element behind a failed guard cannot be checked):
             x = 1 / x_a,   e = e_a / (|x_a| (|x_a| - e_a)) + u / (|x_a| - e_a) + eta

-- every term is the first-order one plus its exact remainder, nothing is dropped.  A sum of non-negative terms so carries (roundings
on its path) u relative to itself, a signed sum the same relative to the sum of the absolute values, and the determinant
a d - (br^2 + bi^2) is bounded against a d + br^2 + bi^2, as one expects.  The formulas are those of csrc/spatial.h in the order
written there, on w_j = v_j 2^-e (e the binary exponent of the float64 sum of the v_j: a power of two changes no relative bound, so it
need not be the device's e where the two differ by one).  Every bar is multiplied by SLACK, which covers the float64 evaluation of x
and e themselves.  Roundings counted per output: see each bar function."""
import numpy as np

import ratio_restatement as RR
import spatial_em_restatement as EM
import spatial_restatement as SR

U = 2.0 ** -24
ETA = 2.0 ** -148                   # twice the half-spacing of the subnormal float32 numbers: the scaling exponent may be off by one
SLACK = 1.001
LOADING = SR.LOADING
K_ATOMS = 16


# ---- 1. problems ---------------------------------------------------------------------------------------------------------------------

def uniform(F, T, S, seed, K=K_ATOMS, tiny_frame=None):
    """The inputs of tests/test_gpu_spatial_reconstruction.py: |X| in [0.5, 2], independent phases, uniform W and H, a random arg-max."""
    rng = np.random.RandomState(seed)
    X = (rng.uniform(0.5, 2.0, (2, F, T)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (2, F, T)))).astype(np.complex64)
    W = rng.uniform(0.01, 1.0, (F, K)).astype(np.float32)
    W[F - 1] *= np.float32(100)
    W[:, K - 1] *= np.float32(100)
    H = rng.uniform(0.01, 1.0, (K, 2 * T)).astype(np.float32)
    am = rng.randint(0, S, (K, T)).astype(np.uint8)
    if tiny_frame is not None:
        X[:, :, tiny_frame] *= np.float32(1e-10)
    return W, H, am, None, X


def structured(F, T, S, seed, K=K_ATOMS, weak=None, absent=None, zero_bin=None, zero_frame=None, tiny_frame=None, soft=False):
    """-> (W (F, K), H (K, 2T), argmax (K, T) uint8, masks (S, K, T) float32 or None, X (2, F, T) complex64).

    X is the sum of S source images g_i[f,t] (1, a_i exp(-j phi_i f)): every source has its own level ratio a_i and delay phi_i, the
    level falls 60 dB over the bins and up to 30 dB over the frames, and every source has another 20 dB of its own scatter.  Atom k
    belongs to target k mod S; W carries the spectral shape, H the per-frame and per-channel levels of the atom's target, so the
    ratio stage's mask of target i follows that target's share.  weak = (i, dB): target i's image and coefficients are dB down
    (amplitude), so its estimates are about 10^(-dB/20) of X, its powers the square of that.  absent = (i, f): target i's atoms are 0 in
    bin f (n = 0, R = I).  zero_bin / zero_frame: X exactly 0 there.  tiny_frame: that frame of X times 1e-10.  soft: float masks 0.9 one-hot + 0.1 / S (den = W.H_c)."""
    rng = np.random.RandomState(seed)
    f = np.arange(F)[:, None]
    lev = 10.0 ** (-3.0 * f / max(F - 1, 1))
    env = 10.0 ** (-1.5 * rng.uniform(0, 1, (1, T)))
    owner = np.arange(K) % S
    gain = np.ones(S)
    if weak is not None:
        gain[weak[0]] = 10.0 ** (-weak[1] / 20.0)
    a = 0.5 + 0.4 * np.arange(S) / max(S - 1, 1)
    X = np.zeros((2, F, T), np.complex128)
    for i in range(S):
        g = (rng.randn(F, T) + 1j * rng.randn(F, T)) * lev * env * 10.0 ** (-rng.uniform(0, 1, (F, T))) * gain[i]
        if absent is not None and absent[0] == i:
            g[absent[1]] = 0
        X[0] += g
        X[1] += a[i] * np.exp(-2j * np.pi * (i - S / 2.0) * 3 * f / (2.0 * F)) * g
    W = lev * 10.0 ** (-rng.uniform(0, 1, (F, K)))
    if absent is not None:
        W[absent[1], owner == absent[0]] = 0
    H = np.empty((K, 2 * T))
    for c in range(2):
        H[:, c * T:(c + 1) * T] = (gain[owner] * (a[owner] if c else 1.0))[:, None] * env * rng.uniform(0.5, 1.0, (K, T))
    if zero_bin is not None:
        X[:, zero_bin] = 0
    if zero_frame is not None:
        X[:, :, zero_frame] = 0
    if tiny_frame is not None:
        X[:, :, tiny_frame] *= 1e-10
    am = np.repeat(owner[:, None], T, axis=1).astype(np.uint8)
    masks = None
    if soft:
        masks = (0.9 * RR.one_hot(am, S) + 0.1 / S).astype(np.float32)
    return W.astype(np.float32), H.astype(np.float32), am, masks, X.astype(np.complex64)


def host_ratio(problem, S):
    """The ratio stage's estimates of a problem by its restatement, rounded to float32: what stands in for the device's spec on the host."""
    W, H, am, masks, X = problem
    with np.errstate(invalid='ignore'):
        E = RR.ratio_one_hot(W, H, am, S, X) if masks is None else RR.ratio_soft(W, H, masks, X)
    return E.astype(np.complex64)


# ---- 2. the device's order, and the float32 model ------------------------------------------------------------------------------------

def device_sum(x):
    """float64 (..., T) -> (...): the order of gcc_spatial_cov_kernel and gcc_spatial_em_kernel.  Lane l adds its frames 2l, 2l+1,
    2l+128, 2l+129, ... sequentially to +0.0; the 64 partials are combined by x[l] += x[l ^ k] for k = 1, 2, 4, 8, 16, 32 (a + b = b + a:
    every lane ends with the same sum).  A frame the device does not add (t >= T, or a skipped frame of the EM sum) is a +0.0 here:
    the same bits, since a partial that started as +0.0 is never -0.0."""
    x = np.asarray(x, np.float64)
    T = x.shape[-1]
    sweeps = -(-T // 128)
    z = np.concatenate([x, np.zeros(x.shape[:-1] + (sweeps * 128 - T,))], axis=-1).reshape(x.shape[:-1] + (sweeps, 64, 2))
    with np.errstate(invalid='ignore', over='ignore'):
        part = np.zeros(x.shape[:-1] + (64,))
        for s in range(sweeps):
            part = part + z[..., s, :, 0]
            part = part + z[..., s, :, 1]
        lanes = np.arange(64)
        for k in (1, 2, 4, 8, 16, 32):
            part = part + part[..., lanes ^ k]
    return part[..., 0]


def ascending_sum(x):
    return np.cumsum(np.asarray(x, np.float64), axis=-1)[..., -1]


def em_close(sums, use, loading='trace', count='used'):
    """Step 2 of the iteration after the sums: R' = A / n (I when n = 0), R~' = R' + lambda 1/2 tr(R') I, in float64 before the one
    rounding -- the formulas of EM.em_step.  loading='lambda' and count='all' are planted mistakes."""
    cnt = (use.sum(axis=-1) if count == 'used' else np.full(use.shape[0], use.shape[1])).astype(np.float64)
    none = cnt == 0
    den = np.where(none, 1.0, cnt)
    with np.errstate(invalid='ignore', over='ignore'):
        r00, r11 = np.where(none, 1.0, sums[0] / den), np.where(none, 1.0, sums[1] / den)
        rr, ri = np.where(none, 0.0, sums[2] / den), np.where(none, 0.0, sums[3] / den)
        load = LOADING * (0.5 * (r00 + r11)) if loading == 'trace' else LOADING
        return np.stack([r00 + load, r11 + load, rr, ri], axis=-1)


def model_cov(E, frame_sum=device_sum):
    return SR.covariances(E, frame_sum=frame_sum)


def model_filter(E, X, R):
    """gcc_spatial_filter_kernel<S, false>: the powers from the estimates."""
    return SR.spatial_filter(E, X, np.float32, R=R)


def model_filter_ws(v, R, X):
    """gcc_spatial_filter_kernel<S, true>: the powers from the workspace."""
    return EM.filter_with(np.asarray(v, np.float32), R, X, np.float32)


def model_em_step(v, R, X, frame_sum=device_sum, **variant):
    return EM.em_step(np.asarray(v, np.float32), R, X, np.float32, frame_sum=frame_sum, **variant)


def reference_em_step(v, R, X):
    """One float64 iteration from float32 state -> (v' float64, R~' float64 BEFORE its rounding to float32, the frames counted)."""
    kept = []

    def close(sums, use):
        kept.append((em_close(sums, use), use))
        return kept[-1][0]
    vn, _ = EM.em_step(np.asarray(v, np.float32).astype(np.float64), R, X, np.float64, close=close)
    return vn, np.stack([k[0] for k in kept]), np.stack([k[1] for k in kept])


MISTAKES = ('flip_im', 'drop_sigma', 'zero_weak', 'drop128', 'odd_twice', 'r_first', 'power', 'lambda', 'count_all')


def model_stages(E, X, n, mistake=None, target=0):
    """Every stage of calls with 0 ... n iterations on the estimates E, as the float32 model has them: the dictionary check_cell reads.
    ``mistake`` plants one of MISTAKES (``target``: the target it concerns) in every stage it applies to."""
    assert mistake is None or mistake in MISTAKES
    T = E.shape[-1]
    fs = device_sum
    if mistake == 'drop128':
        fs = lambda x: device_sum(np.asarray(x)[..., :128])
    if mistake == 'odd_twice':
        fs = lambda x: device_sum(np.concatenate([x, x[..., -1:]], axis=-1)) if T % 2 else device_sum(x)
    variant = {}
    if mistake == 'r_first':
        variant = dict(order='r_first')
    if mistake == 'power':
        variant = dict(weighting='power')
    if mistake == 'lambda':
        variant = dict(close=lambda sums, use: em_close(sums, use, loading='lambda'))
    if mistake == 'count_all':
        variant = dict(close=lambda sums, use: em_close(sums, use, count='all'))

    def output(v, R):
        R = np.array(R)
        if mistake == 'flip_im':
            R[target, :, 3] *= -1
        if mistake == 'drop_sigma':                            # Sigma without the target, its output from that y
            v0 = np.array(v)
            v0[target] = 0
            with np.errstate(all='ignore'):
                out = EM.filter_with(v0, R, X, np.float32)
                _, e, _, _, _, y = EM._solve(v0, R.astype(np.float32), EM._planes(X, np.float32), np.float32, True)
                u = EM._u(R.astype(np.float32), target, y)
                w = np.ldexp(v[target], -e).astype(np.float32)
                out[target, 0] = w * u[0] + 1j * (w * u[1])
                out[target, 1] = w * u[2] + 1j * (w * u[3])
            return out
        out = EM.filter_with(v, R, X, np.float32)
        if mistake == 'zero_weak':
            out[target] = 0
        return out

    v, R = SR.powers(E, np.float32), model_cov(E, fs)
    stages = dict(E=E, X=X, cov=[R], powers=[None], out=[output(v, R)])
    for _ in range(n):
        v, R = model_em_step(v, R, X, fs, **variant)
        stages['cov'].append(R)
        stages['powers'].append(v)
        stages['out'].append(output(v, R))
    return stages


# ---- 3. the bars ---------------------------------------------------------------------------------------------------------------------

class Q(object):
    """(x, e): an exact value and a bound of the float32 result's distance from it (the module's header)."""
    __slots__ = ('x', 'e')

    def __init__(self, x, e=0.0):
        self.x, self.e = np.asarray(x, np.float64), e


def _mul(a, b):
    with np.errstate(invalid='ignore', over='ignore'):         # behind a failed guard e is inf, and 0 * inf a NaN: never compared
        x = a.x * b.x
        t = np.abs(a.x) * b.e + np.abs(b.x) * a.e + a.e * b.e
        return Q(x, t + U * (np.abs(x) + t) + ETA)


def _add(a, b, sign=1.0):
    with np.errstate(invalid='ignore', over='ignore'):
        x = a.x + sign * b.x
        t = a.e + b.e
        return Q(x, t + U * (np.abs(x) + t))


def _sub(a, b):
    return _add(a, b, -1.0)


def _pow2(a, c):
    return Q(a.x * c, a.e * c + ETA)


def _inv(a):
    """-> (1 / a, guard).  Behind a failed guard the pair is (0, inf)."""
    ok = np.abs(a.x) > 2 * a.e
    lo = np.where(ok, np.abs(a.x) - a.e, 1.0)
    x = np.where(ok, 1.0 / np.where(ok, a.x, 1.0), 0.0)
    e = np.where(ok, a.e / (np.where(ok, np.abs(a.x), 1.0) * lo) + U / lo + ETA, np.inf)
    return Q(x, e), ok


def _sum(terms):
    s = terms[0]
    for t in terms[1:]:
        s = _add(s, t)
    return s


def q_powers(E):
    """spatial_power on exact estimates: 4 products, 3 sums, the half."""
    E = np.asarray(E).astype(np.complex64)
    r0, i0, r1, i1 = (Q(p) for p in (E[:, 0].real, E[:, 0].imag, E[:, 1].real, E[:, 1].imag))
    v = _pow2(_add(_add(_mul(r0, r0), _mul(i0, i0)), _add(_mul(r1, r1), _mul(i1, i1))), 0.5)
    return [Q(v.x[i], v.e[i]) for i in range(E.shape[0])]


def q_exact(v):
    """Powers that the device read from its workspace: exact inputs."""
    v = np.asarray(v, np.float32)
    return [Q(v[i]) for i in range(v.shape[0])]


def _rows(R):
    R = np.asarray(R, np.float32).astype(np.float64)
    return [[Q(R[j, :, k][:, None]) for k in range(4)] for j in range(R.shape[0])]


def _q_solve(v, R, X):
    """spatial_solve: w, Sigma_w, 1 / det and y, and the guard of the reciprocal."""
    S = len(v)
    r = _rows(R)
    X = np.asarray(X).astype(np.complex64)
    x0r, x0i, x1r, x1i = (Q(p) for p in (X[0].real, X[0].imag, X[1].real, X[1].imag))
    total = sum(q.x for q in v)
    live = np.isfinite(total) & (total > 0)
    e = np.where(live, np.frexp(np.where(live, total, 1.0))[1], 0)
    down, up = np.ldexp(1.0, -e), np.ldexp(1.0, e)
    w = [_pow2(q, down) for q in v]
    a, d, br, bi = (_sum([_mul(w[j], r[j][k]) for j in range(S)]) for k in range(4))
    det = _sub(_mul(a, d), _add(_mul(br, br), _mul(bi, bi)))
    rdet, ok = _inv(det)
    y0r = _mul(_sub(_mul(d, x0r), _sub(_mul(br, x1r), _mul(bi, x1i))), rdet)
    y0i = _mul(_sub(_mul(d, x0i), _add(_mul(br, x1i), _mul(bi, x1r))), rdet)
    y1r = _mul(_sub(_mul(a, x1r), _add(_mul(br, x0r), _mul(bi, x0i))), rdet)
    y1i = _mul(_sub(_mul(a, x1i), _sub(_mul(br, x0i), _mul(bi, x0r))), rdet)
    return dict(r=r, w=w, up=up, a=a, d=d, br=br, bi=bi, rdet=rdet, y=(y0r, y0i, y1r, y1i), ok=ok & live, live=live)


def _q_apply(r, y):
    """spatial_apply: u = R~ y in the association of the filter's output."""
    y0r, y0i, y1r, y1i = y
    return (_add(_mul(r[0], y0r), _sub(_mul(r[2], y1r), _mul(r[3], y1i))), _add(_mul(r[0], y0i), _add(_mul(r[2], y1i), _mul(r[3], y1r))),
            _add(_add(_mul(r[2], y0r), _mul(r[3], y0i)), _mul(r[1], y1r)), _add(_sub(_mul(r[2], y0i), _mul(r[3], y0r)), _mul(r[1], y1i)))


def bar_filter(v, R, X):
    """The filter's output w_i (R~_i y).  v: q_powers(E) (WS = false) or q_exact(powers) (WS = true); R (S, F, 4) float32; X.
    -> (bar_re, bar_im (S, 2, F, T), guard (F, T), value (S, 2, F, T) complex128 as this evaluation has it).

    Roundings on the path of one output, each relative to the quantity it rounds: v_i 7 (WS = false; 0 from the workspace);
    a, d, br, bi one product and S - 1 sums each on top of v; det 3 products, 2 sums; 1 / det 1; a numerator of y 3 products, 2 sums;
    y its product with 1 / det; u_i 3 products, 2 sums; the output its product with w_i.  The signed sums (det, the numerators, u_i)
    enter by their terms' bounds, so a cancelling sum keeps the bound of its parts.  Guard: |det| > 2 |delta det|."""
    g = _q_solve(v, R, X)
    S = len(v)
    shape = (S, 2) + g['ok'].shape
    bar_re, bar_im, value = np.zeros(shape), np.zeros(shape), np.zeros(shape, np.complex128)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(S):
            u = _q_apply(g['r'][i], g['y'])
            o = [_mul(g['w'][i], c) for c in u]
            for c in range(2):
                bar_re[i, c], bar_im[i, c] = SLACK * o[2 * c].e, SLACK * o[2 * c + 1].e
                value[i, c] = o[2 * c].x + 1j * o[2 * c + 1].x
    return bar_re, bar_im, g['ok'], value


def _q_em(v, R, X):
    """spatial_em_frame: per target the new power (before the clamp at 0), the four terms C"_i / v"_i and the guard of 1 / v"_i."""
    g = _q_solve(v, R, X)
    S = len(v)
    r, w, up, a, d, br, bi, rdet = g['r'], g['w'], g['up'], g['a'], g['d'], g['br'], g['bi'], g['rdet']
    y0r, y0i, y1r, y1i = g['y']
    zero = Q(np.zeros(g['ok'].shape))
    out = []
    for i in range(S):
        u0r, u0i, u1r, u1i = _q_apply(r[i], g['y'])
        others = [j for j in range(S) if j != i]
        n0, n1, nr, ni = (_sum([_mul(w[j], r[j][k]) for j in others]) if others else zero for k in range(4))
        k = _mul(_sub(_add(_mul(d, n0), _mul(a, n1)), _pow2(_add(_mul(br, nr), _mul(bi, ni)), 2.0)), rdet)
        h = _add(_add(_mul(y0r, u0r), _mul(y0i, u0i)), _add(_mul(y1r, u1r), _mul(y1i, u1i)))
        v2 = _pow2(_add(_mul(w[i], h), _pow2(k, up)), 0.5)
        vi = _mul(w[i], v2)
        x_, y_, z_, q_ = r[i]
        kk, ll = _add(_mul(br, z_), _mul(bi, q_)), _sub(_mul(bi, z_), _mul(br, q_))
        m00r = _sub(_mul(d, x_), kk)
        m11r, m11i = _sub(_mul(a, y_), kk), ll
        m01r, m01i = _sub(_mul(d, z_), _mul(br, y_)), _sub(_mul(d, q_), _mul(bi, y_))
        m10r, m10i = _sub(_mul(a, z_), _mul(br, x_)), _sub(_mul(bi, x_), _mul(a, q_))
        p00 = _mul(_add(_mul(n0, m00r), _sub(_mul(nr, m10r), _mul(ni, m10i))), rdet)
        p11 = _mul(_add(_add(_mul(nr, m01r), _mul(ni, m01i)), _mul(n1, m11r)), rdet)
        p01r = _mul(_add(_mul(n0, m01r), _sub(_mul(nr, m11r), _mul(ni, m11i))), rdet)
        p01i = _mul(_add(_mul(n0, m01i), _add(_mul(nr, m11i), _mul(ni, m11r))), rdet)
        rv, okv = _inv(v2)
        terms = (_mul(_add(_mul(w[i], _add(_mul(u0r, u0r), _mul(u0i, u0i))), _pow2(p00, up)), rv),
                 _mul(_add(_mul(w[i], _add(_mul(u1r, u1r), _mul(u1i, u1i))), _pow2(p11, up)), rv),
                 _mul(_add(_mul(w[i], _add(_mul(u0r, u1r), _mul(u0i, u1i))), _pow2(p01r, up)), rv),
                 _mul(_add(_mul(w[i], _sub(_mul(u0i, u1r), _mul(u0r, u1i))), _pow2(p01i, up)), rv))
        out.append((vi, terms, g['ok'] & okv))
    return g, out


def bar_em_powers(v, R, X):
    """The new powers v'_i = max(0, w_i v"_i), v"_i = 1/2 (w_i h_i + 2^e k_i).  -> (bar (S, F, T), guard (F, T), value (S, F, T)).

    On top of y and u_i (bar_filter): h_i = Re(y^H u_i) 4 products, 3 sums; N_i one product and S - 2 sums per entry; k_i 4 products,
    3 sums and the product with 1 / det; v"_i one product, one sum; v'_i its product with w_i.  max(0, .) moves nothing further than
    its argument moved.  Relative to the element itself this is near 10^2 ... 10^3 u: y carries the conditioning of Sigma_w.
    Guard: that of 1 / det."""
    g, per = _q_em(v, R, X)
    with np.errstate(invalid='ignore', over='ignore'):
        bar = np.stack([SLACK * vi.e for vi, _, _ in per])
        value = np.stack([np.maximum(vi.x, 0.0) for vi, _, _ in per])
    return bar, g['ok'], value


def bar_em_cov(v, R, X, use):
    """The new covariances R~'_i.  use (S, F, T): the frames counted (those whose new power is not 0).
    -> (bar (S, F, 4), guard (S, F), value (S, F, 4) before the rounding).

    A frame's term C"_i / v"_i: on top of u_i, N_i and 1 / det, M_i = det Sigma_w^-1 R~_i 2 products and up to 2 sums per entry, an
    entry of P_i 3 products, 2 sums and the product with 1 / det, w_i u u^H 3 products and one sum, the sum of the two, and the product
    with 1 / v"_i (v"_i as in bar_em_powers), whose guard is |v"_i| > 2 |delta v"_i|.  R'_i is the mean of the counted terms: it
    carries the mean of their bounds, plus 2^-50 of the mean of their absolute values for the float64 sum and quotient in any order;
    R~'_i = R'_i + lambda 1/2 tr(R'_i) I carries (1 + lambda / 2) of that on the diagonal plus lambda / 2 of the other diagonal
    entry's, and the one rounding to float32.  Where no frame is counted R~' = (1 + lambda) I exactly and the bar is that rounding's.
    Guard of an (i, f): every counted frame's guards hold."""
    _, per = _q_em(v, R, X)
    use = np.asarray(use, bool)
    S, F, _ = use.shape
    bar, value, guard = np.zeros((S, F, 4)), np.zeros((S, F, 4)), np.zeros((S, F), bool)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for i, (_, terms, ok) in enumerate(per):
            cnt = use[i].sum(axis=-1).astype(np.float64)
            none = cnt == 0
            den = np.where(none, 1.0, cnt)
            guard[i] = (ok | ~use[i]).all(axis=-1)
            mean = [np.where(use[i], t.x, 0.0).sum(axis=-1) / den for t in terms]
            err = [(np.where(use[i] & ok, t.e, 0.0).sum(axis=-1) + 2.0 ** -50 * np.where(use[i], np.abs(t.x), 0.0).sum(axis=-1)) / den
                   for t in terms]
            r00, r11 = np.where(none, 1.0, mean[0]), np.where(none, 1.0, mean[1])
            load = LOADING * 0.5 * (r00 + r11)
            eload = LOADING * 0.5 * (err[0] + err[1])
            value[i] = np.stack([r00 + load, r11 + load, np.where(none, 0.0, mean[2]), np.where(none, 0.0, mean[3])], axis=-1)
            e = np.stack([err[0] + eload, err[1] + eload, err[2], err[3]], axis=-1)
            e = np.where(none[:, None], 0.0, e)
            bar[i] = SLACK * (e + U * (np.abs(value[i]) + e))
    return bar, guard, value


# ---- 4. the cells and their check ----------------------------------------------------------------------------------------------------

# name: F, T, S, n iterations, batch, position of the cell's own file in it, how the file is built
CELLS = {
    'uniform':     dict(F=40, T=129, S=3, n=1, B=1, pos=0, kind='uniform', args={}),
    'one_frame':   dict(F=4, T=1, S=2, n=1, B=1, pos=0, kind='structured', args={}),
    'weak40_soft': dict(F=17, T=2, S=2, n=2, B=1, pos=0, kind='structured', args=dict(weak=(1, 40), soft=True)),
    'weak80':      dict(F=33, T=127, S=3, n=3, B=3, pos=0, kind='structured', args=dict(weak=(2, 80))),
    'absent':      dict(F=40, T=128, S=4, n=1, B=1, pos=0, kind='structured', args=dict(absent=(0, 7))),
    'zero_bin':    dict(F=17, T=129, S=5, n=2, B=1, pos=0, kind='structured', args=dict(zero_bin=3, soft=True)),
    'zero_frame':  dict(F=33, T=257, S=6, n=1, B=3, pos=2, kind='structured', args=dict(zero_frame=130)),
    'tiny_frame':  dict(F=40, T=257, S=7, n=1, B=1, pos=0, kind='structured', args=dict(tiny_frame=11)),
    'weak40':      dict(F=4, T=129, S=8, n=2, B=1, pos=0, kind='structured', args=dict(weak=(5, 40))),
    'one_target':  dict(F=17, T=128, S=1, n=3, B=1, pos=0, kind='structured', args={}),
}


def cell_files(name):
    """The B problems of a cell (the cell's own at ``pos``, uniform files of the same shape around it)."""
    c = CELLS[name]
    seed = 1000 + 7 * sorted(CELLS).index(name)
    build = structured if c['kind'] == 'structured' else uniform
    own = build(c['F'], c['T'], c['S'], seed, **c['args'])
    files = []
    for b in range(c['B']):
        if b == c['pos']:
            files.append(own)
        else:
            other = uniform(c['F'], c['T'], c['S'], seed + 1 + b)
            if own[3] is not None:                              # one call has one mask form
                other = other[:3] + ((0.9 * RR.one_hot(other[2], c['S']) + 0.1 / c['S']).astype(np.float32),) + other[4:]
            files.append(other)
    return files


def _compare(failures, what, got, ref, bar, ok, zeros_identical=False):
    """One real array against its float64 reference, element by element -> the largest share of a bar.  A NaN must be a NaN, an exact
    zero of the reference an exact zero; no other element may sit behind a failed guard."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.broadcast_to(ok, ref.shape)
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        failures.append('%s: NaN where the reference has none, or the reverse' % what)
    zero = ref == 0
    if not (got[zero] == 0).all():
        failures.append('%s: %d exact zeros of the reference are not zero' % (what, int((got[zero] != 0).sum())))
    if zeros_identical and not np.array_equal(got == 0, zero):
        failures.append('%s: the zero pattern differs' % what)
    rest = np.isfinite(ref) & ~zero
    if (rest & ~ok).any():
        failures.append('%s: %d elements behind a failed guard' % (what, int((rest & ~ok).sum())))
    m = rest & ok
    if not m.any():
        return 0.0
    with np.errstate(invalid='ignore', divide='ignore'):
        share = np.where(m & (got != ref), np.abs(got - ref) / np.where(m, bar, 1.0), 0.0)
    share = np.where(np.isnan(share), np.inf, share)
    worst = float(share.max())
    if worst > 1.0:
        at = np.unravel_index(int(share.argmax()), share.shape)
        failures.append('%s: %.3g of the bar at %s (got %.9g, reference %.9g, bar %.3g); %d elements over' %
                        (what, worst, at, got[at], ref[at], bar[at], int((share > 1.0).sum())))
    return worst


def _complex(failures, what, got, ref, bar_re, bar_im, ok):
    got, ref = np.asarray(got), np.asarray(ref)
    return max(_compare(failures, what + ' (re)', got.real, ref.real, bar_re, ok[None, None]),
               _compare(failures, what + ' (im)', got.imag, ref.imag, bar_im, ok[None, None]))


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_cell(stages, what=''):
    """stages: E (S, 2, F, T) complex64 the ratio estimates and X (2, F, T) as the producer held them; cov[m] (S, F, 4) float32,
    powers[m] (S, F, T) float32 (None for m = 0) and out[m] (S, 2, F, T) complex64 of a call with m iterations, m = 0 ... n.
    -> (failures under the bars, elements that are not the float32 model's bits, the largest share of a bar per output).
    Every stage is checked on the state the producer held before it."""
    E, X = stages['E'], stages['X']
    S = E.shape[0]
    n = len(stages['cov']) - 1
    fail, bits, share = [], [], {}

    def note(key, s):
        share[key] = max(share.get(key, 0.0), s)

    def mixture(m, bar_re, bar_im, ok):
        # sum_i w_i R~_i y = Sigma_w y = X: the targets add up to the mixture within the sum of their bars; one target returns it
        out = stages['out'][m].astype(np.complex128)
        Xc = np.asarray(X).astype(np.complex128)
        live = (np.abs(out).sum(axis=0) != 0).any(axis=0)
        total = np.where(live[None], out.sum(axis=0), Xc)
        f = []
        s = _complex(f, '%s n=%d sum of the targets' % (what, m), total[None], Xc[None], bar_re.sum(axis=0)[None] + 1e-300,
                     bar_im.sum(axis=0)[None] + 1e-300, ok | ~live)
        fail.extend(x for x in f if 'of the bar' in x)
        note('sum of the targets', s)

    # the covariance launch: within one float32 ulp of the ascending-order sums, and bit for bit the exact-order restatement
    asc = SR.covariances(E).astype(np.float64)
    note('covariance launch (ulp)', _compare(fail, '%s covariance launch' % what, stages['cov'][0], asc,
                                             np.spacing(np.abs(asc).astype(np.float32)).astype(np.float64) + 2.0 ** -40, np.ones((), bool)))
    cov0 = model_cov(E)
    if not _bits(stages['cov'][0], cov0):
        bits.append('%s covariance launch: %d entries differ' % (what, int((stages['cov'][0] != cov0).sum())))
    # the filter, WS = false
    ref = SR.spatial_filter(E, X, np.float64, R=stages['cov'][0])
    bar_re, bar_im, ok, value = bar_filter(q_powers(E), stages['cov'][0], X)
    note('filter', _complex(fail, '%s filter' % what, stages['out'][0], ref, bar_re, bar_im, ok))
    mixture(0, bar_re, bar_im, ok)
    model = model_filter(E, X, stages['cov'][0])
    if not _bits(stages['out'][0], model):
        bits.append('%s filter: %d elements differ' % (what, int((stages['out'][0] != model).sum())))
    for m in range(1, n + 1):
        before = SR.powers(E, np.float32) if m == 1 else stages['powers'][m - 1]
        qv = q_powers(E) if m == 1 else q_exact(before)
        R = stages['cov'][m - 1]
        vref, Rref, use = reference_em_step(before, R, X)
        tag = '%s iteration %d' % (what, m)
        bar, ok, _ = bar_em_powers(qv, R, X)
        note('EM powers', _compare(fail, tag + ' powers', stages['powers'][m], vref, bar, ok[None], zeros_identical=True))
        bar, okc, _ = bar_em_cov(qv, R, X, use)
        note('EM covariances', _compare(fail, tag + ' covariances', stages['cov'][m], Rref, bar, okc[..., None]))
        mv, mR = model_em_step(before, R, X)
        if not _bits(stages['powers'][m], mv):
            bits.append('%s powers: %d elements differ' % (tag, int((stages['powers'][m] != mv).sum())))
        if not _bits(stages['cov'][m], mR):
            bits.append('%s covariances: %d entries differ' % (tag, int((stages['cov'][m] != mR).sum())))
        # the filter, WS = true, on that call's own workspace
        ref = EM.filter_with(stages['powers'][m], stages['cov'][m], X, np.float64)
        bar_re, bar_im, ok, _ = bar_filter(q_exact(stages['powers'][m]), stages['cov'][m], X)
        note('filter from the workspace', _complex(fail, '%s n=%d filter from the workspace' % (what, m), stages['out'][m], ref, bar_re, bar_im, ok))
        mixture(m, bar_re, bar_im, ok)
        model = model_filter_ws(stages['powers'][m], stages['cov'][m], X)
        if not _bits(stages['out'][m], model):
            bits.append('%s n=%d filter from the workspace: %d elements differ' % (what, m, int((stages['out'][m] != model).sum())))
    if S == 1:
        for m in range(n + 1):
            f = []
            Xc = np.asarray(X).astype(np.complex128)
            b = bar_filter(q_powers(E) if m == 0 else q_exact(stages['powers'][m]), stages['cov'][m], X)
            note('one target returns the mixture', _complex(f, '%s n=%d one target' % (what, m), stages['out'][m], Xc[None], b[0], b[1], b[2]))
            fail.extend(f)
    return fail, bits, share
