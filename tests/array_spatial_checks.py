"""Element-wise checks of the M x M spatial filter of the microphone-array path (csrc/array_spatial.hip, include/gccnmf_array_spatial.h):
the M-channel form of tests/spatial_checks.py, whose rounding model (Q, _mul, _add, _sub, _inv, _pow2, SLACK), summation order
(device_sum) and comparison rules it takes as they are.  Plain NumPy; nothing here knows about the device.
tests/test_array_spatial_host.py runs it on NumPy's own float32, tests/test_gpu_array_spatial_stages.py on what the device returned.

1. ``structured``: the M-channel extension of spatial_checks.structured -- every source has its own per-channel gains and delays, the
   level falls 60 dB over the bins, and the options weak, absent, zero_bin, zero_frame and tiny_frame mean what they mean there.
2. ``bar_filter_M``: a derived bar for every element of the filter's output.  A quantity is a pair (x, e) as in spatial_checks; the
   pairs go through the LDL^H steps, the substitutions and the output products in the kernel's order -- through the very lines of
   array_spatial_restatement.ldl_solve and apply_row, which take any operands with *, + and - -- with _inv's guard on every pivot d_k.
   No measured factor and no max|X|.  Roundings on the path of one output: a power 2 M products, 2 M - 1 sums and the quotient by M;
   a component of Sigma_w one product and S - 1 sums on top; the factorisation, the substitutions and u = R~ y as the header writes
   them (of the order of M^3 / 3 + 2 M^2 complex multiply-subtracts); the output its product with w_i.
3. ``CELLS`` and ``check_cell``: the cells (M, S, F, T, batch) of the device test and the one function that checks a cell's two stages,
   whoever produced them."""
import numpy as np

import array_restatement as A
import array_spatial_restatement as AS
import spatial_checks as SC
from spatial_checks import Q, _mul, _add, _sub, _inv, _pow2, SLACK

U, ETA = SC.U, SC.ETA
K_ATOMS = 16
GUARD_CAP = 1e-3                    # the share of a cell's non-zero finite elements that may sit behind a failed guard


# ---- 1. problems ---------------------------------------------------------------------------------------------------------------------

def structured(M, F, T, S, seed, K=K_ATOMS, weak=None, absent=None, zero_bin=None, zero_frame=None, tiny_frame=None, line=False):
    """-> (W (F, K), H (K, M T), argmax (K, T) uint8, X (M, F, T) complex64).

    X is the sum of S source images g_i[f,t] a_i,c exp(-j phi_i,c f): source i has its own gain at every channel (1 at channel 0,
    drawn from [0.5, 1] elsewhere) and its own delay at every channel (0 at channel 0, up to +- 3 samples elsewhere: an irregular
    array, so that the S steering vectors are in general position in every bin -- with the delays of a line array they coincide
    in the low bins and wherever the phases alias, Sigma_w is then M - 1 pivots of the size of the loading, and the running bounds of
    bar_filter_M grow by 1 / d_k at each of them until a guard fails), the level falls 60 dB over the bins and up to 30 dB over the
    frames, and every source has another 20 dB of its own scatter.  Atom k belongs to target k mod S; W carries the spectral shape, H
    the per-frame and per-channel levels of the atom's target.  The options are those of spatial_checks.structured.  line: the
    gains and delays of a line array instead (gain falling linearly along the channels, delay proportional to the channel): the
    regime in which the running bounds give up, kept for the normwise bar below."""
    rng = np.random.RandomState(seed)
    f = np.arange(F)[:, None]
    lev = 10.0 ** (-3.0 * f / max(F - 1, 1))
    env = 10.0 ** (-1.5 * rng.uniform(0, 1, (1, T)))
    owner = np.arange(K) % S
    gain = np.ones(S)
    if weak is not None:
        gain[weak[0]] = 10.0 ** (-weak[1] / 20.0)
    place = np.random.RandomState(seed + 7919)                 # the array: its own stream, so that the options change nothing else
    a = place.uniform(0.5, 1.0, (S, M))
    delay = place.uniform(-3.0, 3.0, (S, M))
    a[:, 0], delay[:, 0] = 1.0, 0.0
    if line:
        a = 1.0 - (1.0 - a[:, -1:]) * np.arange(M)[None] / (M - 1.0)
        delay = place.uniform(-1.5, 1.5, (S, 1)) * np.arange(M)[None]
    X = np.zeros((M, F, T), np.complex128)
    for i in range(S):
        g = (rng.randn(F, T) + 1j * rng.randn(F, T)) * lev * env * 10.0 ** (-rng.uniform(0, 1, (F, T))) * gain[i]
        if absent is not None and absent[0] == i:
            g[absent[1]] = 0
        for c in range(M):
            X[c] += a[i, c] * np.exp(-2j * np.pi * delay[i, c] * f / (2.0 * F)) * g
    W = lev * 10.0 ** (-rng.uniform(0, 1, (F, K)))
    if absent is not None:
        W[absent[1], owner == absent[0]] = 0
    H = np.empty((K, M * T))
    for c in range(M):
        H[:, c * T:(c + 1) * T] = (gain[owner] * a[owner, c])[:, None] * env * rng.uniform(0.5, 1.0, (K, T))
    if zero_bin is not None:
        X[:, zero_bin] = 0
    if zero_frame is not None:
        X[:, :, zero_frame] = 0
    if tiny_frame is not None:
        X[:, :, tiny_frame] *= 1e-10
    am = np.repeat(owner[:, None], T, axis=1).astype(np.uint8)
    return W.astype(np.float32), H.astype(np.float32), am, X.astype(np.complex64)


def uniform(M, F, T, S, seed, K=K_ATOMS):
    """A file beside the cell's own in a batch: |X| in [0.5, 2], independent phases, uniform W and H, a random arg-max."""
    rng = np.random.RandomState(seed)
    X = (rng.uniform(0.5, 2.0, (M, F, T)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (M, F, T)))).astype(np.complex64)
    W = rng.uniform(0.01, 1.0, (F, K)).astype(np.float32)
    H = rng.uniform(0.01, 1.0, (K, M * T)).astype(np.float32)
    am = rng.randint(0, S, (K, T)).astype(np.uint8)
    return W, H, am, X


def host_ratio(problem, S):
    """The ratio stage's estimates of a problem by its restatement, rounded to float32: what stands in for the device's spec on the host."""
    W, H, am, X = problem
    with np.errstate(invalid='ignore'):
        return A.ratio_one_hot(W, H, am, S, X).astype(np.complex64)


# ---- 2. the bar ----------------------------------------------------------------------------------------------------------------------

class Pair(object):
    """A Q of spatial_checks with the operators array_spatial_restatement.ldl_solve and apply_row use."""
    __slots__ = ('q',)

    def __init__(self, q):
        self.q = q

    def __mul__(self, o):
        return Pair(_mul(self.q, o.q))

    def __add__(self, o):
        return Pair(_add(self.q, o.q))

    def __sub__(self, o):
        return Pair(_sub(self.q, o.q))

    def __neg__(self):
        return Pair(Q(-self.q.x, self.q.e))                    # exact


def q_powers(E):
    """The powers on exact estimates: per channel 2 products and a sum, M - 1 sums, the quotient by M (one rounding)."""
    E = np.asarray(E).astype(np.complex64)
    S, M = E.shape[:2]
    out = []
    for i in range(S):
        s = None
        for c in range(M):
            r, im = Q(E[i, c].real), Q(E[i, c].imag)
            term = _add(_mul(r, r), _mul(im, im))
            s = term if s is None else _add(s, term)
        x, e = s.x / M, s.e / M
        out.append(Q(x, e + U * (np.abs(x) + e) + ETA))
    return out


def bar_filter_M(v, R, X):
    """The filter's output w_i (R~_i y).  v: q_powers(E); R (S, F, M M) float32; X (M, F, T).
    -> (bar_re, bar_im (S, M, F, T), guard (F, T), value (S, M, F, T) complex128 as this evaluation has it).
    Guard: |d_k| > 2 |delta d_k| for every pivot (and a finite, positive sum of the powers)."""
    S = len(v)
    R = np.asarray(R, np.float32).astype(np.float64)
    X = np.asarray(X).astype(np.complex64)
    M = X.shape[0]
    MM = M * M
    r = [[Pair(Q(R[j, :, g][:, None])) for g in range(MM)] for j in range(S)]
    total = sum(q.x for q in v)
    live = np.isfinite(total) & (total > 0)
    e = np.where(live, np.frexp(np.where(live, total, 1.0))[1], 0)
    down = np.ldexp(1.0, -e)
    w = [Pair(_pow2(q, down)) for q in v]
    guards = [live]

    def recip(d):
        inv, ok = _inv(d.q)
        guards.append(ok)
        return Pair(inv)

    with np.errstate(invalid='ignore', over='ignore'):
        sg = []
        for g in range(MM):
            acc = w[0] * r[0][g]
            for j in range(1, S):
                acc = acc + w[j] * r[j][g]
            sg.append(acc)
        xr, xi = [Pair(Q(X[c].real)) for c in range(M)], [Pair(Q(X[c].imag)) for c in range(M)]
        yr, yi, _ = AS.ldl_solve(sg, xr, xi, M, recip=recip)
        shape = (S, M) + live.shape
        bar_re, bar_im, value = np.zeros(shape), np.zeros(shape), np.zeros(shape, np.complex128)
        for i in range(S):
            for a in range(M):
                ur, ui = AS.apply_row(r[i], a, yr, yi, M)
                o_re, o_im = (w[i] * ur).q, (w[i] * ui).q
                bar_re[i, a], bar_im[i, a] = SLACK * o_re.e, SLACK * o_im.e
                value[i, a] = o_re.x + 1j * o_im.x
    ok = guards[0]
    for g in guards[1:]:
        ok = ok & g
    return bar_re, bar_im, ok, value


def normwise_filter(E, R, X, out):
    """A second, normwise bar that needs no guard on the pivots: per (target, bin, frame) the distance of ``out`` from the float64
    filter over the M channels, and the residual of the sum of the targets, against bounds from the backward error of the solve.
    -> (share of the bar (S, F, T), share of the residual bar (F, T), checked (F, T): live frames with eta < 1/2).

    With u = 2^-24, u_c = 2 sqrt(2) u for a complex product and its sum (two rounded products, one rounded sum), Sigma = Sigma_w
    in float64 from the float32 R~ and the exact powers, kappa = ||Sigma||_2 / lambda_min(Sigma), y = Sigma^-1 X:
      forming Sigma_w  every component is sum_j w_j r_jg with w_j carrying the 2 M + 2 roundings of a power and the sum S more:
                       |dSigma| <= (2 M + S + 3) u sum_j w_j |R~_j| componentwise; || |R~_j| ||_F <= tr R~_j and
                       sum_j w_j tr R~_j = tr Sigma <= M ||Sigma||_2, so ||dSigma||_2 <= (2 M + S + 3) M u ||Sigma||_2
      the solve        LDL^H of a positive definite matrix and the two substitutions are backward stable as Cholesky is
                       (Higham, Accuracy and Stability, theorems 10.3 and 10.4: |dA| <= gamma_{3n+1} |R^T| |R|, || |R^T| |R| ||_2 <=
                       n ||A||_2; |L| |D| |L^H| = |R^H| |R|); this order has one more rounding per entry (l d_m, and the reciprocal
                       in place of a quotient): ||dSigma||_2 <= M (3 M + 4) u_c ||Sigma||_2
      so (Sigma + dSigma) y^ = X with ||dSigma||_2 <= rho ||Sigma||_2, rho = ((2 M + S + 3) M + (3 M + 4) M 2 sqrt 2) u, and with
      eta = kappa rho < 1/2:  ||y^ - y|| <= eta / (1 - eta) ||y||,  ||y^|| <= ||y|| / (1 - eta)
      the outputs      w_i R~_i y^: M complex products and M - 1 sums a row, the product with w_i and w_i's own 2 M + 2 roundings:
                       ||o^_i - o_i|| <= w_i ||R~_i||_2 ||y|| (eta + c_o) / (1 - eta),  c_o = (M + 1) sqrt(M) u_c + (2 M + 3) u
                       (a row's componentwise bound against | R~_i | | y^ | costs the sqrt(M) in norm)
      the residual     sum_i o^_i - X = -dSigma y^ + the outputs' roundings: no factor kappa:
                       <= (rho ||Sigma||_2 + c_o sum_i w_i ||R~_i||_2) ||y|| / (1 - eta)
    Everything on the right is evaluated in float64 from the inputs; SLACK covers that evaluation."""
    E, X, out = np.asarray(E), np.asarray(X).astype(np.complex64).astype(np.complex128), np.asarray(out).astype(np.complex128)
    S, M = E.shape[:2]
    ref = AS.spatial_filter(E, X, np.float64, R=R)
    H = AS.hermitian(np.asarray(R, np.float32).astype(np.float64), M)                 # (S, F, M, M)
    with np.errstate(all='ignore'):
        w, vs = AS._scaled(AS.powers(E, np.float64))
        live = np.isfinite(vs) & (vs > 0) & np.isfinite(X).all(axis=0)
        sigma = sum(w[j][:, :, None, None] * H[j][:, None] for j in range(S))
        sigma = np.where(live[:, :, None, None] & np.isfinite(sigma).all(axis=(-1, -2), keepdims=True), sigma, np.eye(M))
        ev = np.linalg.eigvalsh(sigma)
        lo, hi = ev[..., 0], ev[..., -1]
        rho = ((2 * M + S + 3) * M + (3 * M + 4) * M * 2 * np.sqrt(2.0)) * U
        c_o = (M + 1) * np.sqrt(M) * 2 * np.sqrt(2.0) * U + (2 * M + 3) * U
        eta = np.where(lo > 0, hi / np.where(lo > 0, lo, 1.0) * rho, np.inf)
        checked = live & (eta < 0.5)
        eta = np.where(checked, eta, 0.0)
        ynorm = np.linalg.norm(np.linalg.solve(sigma, np.transpose(np.where(live[None], X, 0), (1, 2, 0))[..., None])[..., 0], axis=-1)
        rnorm = np.linalg.eigvalsh(H)[..., -1]                                         # (S, F)
        wr = w * rnorm[:, :, None]
        bar = SLACK * wr * ynorm[None] * (eta + c_o)[None] / (1 - eta)[None] + 1e-300
        share = np.where(checked[None], np.linalg.norm(out - ref, axis=1) / bar, 0.0)
        rbar = SLACK * (rho * hi + c_o * wr.sum(axis=0)) * ynorm / (1 - eta) + 1e-300
        rshare = np.where(checked, np.linalg.norm(out.sum(axis=0) - X, axis=0) / rbar, 0.0)
    share, rshare = np.where(np.isnan(share), np.inf, share), np.where(np.isnan(rshare), np.inf, rshare)
    return share, rshare, checked, live


# ---- 3. the cells and their check ----------------------------------------------------------------------------------------------------

# (M, S, F, T, batch): position of the cell's own file, nsig_pitch (None: S M rounded up to even), how the file is built, its seed
CELLS = {
    (3, 2, 17, 2, 1):    dict(pos=0, pitch=None, args={}, seed=11),
    (5, 1, 4, 1, 1):     dict(pos=0, pitch=None, args={}, seed=12),
    (4, 3, 33, 129, 3):  dict(pos=1, pitch=None, args={}, seed=13),
    (6, 4, 40, 257, 1):  dict(pos=0, pitch=None, args=dict(zero_frame=130, tiny_frame=11), seed=14),
    (7, 5, 17, 127, 1):  dict(pos=0, pitch=None, args=dict(weak=(3, 80)), seed=15),
    (8, 8, 17, 130, 2):  dict(pos=0, pitch=64, args={}, seed=16),
    (3, 3, 33, 128, 1):  dict(pos=0, pitch=10, args=dict(absent=(0, 7)), seed=17),
}


def cell_files(cell):
    """The `batch` problems of a cell (the cell's own at ``pos``, uniform files of the same shape around it)."""
    M, S, F, T, B = cell
    c = CELLS[cell]
    return [structured(M, F, T, S, c['seed'], **c['args']) if b == c['pos'] else uniform(M, F, T, S, 100 * c['seed'] + b) for b in range(B)]


def _compare(failures, what, got, ref, bar, ok):
    """One real array against its float64 reference, element by element, by the rules of spatial_checks._compare except that the
    elements behind a failed guard are counted, not failed -> (the largest share of a bar, non-zero finite elements, those behind a
    failed guard)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.broadcast_to(ok, ref.shape)
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        failures.append('%s: NaN where the reference has none, or the reverse' % what)
    zero = ref == 0
    if not (got[zero] == 0).all():
        failures.append('%s: %d exact zeros of the reference are not zero' % (what, int((got[zero] != 0).sum())))
    rest = np.isfinite(ref) & ~zero
    m = rest & ok
    worst = 0.0
    if m.any():
        with np.errstate(invalid='ignore', divide='ignore'):
            share = np.where(m & (got != ref), np.abs(got - ref) / np.where(m, bar, 1.0), 0.0)
        share = np.where(np.isnan(share), np.inf, share)
        worst = float(share.max())
        if worst > 1.0:
            at = np.unravel_index(int(share.argmax()), share.shape)
            failures.append('%s: %.3g of the bar at %s (got %.9g, reference %.9g, bar %.3g); %d elements over' %
                            (what, worst, at, got[at], ref[at], bar[at], int((share > 1.0).sum())))
    return worst, int(rest.sum()), int((rest & ~ok).sum())


def check_cell(E, X, cov, out, what=''):
    """E (S, M, F, T) complex64 the ratio estimates and X (M, F, T) as the producer held them; cov (S, F, M M) float32 and out
    (S, M, F, T) complex64 what it made of them.  -> (failures under the bars, stages that are not the float32 restatement's bits, the
    largest share of a bar per check, (non-zero finite elements, those behind a failed pivot guard, those with no float64 check at
    all: behind a failed guard AND in a frame whose eta is not below 1/2))."""
    fail, bits, share = [], [], {}
    S, M = E.shape[:2]
    # the covariance launch: within one float32 ulp of the ascending-order sums, and bit for bit the device-order restatement
    asc = AS.covariances(E).astype(np.float64)
    share['covariance launch (ulp)'] = _compare(fail, '%s covariance launch' % what, cov, asc,
                                                np.spacing(np.abs(asc).astype(np.float32)).astype(np.float64) + 2.0 ** -40, np.ones((), bool))[0]
    model = AS.covariances(E, frame_sum=SC.device_sum)
    if not SC._bits(np.asarray(cov), model):
        bits.append('%s covariance launch: %d entries differ' % (what, int((np.asarray(cov) != model).sum())))
    # the filter on the producer's own covariances
    ref = AS.spatial_filter(E, X, np.float64, R=cov)
    bar_re, bar_im, ok, value = bar_filter_M(q_powers(E), cov, X)
    s_re, n_re, g_re = _compare(fail, '%s filter (re)' % what, out.real, ref.real, bar_re, ok[None, None])
    s_im, n_im, g_im = _compare(fail, '%s filter (im)' % what, out.imag, ref.imag, bar_im, ok[None, None])
    share['filter'] = max(s_re, s_im)
    counted, behind = n_re + n_im, g_re + g_im              # (the caller holds the count against GUARD_CAP, over the files of its cell)
    model = AS.spatial_filter(E, X, np.float32, R=cov)
    if not SC._bits(np.asarray(out), model):
        bits.append('%s filter: %d elements differ' % (what, int((np.asarray(out) != model).sum())))
    # sum_i w_i R~_i y = Sigma_w y = X: the targets add up to the mixture within the sum of their bars; one target returns it
    o = np.asarray(out).astype(np.complex128)
    Xc = np.asarray(X).astype(np.complex128)
    livef = (np.abs(o).sum(axis=0) != 0).any(axis=0)
    total = np.where(livef[None], o.sum(axis=0), Xc)
    f = []
    s = max(_compare(f, '%s sum of the targets (re)' % what, total.real, Xc.real, bar_re.sum(axis=0) + 1e-300, (ok | ~livef)[None])[0],
            _compare(f, '%s sum of the targets (im)' % what, total.imag, Xc.imag, bar_im.sum(axis=0) + 1e-300, (ok | ~livef)[None])[0])
    fail.extend(x for x in f if 'of the bar' in x)
    share['sum of the targets'] = s
    # the normwise bar and the residual: every live frame whose eta is below 1/2, whatever the pivots' guards say
    nshare, rshare, checked, live = normwise_filter(E, cov, X, out)
    share['normwise'], share['residual'] = float(nshare.max()), float(rshare.max())
    for name, sh in (('normwise bar', nshare), ('residual of the sum of the targets', rshare)):
        if sh.max() > 1.0:
            fail.append('%s %s: %.3g of the bar at %s; %d over' % (what, name, sh.max(), np.unravel_index(int(sh.argmax()), sh.shape),
                                                                  int((sh > 1.0).sum())))
    nonzero = np.isfinite(ref) & (ref != 0)
    unchecked = int((nonzero & ~(ok | checked)[None, None]).sum()) * 2          # (re and im, as `counted` counts)
    return fail, bits, share, (counted, behind, unchecked)
