"""Comparison rules of the real-time block call's stage tests (tests/test_gpu_rt_stages.py), in plain NumPy so that the CPU suite can show
they are sound and sensitive (tests/test_rt_checks.py) without torch or a device.  gccnmf_rt_process_block_ll (csrc/rt.hip) returns every
intermediate of a call, so every rule below is evaluated from the DEVICE'S OWN inputs to that stage -- no error is carried from one stage
into the next -- against float64, per element, with a worst-case bar derived from the arithmetic (never measured on the code under test).
`check_call` applies all nine to one call; the GPU suite feeds it the device's buffers, the CPU suite the float32 restatement `model32`.

  1 shift       in_ring = concat(in_ring[:, B:], block_in) bit for bit; every out_ring position no frame of the call covers = the shifted
                old value (0 in the last block) bit for bit
  2 analysis    X = rfft(w x), not conjugated.  Radix-2 windows: fft_checks.stft_bar.  Direct-sum windows: a float32 sum of N products
                against the float32 table the kernel read: gcc_checks.check_gemm_like, Kd = N
  3 coherence   fft_checks.check_coherence from the device's X where neither X is exactly 0; both parts NaN where one is (0 / 0, the
                reference's convention on this path)
  4 scores      G[tau,k,t] = sum_f (C.re cos + C.im sin) W in float64 from the device's C, b = gemm_bound(sum_f (|C.re||cos| + |C.im||sin|)
                |W|, F).  EVERY cell: 0 <= dev < D and G[dev] >= max_tau G - (b[dev] + b[argmax]); a frame with a NaN bin gives 0; among
                bitwise identical steering columns the device reports the first.  `decided_share` guards against vacuity
  5 mask        boxcar exact; window function exp(-x) / (1 + nf) + nf, x = (dist / eps)^beta, within RT_EXP_U u (1 + x) e^-x / (1 + nf)
                + 2 u |m|; rows K .. Kp-1 untouched.  Multi-target: one-hot, the target with the largest float64 score (allowance of rule 4)
  6 tf mask     sum_k W HMask / sum_k W from the device's HMask, k < K: (gemm_bound(num) + |m| gemm_bound(den)) / den, Kd = K;
                Y = float32(tfMask) * X bit for bit; multi-target: the N masks add up to 1 within the sum of their bars
  7 inference   Rv = |X| / (W h), Hcoef = h (W^T Rv) / colsumW from the device's own Rv and the PREVIOUS update's h (ones, or the Hcoef of
                the run with one update fewer: the call is deterministic); tfMask [2][F][Tc] from the device's Hcoef and HMask; a channel
                that is silent in a frame (|X| = 0 in every bin) has Rv = Hcoef = tfMask = Y = 0 exactly, not 0 / 0
  8 synthesis   float64 inverse of the device's Y (X with the separation off): fft_checks.frames_bar / the GEMM bound with Kd = N, plus
                Tc u |running sum| for the overlap-add; block_out = its out_ring slice bit for bit; frames mode: the frames themselves
  9 localise    gccphat = float64 nanmean over the non-NaN terms of the device's C (gemm_bound, Kd = F), NaN where every term is; written
                hist columns = gccphat, the others untouched, hist_pos = (pos0 + Tc) % Lh; the target = window_mean_f32 of the device's
                hist through numpy.argmax / pick_peaks, exactly; everything else in the target row untouched

RT_EXP_U is the one ASSUMED constant (like fft_checks.HYPOT_U): no statement of the accuracy of expf and powf on this target was found in
the documentation installed with the toolchain.  The unit is u (1 + x) e^-x / (1 + nf): a relative error on expf's result e^-x plus an
absolute error on its argument x (powf, the float32 division dist / eps and subtraction i - target in front of it).  The worst error seen
on the MI355X over every window-function cell of the GPU suite was 2.17 of these units (LABBOOK R15); the constant is twice that rounded
up, the factor 2 being margin because the argument set is small (a few hundred distinct (dist, eps, beta) triples).

Numbers the kernel rounds that the float64 restatements do not restate (the window product w x, the product w h of the inference mask,
dist / eps ...) are single roundings of a term; gemm_bound's Kd + 4 and RT_EXP_U hold them.
"""
import numpy as np

import fft_checks as K
import gcc_checks as G
from rt_multi_restatement import window_mean_f32, pick_peaks, nanargmax_first
import angular_nl_restatement as NL

U32 = K.U32
RT_EXP_U = 5.0          # ASSUMPTION (see above): expf(-powf(.)) within 5 units; measured 2.17
SENTINEL_I = -77        # argmaxTDOA before the call
MAX_TAU = 8.0           # the TDOA grid spans [-MAX_TAU, 0.8 MAX_TAU] samples (asymmetric: a delay of 0 has one nearest grid point)
DELAYS = (-3, 1, 4)     # samples, one per source
TIE_PAIRS = ((3, 7), (3, 36), (5, 70))      # duplicate steering columns (a, b): lane halves, the two tiles of a pass, two passes


def round_up(n, m):
    return -(-n // m) * m


class Cell(object):
    """One call's configuration.  S > 0: bank of S streams (stream 1 separation off, stream 2 localisation off); NT > 0: multi-target
    layout of NT targets; alpha > 0: GCC-NONLIN through the 8-word row (bit 24)."""

    def __init__(self, name, N, hop, B, K_, D, Lh=8, L=None, mode=2, od=2, frames=False, nH=0, S=0, NT=0, alpha=0.0, sep=1, loc=1,
                 ties=False, zero_frame=None, silent_right=False, nan_bins=None, hist_nan=False, row=(None, 5.0, 2.0, 0.0), pos0=None,
                 decided=True):
        self.name, self.N, self.hop, self.B, self.K, self.D, self.Lh, self.L = name, N, hop, B, K_, D, Lh, L
        self.mode, self.od, self.frames, self.nH, self.S, self.NT, self.alpha, self.sep, self.loc = mode, od, frames, nH, S, NT, alpha, sep, loc
        self.ties, self.zero_frame, self.silent_right, self.nan_bins, self.hist_nan, self.row = ties, zero_frame, silent_right, nan_bins, hist_nan, row
        self.decided = decided
        assert B % hop == 0 and N % 2 == 0
        self.Tc, self.F, self.Kp, self.Dp = B // hop, N // 2 + 1, round_up(K_, 64), round_up(D, 32)
        self.L = min(Lh, self.Tc + 2) if L is None else L
        self.pow2 = N >= 64 and N & (N - 1) == 0
        self.ring = self.Tc * N if frames else 8 * B
        self.start0 = 0 if frames else self.ring - N - (self.Tc - 1) * hop
        self.step = N if frames else hop
        self.bank, self.multi = S > 0, NT > 0
        self.nS, self.nM = max(S, 1), max(NT, 1)
        self.rowlen = 16 if self.multi else 8 if (self.bank or alpha > 0) else 4
        self.pos0 = (Lh - 2) if pos0 is None else pos0
        if self.multi:
            self.mode = 1
        assert self.start0 >= 0 and self.L <= Lh and not (self.bank and frames)

    def bits(self):
        b = 1 if self.frames else 0
        if self.bank:
            b |= 8 | ((self.S - 1) << 8)
        if self.multi:
            b |= (1 << 20) | ((self.NT - 1) << 21)
        if self.alpha > 0 and not (self.bank or self.multi):
            b |= 1 << 24
        return b

    def with_updates(self, nH):
        c = Cell.__new__(Cell)
        c.__dict__.update(self.__dict__)
        c.nH = nH
        return c

    def starts(self):
        return [self.start0 + t * self.step for t in range(self.Tc)]

    def covered(self):
        m = np.zeros(self.ring, bool)
        for st in self.starts():
            m[st:st + self.N] = True
        return m

    def targets(self):
        """Multi-target rows: in both lane halves of the score kernel (row tau lies in half (tau >> 2) & 1), spread over the grid."""
        if self.NT == 1:
            return np.array([(self.D // 2) | 4])
        return np.round(np.linspace(2, self.D - 3, self.NT)).astype(int)

    def __repr__(self):
        return self.name


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def dft_table(N):
    ang = 2.0 * np.pi * np.arange(N, dtype=np.float64) / N
    return np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32))


def taus(c):
    tmax = min(MAX_TAU, 0.225 * c.N)                          # N = 4: the scores have period 2 in tau; stay inside one period
    return np.linspace(-tmax, 0.8 * tmax, c.D), tmax


def make_tables(c):
    """W [F][Kp] (columns K.. finite, near 1e3: nothing may read them), cos / sin [F][Dp] of 2 pi f tau / N (columns D.. hold twice the
    column nearest the first source's delay: an admitted padded row would win), windows, transform table, colsumW."""
    rng = np.random.RandomState(c.N * 131 + c.K * 7 + c.D)
    F, N = c.F, c.N
    f = np.arange(F)
    band = lambda i: ((f * 3) // F == i).astype(np.float64)
    W = (rng.rand(F, c.Kp) + 0.02)
    for k in range(c.K):
        W[:, k] *= 1 + 4 * band(k % 3)
    # the Nyquist row and the last row of the first score wave's band weigh 8 times the others: a sum that drops one of them moves
    W[F - 1, :c.K] *= 8
    W[min(((F + 15) // 16) * 2, F) - 1, :c.K] *= 8
    W[:, :c.K] /= np.linalg.norm(W[:, :c.K], axis=0)
    W[:, c.K:] = 1e3 * (1 + rng.rand(F, c.Kp - c.K))
    W = W.astype(np.float32)
    tau, tmax = taus(c)
    ang = 2.0 * np.pi * np.outer(f / float(N), tau)
    cosT, sinT = np.zeros((F, c.Dp), np.float32), np.zeros((F, c.Dp), np.float32)
    cosT[:, :c.D], sinT[:, :c.D] = np.cos(ang), np.sin(ang)
    near = [int(np.argmin(np.abs(tau - d * tmax / MAX_TAU))) for d in DELAYS]
    if c.ties:                                                 # duplicate columns, scaled so that they win for many atoms
        src = {3: near[0], 5: near[1]}
        assert not set(src.values()) & {3, 5, 7, 36, 70}
        for T_ in (cosT, sinT):
            for a in src:
                T_[:, a] = np.float32(1.25) * T_[:, src[a]]
            for a, b in TIE_PAIRS:
                if b < c.D:
                    T_[:, b] = T_[:, a]
    for T_ in (cosT, sinT):
        T_[:, c.D:] = 2 * T_[:, near[0]:near[0] + 1]
    if c.nan_bins is not None:
        window = np.ones(N, np.float32)
    else:
        window = np.sqrt(np.hamming(N)).astype(np.float32)
    swindow = (np.sqrt(np.hanning(N) + 0.05) * 0.8).astype(np.float32)
    if c.pow2:
        twiddle = np.ascontiguousarray(K.twiddles(N)).view(np.float32).reshape(-1, 2)
    else:
        twiddle = dft_table(N)
    colsum = np.zeros(c.Kp, np.float32)
    colsum[:c.K] = W[:, :c.K].sum(axis=0, dtype=np.float32)
    colsum[c.K:] = np.nan
    return dict(W=W, cosT=cosT, sinT=sinT, window=window, swindow=swindow, twiddle=twiddle, colsumW=colsum)


def stream_signal(c, seed):
    """(2, ring + B) float32: three band-shaped noise sources, the right channel delayed by DELAYS (scaled to the cell's grid), amplitude
    stepping over powers of two per hop."""
    n = c.ring + c.B + 64
    rng = np.random.RandomState(seed)
    tmax = taus(c)[1]
    xL, xR = np.zeros(n), np.zeros(n)
    nf = n // 2 + 1
    for i, d in enumerate(DELAYS):
        spec = np.fft.rfft(rng.standard_normal(n))
        mask = np.where((np.arange(nf) * 3) // nf == i, 1.0, 0.05)
        s = np.fft.irfft(spec * mask, n)
        di = int(round(d * tmax / MAX_TAU))
        xL += s
        xR += np.roll(s, di)
    x = np.stack([xL, xR])[:, 32:32 + c.ring + c.B]
    amp = np.repeat(K.amplitudes(-(-x.shape[1] // c.hop)), c.hop)[:x.shape[1]]
    return (x * amp).astype(np.float32)


def make_inputs(c):
    """Everything one call reads, host side; per-stream buffers carry a leading S axis (1 outside the bank)."""
    I = make_tables(c)
    S, nM = c.nS, c.nM
    rng = np.random.RandomState(len(c.name) * 1009 + c.N)
    in_ring, block_in = np.zeros((S, 2, c.ring), np.float32), np.zeros((S, 2, c.B), np.float32)
    for s in range(S):
        x = stream_signal(c, 17 * c.N + s)
        if c.frames:
            after = np.zeros((2, c.ring), np.float32)
            for t in range(c.Tc):
                after[:, t * c.N:(t + 1) * c.N] = x[:, t * c.hop:t * c.hop + c.N]
        else:
            after = x[:, c.B:c.B + c.ring].copy()              # the input buffer as the frames will see it: after the shift
        if c.zero_frame is not None:
            st = c.starts()[c.zero_frame]
            after[:, st:st + c.N] = 0
        if c.silent_right:
            after[1] = 0
        if c.nan_bins is not None:                             # L = delta[n] + delta[n - N/2], R = L / 2: odd bins exactly zero
            st = c.starts()[c.nan_bins]
            after[:, st:st + c.N] = 0
            after[0, st], after[0, st + c.N // 2] = 1, 1
            after[1, st], after[1, st + c.N // 2] = 0.5, 0.5
        if c.frames:
            in_ring[s] = after
        else:
            in_ring[s] = np.concatenate([x[:, :c.B], after[:, :c.ring - c.B]], axis=1)
            block_in[s] = after[:, c.ring - c.B:]
    I['in_ring'], I['block_in'] = in_ring, block_in
    I['out_ring'] = (rng.standard_normal((S, nM, 2, c.ring)) * 0.25).astype(np.float32)
    hist = (rng.standard_normal((S, c.D, c.Lh)) * 0.1).astype(np.float32)
    if c.hist_nan:
        hist[:] = np.nan
    else:
        hist[:, 2, :] = np.nan                                 # a TDOA whose older columns are all NaN
        hist[:, ::5, c.pos0 - 1] = np.nan                      # NaN in the newest old column for some TDOAs
    I['hist'], I['hist_pos'] = hist, np.full(S, c.pos0, np.int32)
    target = np.zeros((S, c.rowlen), np.float32)
    target[:, 1:4] = c.row[1:]
    tau, tmax = taus(c)                                        # default target: 0.4 above column 3 (a tie column) / the second source's
    target[:, 0] = c.row[0] if c.row[0] is not None else 0.4 + (3 if c.ties else int(np.argmin(np.abs(tau - DELAYS[1] * tmax / MAX_TAU))))
    if c.rowlen >= 8:
        target[:, 4:8] = (1, 1, c.alpha, 0)
    if c.bank and S >= 3:
        target[1, 4], target[2, 5] = 0, 0
        target[1, 0], target[2, 0] = 3, c.D - 4
    if c.multi:
        target[:, 8:] = -5                                     # unused target words: garbage
        target[:, 8:8 + c.NT] = c.targets()
    I['target'] = target
    return I


NAN_OUT = ('block_out', 'X', 'Y', 'C', 'HMask', 'tfMask', 'gccphat', 'Hcoef', 'Rv')


def output_shapes(c):
    S, nM, F, Tc = c.nS, c.nM, c.F, c.Tc
    return dict(block_out=(S, nM, 2, c.B), X=(S, 2, F, Tc, 2), Y=(S, nM, 2, F, Tc, 2), C=(S, F, Tc, 2), HMask=(S, nM, c.Kp, Tc),
                tfMask=(S, nM, 2, F, Tc), gccphat=(S, c.D, Tc), Hcoef=(S, c.Kp, 2 * Tc), Rv=(S, F, 2 * Tc), argmax=(S, c.Kp, Tc))


def cplx(a):
    a = np.ascontiguousarray(a, np.float32)
    return a.view(np.complex64)[..., 0]


# ---- float64 restatements -------------------------------------------------------------------------------------------------------------
def frames_of_ring(c, ring_in):
    idx = np.asarray(c.starts())[:, None] + np.arange(c.N)[None, :]
    return np.asarray(ring_in)[:, idx]                         # (2, Tc, N)


def analysis64(c, I, ring_in):
    """-> (X (2, F, Tc) complex128, bar (F, Tc) or None, absprod (2 parts: (2, F, Tc)) or None)"""
    if c.pow2:
        ref, sumabs = K.stft64(np.asarray(ring_in)[:, c.start0:], I['window'], c.N, c.step, c.Tc)
        return np.conj(ref), K.stft_bar(sumabs, c.N), None
    w = I['window'].astype(np.float64)
    xw = w * frames_of_ring(c, ring_in).astype(np.float64)
    tab = I['twiddle'].astype(np.float64)
    idx = (np.arange(c.F)[:, None] * np.arange(c.N)[None, :]) % c.N
    cm, sm = tab[idx, 0], tab[idx, 1]                          # (F, N)
    X = np.einsum('ctn,fn->cft', xw, cm) - 1j * np.einsum('ctn,fn->cft', xw, sm)
    a = np.abs(xw)
    return X, None, (np.einsum('ctn,fn->cft', a, np.abs(cm)), np.einsum('ctn,fn->cft', a, np.abs(sm)))


def first_identical(cosT, sinT, D):
    """first_of[tau] = the smallest tau' whose float32 steering column has the same bits."""
    key = np.concatenate([cosT[:, :D], sinT[:, :D]]).view(np.uint32).T
    seen, out = {}, np.zeros(D, np.int64)
    for t in range(D):
        out[t] = seen.setdefault(key[t].tobytes(), t)
    return out


def scores64(c, I, Cd):
    """float64 scores from a coherence image (F, Tc) complex: (G (D, K, Tc), bound (D, K, Tc), NaN frames (Tc,))."""
    cre, cim = np.real(Cd).astype(np.float64), np.imag(Cd).astype(np.float64)
    nanf = np.isnan(cre).any(axis=0) | np.isnan(cim).any(axis=0)
    cre, cim = np.where(np.isnan(cre), 0, cre), np.where(np.isnan(cim), 0, cim)
    co, si = I['cosT'][:, :c.D].astype(np.float64), I['sinT'][:, :c.D].astype(np.float64)
    Wk = I['W'][:, :c.K].astype(np.float64)
    A = cre[:, None, :] * co[:, :, None] + cim[:, None, :] * si[:, :, None]
    Ab = np.abs(cre)[:, None, :] * np.abs(co)[:, :, None] + np.abs(cim)[:, None, :] * np.abs(si)[:, :, None]
    return np.einsum('fdt,fk->dkt', A, Wk), G.gemm_bound(np.einsum('fdt,fk->dkt', Ab, np.abs(Wk)), c.F), nanf


def decided_share(Gs, bnd, first_of, nanf):
    """Share of the (k, t) cells of live frames whose float64 leader beats the best DIFFERENT steering column (bitwise duplicates are one
    column) by more than the two bounds -- so that rule 4 pins the device's index there.  1.0 when no frame is live."""
    live = ~nanf
    if not live.any():
        return 1.0
    uniq = np.flatnonzero(first_of == np.arange(len(first_of)))
    g, b = Gs[uniq][:, :, live], bnd[uniq][:, :, live]
    order = np.argsort(g, axis=0)
    top, second = order[-1][None], order[-2][None]
    lead = np.take_along_axis(g, top, 0) - np.take_along_axis(g, second, 0)
    allow = np.take_along_axis(b, top, 0) + np.take_along_axis(b, second, 0)
    return float(np.mean(lead > allow))


def decided64(c, I):
    """The decided share of every stream from float64 alone: float64 analysis of the inputs, float64 coherence, float64 scores."""
    out = []
    for s in range(c.nS):
        ring = I['in_ring'][s] if c.frames else np.concatenate([I['in_ring'][s][:, c.B:], I['block_in'][s]], axis=1)
        Gs, bnd, nanf = scores64(c, I, coherence64(analysis64(c, I, ring)[0]))
        out.append(decided_share(Gs, bnd, first_identical(I['cosT'], I['sinT'], c.D), nanf))
    return min(out)


def coherence64(X):
    X = np.asarray(X, np.complex128)
    with np.errstate(invalid='ignore', divide='ignore'):
        return X[0] * np.conj(X[1]) / np.abs(X[0]) / np.abs(X[1])


def synthesis64(c, I, S2):
    """S2 (2, F, Tc) complex64 -> (frames (2, Tc, N) float64, bar (Tc, N))."""
    N, H = c.N, c.N // 2
    sw = I['swindow']
    if c.pow2:
        fr, sumabs = K.istft_frames64(np.conj(S2[0]), np.conj(S2[1]), sw, N)
        return fr, K.frames_bar(sumabs, sw, N)
    return synth_direct(c, I, S2, np.float64)


def synth_direct(c, I, S2, dtype):
    """The direct-sum inverse in `dtype` (float64: the reference and its bound; float32: the CPU suite's restatement)."""
    N, H = c.N, c.N // 2
    w = I['swindow'].astype(dtype)
    tab = I['twiddle'].astype(dtype)
    re, im = np.real(S2).astype(dtype), np.imag(S2).astype(dtype)
    idx = (np.arange(1, H)[:, None] * np.arange(N)[None, :]) % N             # (H-1, N)
    cm, sm = tab[idx, 0], tab[idx, 1]
    sign = np.where(np.arange(N) % 2, -1, 1).astype(dtype)
    acc = np.einsum('cft,fn->ctn', re[:, 1:H], cm) - np.einsum('cft,fn->ctn', im[:, 1:H], sm)
    y0, yH = re[:, 0, :, None], re[:, H, :, None]
    fr = w * ((y0 + sign * yH + dtype(2) * acc) * dtype(1.0 / N))
    if dtype is not np.float64:
        return fr, None
    absacc = np.einsum('cft,fn->ctn', np.abs(re[:, 1:H]), np.abs(cm)) + np.einsum('cft,fn->ctn', np.abs(im[:, 1:H]), np.abs(sm))
    absprod = (np.abs(y0) + np.abs(yH) + 2 * absacc).max(axis=0)
    return fr, G.gemm_bound(absprod, N) * np.abs(w) / N


# ---- the rules ------------------------------------------------------------------------------------------------------------------------
def _share(got, ref, bar):
    err = np.abs(np.asarray(got).astype(np.complex128 if np.iscomplexobj(got) or np.iscomplexobj(ref) else np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        sh = np.where(err == 0, 0.0, err / bar)
    return float(sh.max()) if sh.size else 0.0


def gemm_rule(got, ref, absprod, Kd, what):
    G.check_gemm_like(got, ref, absprod, Kd, what=what)
    return _share(got, ref, G.gemm_bound(absprod, Kd))


def untouched(a, what, sentinel=None):
    a = np.asarray(a)
    bad = ~np.isnan(a) if sentinel is None else a != sentinel
    assert not bad.any(), '%s: %d elements written that the call must leave alone (first at %s)' % (what, int(bad.sum()), K._where(bad))


def _note(sh, key, v):
    sh[key] = max(sh.get(key, 0.0), float(v))


def check_call(c, I, O, first=None):
    """All nine rules on one call.  I: make_inputs(c); O: the buffers after the call, shaped like I / output_shapes (X, Y, C as complex).
    `first`: the outputs of the same call with one coefficient update fewer (needed when c.nH > 1).  -> dict of the worst share per bar,
    'exp_units' (worst error of the window mask in RT_EXP_U's units) and 'decided' (smallest decided share of the streams)."""
    sh = {}
    for s in range(c.nS):
        Is = dict(I)
        Os = {}
        for k in ('in_ring', 'block_in', 'out_ring', 'hist', 'hist_pos', 'target'):
            Is[k] = I[k][s]
        for k, v in O.items():
            Os[k] = v[s]
        _check_stream(c, '%s stream %d' % (c.name, s), Is, Os, None if first is None else {k: v[s] for k, v in first.items()}, sh)
    return sh


def _check_stream(c, what, I, O, first, sh):
    F, Tc, N, Kk, D, B = c.F, c.Tc, c.N, c.K, c.D, c.B
    row = I['target']
    sep_on = bool(c.sep) and (not c.bank or row[4] != 0)
    loc_on = bool(c.loc) and (not c.bank or row[5] != 0)
    Wk = I['W'][:, :Kk].astype(np.float64)

    # 1 shift
    if c.frames:
        K.check_bits(O['in_ring'], I['in_ring'], what + ' in_ring (frames mode: input only)')
        shifted = None
    else:
        K.check_bits(O['in_ring'], np.concatenate([I['in_ring'][:, B:], I['block_in']], axis=1), what + ' in_ring after the shift')
        shifted = np.concatenate([I['out_ring'][..., B:], np.zeros(I['out_ring'].shape[:-1] + (B,), np.float32)], axis=-1)
        unc = ~c.covered()
        K.check_bits(O['out_ring'][..., unc], shifted[..., unc], what + ' out_ring outside the frames')
    ring_in = O['in_ring']

    # 2 analysis
    X = O['X']
    ref, bar, absprod = analysis64(c, I, ring_in)
    if c.pow2:
        for ch in range(2):
            _note(sh, 'X radix-2', K.check_bar(X[ch], ref[ch], bar, '%s X channel %d' % (what, ch)))
    else:
        for ch in range(2):
            _note(sh, 'X direct', gemm_rule(X[ch].real, ref[ch].real, absprod[0][ch], N, '%s X re channel %d' % (what, ch)))
            _note(sh, 'X direct', gemm_rule(X[ch].imag, ref[ch].imag, absprod[1][ch], N, '%s X im channel %d' % (what, ch)))

    # 3 coherence
    Cd = O['C']
    zero = (X[0] == 0) | (X[1] == 0)
    assert np.isnan(Cd.real[zero]).all() and np.isnan(Cd.imag[zero]).all(), what + ': C not NaN in both parts where an X is exactly 0'
    nz = ~zero
    if nz.any():
        _note(sh, 'C', K.check_coherence(Cd[nz], X[0][nz], X[1][nz], np.abs(X[0][nz].astype(np.complex128)), np.abs(X[1][nz].astype(np.complex128)), what + ' C'))
    if c.nan_bins is not None:
        t = c.nan_bins
        assert zero[1::2, t].all() and not zero[0::2, t].any(), what + ': the delta pair does not give exactly-zero odd bins'

    # 4 scores and arg-max, 5 coefficient mask
    HM, am = O['HMask'], O['argmax']
    untouched(HM[:, Kk:], what + ' HMask rows K..Kp-1')
    untouched(am[Kk:], what + ' argmaxTDOA rows K..Kp-1', SENTINEL_I)
    if not sep_on:
        untouched(HM, what + ' HMask (separation off)')
        untouched(am, what + ' argmaxTDOA (separation off)', SENTINEL_I)
        untouched(O['tfMask'], what + ' tfMask (separation off)')
        untouched(O['Y'].real, what + ' Y (separation off)')
        untouched(O['Hcoef'], what + ' Hcoef (separation off)')
        untouched(O['Rv'], what + ' Rv (separation off)')
    else:
        Gs, bnd, nanf = scores64(c, I, Cd)
        first_of = first_identical(I['cosT'], I['sinT'], D)
        dev = am[:Kk].astype(np.int64)
        bad = (dev < 0) | (dev >= D)
        assert not bad.any(), '%s argmaxTDOA: %d cells outside [0, D) (first at %s: %d)' % (what, int(bad.sum()), K._where(bad), dev[K._where(bad)])
        assert not dev[:, nanf].any(), what + ' argmaxTDOA: a frame with a NaN bin must give index 0'
        live = ~nanf
        gd, bd = np.take_along_axis(Gs, dev[None], 0)[0], np.take_along_axis(bnd, dev[None], 0)[0]
        top = Gs.argmax(axis=0)
        gm, bm = Gs.max(axis=0), np.take_along_axis(bnd, top[None], 0)[0]
        bad = (gd < gm - (bd + bm)) & live[None, :]
        assert not bad.any(), ('%s argmaxTDOA: %d cells whose score is below the float64 maximum by more than the two bounds (first at %s: device '
                               '%d, float64 %d, %.6e vs %.6e, allowance %.2e)' % (what, int(bad.sum()), K._where(bad), dev[K._where(bad)], top[K._where(bad)],
                                                                                 gd[K._where(bad)], gm[K._where(bad)], (bd + bm)[K._where(bad)]))
        bad = (first_of[dev] != dev) & live[None, :]
        assert not bad.any(), '%s argmaxTDOA: %d cells report a duplicate steering column instead of the first of its kind (first at %s: %d, first %d)' % (
            what, int(bad.sum()), K._where(bad), dev[K._where(bad)], first_of[dev[K._where(bad)]])
        if live.any():
            with np.errstate(invalid='ignore', divide='ignore'):
                _note(sh, 'argmax allowance', np.where(gm == gd, 0, (gm - gd) / (bd + bm))[:, live].max())
        sh['decided'] = min(sh.get('decided', 1.0), decided_share(Gs, bnd, first_of, nanf))
        if c.ties:
            sh['tie cells'] = sh.get('tie cells', 0) + int(np.sum((first_of[top] == top) & np.isin(top, [a for a, b in TIE_PAIRS if b < D]) & live[None, :]))

        if c.multi:
            tg = row[8:8 + c.NT].astype(np.int64)
            hm = HM[:, :Kk]
            G.check_written(hm, what + ' HMask')
            assert np.isin(hm, (0.0, 1.0)).all() and (hm.sum(axis=0) == 1).all(), what + ' HMask: not one-hot'
            pick = hm.argmax(axis=0)
            Gt, bt = Gs[tg], bnd[tg]
            best = nanargmax_first(np.where(nanf[None, None, :], np.nan, Gt), axis=0)
            assert not pick[:, nanf].any(), what + ' HMask: a frame with a NaN bin must go to target 0'
            gp, bp = np.take_along_axis(Gt, pick[None], 0)[0], np.take_along_axis(bt, pick[None], 0)[0]
            gb, bb = np.take_along_axis(Gt, best[None], 0)[0], np.take_along_axis(bt, best[None], 0)[0]
            bad = (gp < gb - (bp + bb)) & live[None, :]
            assert not bad.any(), '%s HMask: %d atoms given to a target whose score is below the best by more than the two bounds (first at %s)' % (
                what, int(bad.sum()), K._where(bad))
            sh['multi agree'] = min(sh.get('multi agree', 1.0), float(np.mean(pick == best)))
        else:
            tgt, eps, beta, nf = [np.float32(v) for v in row[:4]]
            dist32 = np.abs(dev.astype(np.float32) - tgt)
            if c.mode == 0:
                K.check_bits(HM[0, :Kk], (dist32 < eps).astype(np.float32), what + ' HMask (boxcar)')
            else:
                d, e, b_, n_ = np.abs(dev.astype(np.float64) - float(tgt)), float(eps), float(beta), float(nf)
                x = (d / e) ** b_
                m = np.exp(-x) / (1 + n_) + n_
                unit = U32 * (1 + x) * np.exp(-x) / (1 + n_)
                _note(sh, 'HMask window', K.check_bar(HM[0, :Kk], m, RT_EXP_U * unit + 2 * U32 * np.abs(m) + 2.0 ** -149, what + ' HMask (window function)'))
                ok = x < 80
                if ok.any():
                    over = np.maximum(np.abs(HM[0, :Kk].astype(np.float64) - m) - 2 * U32 * np.abs(m), 0)      # what RT_EXP_U has to hold
                    _note(sh, 'exp_units', (over[ok] / unit[ok]).max())

        # 6 time-frequency mask / 7 coefficient inference
        tf, Y = O['tfMask'], O['Y']
        den1 = Wk.sum(axis=1)
        if c.nH == 0:
            untouched(tf[:, 1], what + ' tfMask second plane (no coefficient inference)')
            untouched(O['Hcoef'], what + ' Hcoef (no coefficient inference)')
            untouched(O['Rv'], what + ' Rv (no coefficient inference)')
            total, tbar = 0.0, 0.0
            for i in range(c.nM):
                hmd = HM[i, :Kk].astype(np.float64)
                m = (Wk @ hmd) / den1[:, None]
                bar = (G.gemm_bound(np.abs(Wk) @ np.abs(hmd), Kk) + np.abs(m) * G.gemm_bound(np.abs(Wk).sum(axis=1), Kk)[:, None]) / np.abs(den1)[:, None]
                _note(sh, 'tfMask', K.check_bar(tf[i, 0], m, bar, '%s tfMask target %d' % (what, i)))
                total, tbar = total + tf[i, 0].astype(np.float64), tbar + bar
                for ch in range(2):
                    K.check_bits(Y[i, ch].real, tf[i, 0] * X[ch].real, '%s Y re target %d channel %d' % (what, i, ch))
                    K.check_bits(Y[i, ch].imag, tf[i, 0] * X[ch].imag, '%s Y im target %d channel %d' % (what, i, ch))
            if c.multi:
                _note(sh, 'sum of masks', K.check_bar(total, np.ones_like(total), tbar, what + ' sum of the N masks'))
        else:
            assert c.nH == 1 or first is not None
            absX = np.abs(X.astype(np.complex128))                                       # (2, F, Tc)
            v = np.transpose(absX, (1, 2, 0)).reshape(F, 2 * Tc)                          # col = 2 t + c
            # a channel silent in a frame (|X| = 0 in every bin) gets no coefficients: Rv, Hcoef, its mask and Y are exactly 0, not 0 / 0
            silent = (v == 0).all(axis=0)
            lv = ~silent
            hprev = np.ones((Kk, 2 * Tc)) if c.nH == 1 else first['Hcoef'][:Kk].astype(np.float64)
            with np.errstate(invalid='ignore', divide='ignore'):
                den = Wk @ hprev
                rv = v / den
                bar = rv * K.HYPOT_U * U32 + rv * G.gemm_bound(np.abs(Wk) @ np.abs(hprev), Kk) / np.abs(den)
            G.check_zero(O['Rv'][:, silent], what + ' Rv of a silent channel')
            _note(sh, 'Rv', K.check_bar(O['Rv'][:, lv], rv[:, lv], bar[:, lv], what + ' Rv'))
            rvd = O['Rv'].astype(np.float64)
            cs = I['colsumW'][:Kk].astype(np.float64)[:, None]
            h = hprev * (Wk.T @ rvd) / cs
            bar = G.gemm_bound(np.abs(Wk).T @ np.abs(rvd), F) * np.abs(hprev) / cs + 2 * U32 * np.abs(h)
            G.check_zero(O['Hcoef'][:Kk][:, silent], what + ' Hcoef of a silent channel')
            _note(sh, 'Hcoef', K.check_bar(O['Hcoef'][:Kk][:, lv], h[:, lv], bar[:, lv], what + ' Hcoef'))
            untouched(O['Hcoef'][Kk:], what + ' Hcoef rows K..Kp-1')
            hd = O['Hcoef'][:Kk].astype(np.float64).reshape(Kk, Tc, 2)
            for i in range(c.nM):
                hmd = HM[i, :Kk].astype(np.float64)
                for ch in range(2):
                    hc, lt = hd[:, :, ch], lv[ch::2]
                    with np.errstate(invalid='ignore', divide='ignore'):
                        dn = Wk @ hc
                        m = (Wk @ (hc * hmd)) / dn
                        bar = (G.gemm_bound(np.abs(Wk) @ np.abs(hc * hmd), Kk) + np.abs(m) * G.gemm_bound(np.abs(Wk) @ np.abs(hc), Kk)) / np.abs(dn)
                    G.check_zero(tf[i, ch][:, ~lt], '%s tfMask of a silent channel, target %d channel %d' % (what, i, ch))
                    _note(sh, 'tfMask inferred', K.check_bar(tf[i, ch][:, lt], m[:, lt], bar[:, lt], '%s tfMask target %d channel %d' % (what, i, ch)))
                    K.check_bits(Y[i, ch].real, tf[i, ch] * X[ch].real, '%s Y re target %d channel %d' % (what, i, ch))
                    K.check_bits(Y[i, ch].imag, tf[i, ch] * X[ch].imag, '%s Y im target %d channel %d' % (what, i, ch))

    # 8 synthesis
    h0 = c.ring - (c.od + 1) * B
    for i in range(c.nM):
        src = O['Y'][i] if sep_on else X
        fr, fbar = synthesis64(c, I, src)
        got = O['out_ring'][i]
        if c.frames:
            for ch in range(2):
                _note(sh, 'frames out', K.check_bar(got[ch].reshape(Tc, N), fr[ch], fbar, '%s frames out target %d channel %d' % (what, i, ch)))
            untouched(O['block_out'], what + ' block_out (frames mode)')
        else:
            acc, bar, pmax = shifted[i].astype(np.float64), np.zeros(c.ring), np.zeros((2, c.ring))
            for t, st in enumerate(c.starts()):
                acc[:, st:st + N] += fr[:, t]
                bar[st:st + N] += fbar[t]
                pmax = np.maximum(pmax, np.abs(acc))
            for ch in range(2):
                _note(sh, 'out_ring', K.check_bar(got[ch], acc[ch], bar + Tc * U32 * pmax[ch], '%s out_ring target %d channel %d' % (what, i, ch)))
            K.check_bits(O['block_out'][i], got[:, h0:h0 + B], '%s block_out target %d' % (what, i))

    # 9 localisation
    gp = O['gccphat']
    co, si = I['cosT'][:, :D], I['sinT'][:, :D]
    if c.alpha > 0:
        g64 = NL.gccphat_nl(Cd, co.astype(np.float64), si.astype(np.float64), c.alpha)
        g32 = NL.gccphat_nl(Cd, co, si, c.alpha, np.float32).astype(np.float64)
        bar = np.full(g64.shape, NL.BAR_FACTOR * np.nanmax(np.abs(g32 - g64)))
        key = 'gccphat NONLIN'
    else:
        cre, cim = Cd.real.astype(np.float64), Cd.imag.astype(np.float64)
        term = cre[:, None, :] * co.astype(np.float64)[:, :, None] + cim[:, None, :] * si.astype(np.float64)[:, :, None]
        ab = np.abs(cre)[:, None, :] * np.abs(co).astype(np.float64)[:, :, None] + np.abs(cim)[:, None, :] * np.abs(si).astype(np.float64)[:, :, None]
        cnt = (~np.isnan(term)).sum(axis=0)
        with np.errstate(invalid='ignore', divide='ignore'):
            g64 = np.where(cnt > 0, np.nansum(term, axis=0) / cnt, np.nan)
            bar = G.gemm_bound(np.nansum(ab, axis=0), F) / np.maximum(cnt, 1)
        key = 'gccphat'
    dead = np.isnan(g64)
    assert np.isnan(gp[dead]).all(), what + ' gccphat: not NaN where every term is NaN'
    if (~dead).any():
        _note(sh, key, K.check_bar(gp[~dead], g64[~dead], bar[~dead], what + ' gccphat'))
    pos0 = int(I['hist_pos'])
    want = I['hist'].copy()
    for t in range(Tc):
        want[:, (pos0 + t) % c.Lh] = gp[:, t]
    K.check_bits(O['hist'], want, what + ' hist')
    pos1 = (pos0 + Tc) % c.Lh
    assert int(O['hist_pos']) == pos1, '%s hist_pos %d, expected %d' % (what, int(O['hist_pos']), pos1)
    want = row.copy()
    if loc_on:
        m = window_mean_f32(O['hist'], pos1, c.L)
        if c.multi:
            want[8:8 + c.NT] = pick_peaks(m, c.NT, row[8:8 + c.NT])
        else:
            want[0] = np.float32(np.argmax(m))
    K.check_bits(O['target'], want, what + ' target row')


# ---- float32 restatement of the call (CPU suite): NumPy's summation orders, one float32 rounding per operation -----------------------------
def model32(c, I, bug=None, stale=0.5):
    """The call in float32 NumPy -> the output buffers (as the GPU suite downloads them).  `bug`: one of the mistakes of
    tests/test_rt_checks.py applied to it."""
    f32 = np.float32
    S, nM, F, Tc, N, Kk, D, B = c.nS, c.nM, c.F, c.Tc, c.N, c.K, c.D, c.B
    O = {}
    for k, shp in output_shapes(c).items():
        if k in ('X', 'Y', 'C'):
            O[k] = np.full(shp[:-1], np.nan + 1j * np.nan, np.complex64)
        elif k == 'argmax':
            O[k] = np.full(shp, SENTINEL_I, np.int32)
        else:
            O[k] = np.full(shp, np.nan, f32)
    O['in_ring'], O['out_ring'], O['hist'] = I['in_ring'].copy(), I['out_ring'].copy(), I['hist'].copy()
    O['hist_pos'], O['target'] = I['hist_pos'].copy(), I['target'].copy()
    W32, co, si = I['W'][:, :Kk], I['cosT'], I['sinT']
    w, sw = I['window'], I['swindow']
    for s in range(S):
        row = I['target'][s]
        sep_on = bool(c.sep) and (not c.bank or row[4] != 0)
        loc_on = bool(c.loc) and (not c.bank or row[5] != 0)
        if not c.frames:
            ring = np.concatenate([I['in_ring'][s][:, B:], I['block_in'][s]], axis=1)
            if bug == 'shift_off1':                            # the second chunk of the shift reads one sample further
                flat = np.concatenate([I['in_ring'][s].reshape(-1), np.zeros(1, f32)])
                ring = ring.copy().reshape(-1)
                i = np.arange(8192, 2 * c.ring)
                ok = (i % c.ring) + B + 1 < c.ring
                ring[i[ok]] = flat[i[ok] + B + 1]
                ring = ring.reshape(2, c.ring)
            O['in_ring'][s] = ring
            out = np.concatenate([I['out_ring'][s][..., B:], np.zeros((nM, 2, B), f32)], axis=-1)
        else:
            ring, out = I['in_ring'][s], np.full((nM, 2, c.ring), np.nan, f32)
        # analysis
        if c.pow2:
            X = np.conj(K.stft32(ring[:, c.start0:], w, N, c.step, Tc))
        else:
            xw = w * frames_of_ring(c, ring)
            idx = (np.arange(F)[:, None] * np.arange(N)[None, :]) % N
            cm, sm = I['twiddle'][idx, 0], I['twiddle'][idx, 1]
            X = (np.einsum('ctn,fn->cft', xw, cm) - 1j * np.einsum('ctn,fn->cft', xw, sm)).astype(np.complex64)
        O['X'][s] = X
        with np.errstate(invalid='ignore', divide='ignore'):
            aL, aR = np.abs(X[0]), np.abs(X[1])
            re = X[0].real * X[1].real + X[0].imag * X[1].imag
            im = X[0].imag * X[1].real - X[0].real * X[1].imag
            Cd = ((re / aL / aR) + 1j * (im / aL / aR)).astype(np.complex64)
        O['C'][s] = Cd
        src = np.repeat(X[None], nM, axis=0)
        if sep_on:
            A = Cd.real[:, None, :] * co[:, :, None] + Cd.imag[:, None, :] * si[:, :, None]       # (F, Dp, Tc) float32
            rows = np.arange(F)
            if bug == 'no_nyquist':
                rows = rows[:-1]
            if bug == 'wave_last_row':
                per = ((F + 15) // 16) * 2
                rows = np.delete(rows, per - 1)
            Gs = np.einsum('fdt,fk->dkt', A[rows], W32[rows]).astype(f32)
            Dn = c.Dp if bug == 'padded_row' else D
            with np.errstate(invalid='ignore'):
                Gv = np.where(np.isnan(Gs[:Dn]), -np.inf, Gs[:Dn])
            idx = np.argmax(Gv, axis=0)
            if bug == 'tie_larger':
                idx = Dn - 1 - np.argmax(Gv[::-1], axis=0)
            idx = np.where(np.isnan(Gs[:Dn]).all(axis=0), 0, idx).astype(np.int32)
            kw = Kk - 1 if bug == 'atom_last' else Kk
            O['argmax'][s, :kw] = idx[:kw]
            if c.multi:
                tg = row[8:8 + c.NT].astype(np.int64)
                pick = nanargmax_first(Gs[tg], axis=0)
                for i in range(c.NT):
                    O['HMask'][s, i, :kw] = (pick == i).astype(f32)[:kw]
            else:
                tgt, eps, beta, nf = [f32(v) for v in row[:4]]
                dist = np.abs(idx.astype(f32) - tgt)
                if c.mode == 0:
                    m = (dist < eps).astype(f32)
                else:
                    e = np.exp(-np.power(dist / eps, beta, dtype=f32), dtype=f32)
                    m = e if bug == 'no_nf' else (e / (f32(1) + nf) + nf).astype(f32)
                O['HMask'][s, 0, :kw] = m[:kw]
            HM = np.where(np.isnan(O['HMask'][s][:, :Kk]), 0, O['HMask'][s][:, :Kk])
            den = I['W'].sum(axis=1, dtype=f32) if bug == 'den_kp' else W32.sum(axis=1, dtype=f32)
            if c.nH == 0:
                for i in range(nM):
                    m = ((W32 @ HM[i]) / den[:, None]).astype(f32)
                    O['tfMask'][s, i, 0] = m
                    O['Y'][s, i].real, O['Y'][s, i].imag = m * X.real, m * X.imag
            else:
                v = np.transpose(np.abs(X), (1, 2, 0)).reshape(F, 2 * Tc).astype(f32)
                h = np.full((Kk, 2 * Tc), stale if bug == 'stale_h' else 1.0, f32)
                cs = I['colsumW'][:Kk, None]
                with np.errstate(invalid='ignore', divide='ignore'):
                    for it in range(c.nH):
                        dn = W32 @ h
                        rv = (v / dn).astype(f32) if bug == 'silent_nan' else np.where(dn == 0, f32(0), v / dn).astype(f32)
                        h = (h * ((W32.T @ rv) / cs)).astype(f32)
                O['Rv'][s], O['Hcoef'][s, :Kk] = rv, h
                hd = h.reshape(Kk, Tc, 2)
                for i in range(nM):
                    for ch in range(2):
                        with np.errstate(invalid='ignore', divide='ignore'):
                            dn = W32 @ hd[:, :, ch]
                            m = (W32 @ (hd[:, :, ch] * HM[i])) / dn
                            m = (m if bug == 'silent_nan' else np.where(dn == 0, f32(0), m)).astype(f32)
                        O['tfMask'][s, i, ch] = m
                        O['Y'][s, i, ch].real, O['Y'][s, i, ch].imag = m * X[ch].real, m * X[ch].imag
            src = O['Y'][s]
        # synthesis
        for i in range(nM):
            if c.pow2:
                fr = K.istft_frames32(np.conj(src[i][0]), np.conj(src[i][1]), sw, N)
            else:
                fr = synth_direct(c, I, src[i], f32)[0]
            for t, st in enumerate(c.starts()):
                if c.frames:
                    out[i][:, st:st + N] = fr[:, t]
                else:
                    out[i][:, st:st + N] = out[i][:, st:st + N] + fr[:, t]
            O['out_ring'][s, i] = out[i]
            if not c.frames:
                h0 = c.ring - (c.od + 1 + (1 if bug == 'handout' else 0)) * B
                O['block_out'][s, i] = out[i][:, h0:h0 + B]
        # localisation
        co_, si_ = co[:, :D], si[:, :D]
        if c.alpha > 0:
            gp = NL.gccphat_nl(Cd, co_, si_, c.alpha, f32)
        else:
            term = Cd.real[:, None, :] * co_[:, :, None] + Cd.imag[:, None, :] * si_[:, :, None]
            cnt = (~np.isnan(term)).sum(axis=0)
            with np.errstate(invalid='ignore', divide='ignore'):
                ssum = np.where(np.isnan(term), f32(0), term).sum(axis=0, dtype=f32)
                gp = np.where(cnt > 0, ssum / (f32(F) if bug == 'nan_counted' else cnt.astype(f32)), np.nan).astype(f32)
        O['gccphat'][s] = gp
        pos = int(I['hist_pos'][s])
        for t in range(Tc):
            O['hist'][s][:, pos % c.Lh] = gp[:, t]
            pos += 1
        pos1 = pos % c.Lh
        O['hist_pos'][s] = pos if bug == 'hist_nowrap' else pos1
        if loc_on:
            m = window_mean_f32(O['hist'][s], pos1, c.L)
            if c.multi:
                O['target'][s, 8:8 + c.NT] = pick_peaks(m, c.NT, row[8:8 + c.NT])
            else:
                O['target'][s, 0] = f32(np.argmax(m))
    return O


# ---- the cells: the smallest shapes at which each mechanism of csrc/rt.hip can fail (see tests/test_gpu_rt_stages.py) --------------------------
CELLS = [
    # window sizes x K / Kp x D x Tc; streaming unless said otherwise
    Cell('n64 zero frame', 64, 16, 48, 33, 33, zero_frame=1, ties=True, row=(None, 5.0, 2.0, 0.125)),              # smallest radix-2 size, F = 33: two idle score waves
    Cell('n256 hop 100 boxcar', 256, 100, 300, 100, 65, mode=0, od=1, row=(None, 1.5, 2.0, 0.0), ties=True),
    Cell('n1024 ties', 1024, 512, 512, 64, 130, ties=True),                           # 33 steps per wave: two chunks, ragged second
    Cell('n4', 4, 2, 6, 33, 32, row=(None, 5.0, 1.0, 0.25)),                           # direct sum, F = 3
    Cell('n32 ring wraps', 32, 8, 40, 64, 33, Lh=4, L=4, pos0=3),                     # Tc = 5 > numTDOAHistory = 4
    Cell('n400 block 600 delay 7', 400, 200, 600, 100, 65, od=7, row=(None, 20.0, 1.5, 0.0625)),                     # 16 B = 9600 > 8192: the shift's second chunk
    Cell('n602 delay 1', 602, 301, 301, 64, 32, od=1, row=(None, 3.0, 3.0, 0.0)),      # N % 4 = 2, F = 302 = 4 x 64 + 46
    Cell('n4094', 4094, 2047, 2047, 64, 32),                                          # the raised dynamic-LDS limit
    Cell('n64 hop 80 delay 7', 64, 80, 240, 64, 32, od=7),                            # hop > window: gaps no frame covers
    Cell('n32 hop 40 delay 7', 32, 40, 120, 33, 65, od=7, mode=0),                    # the same on the direct-sum kernels
    Cell('n64 frames nan bins', 64, 64, 192, 64, 33, frames=True, nan_bins=1),
    Cell('n32 frames', 32, 32, 96, 33, 32, frames=True, zero_frame=2),
    Cell('n64 silent right', 64, 32, 64, 64, 32, silent_right=True, decided=False),
    Cell('n32 silent right all-NaN window', 32, 16, 32, 64, 32, silent_right=True, hist_nan=True, L=2),
    Cell('n64 separation off', 64, 32, 32, 64, 32, sep=0),
    Cell('n400 localisation off', 400, 100, 100, 33, 33, loc=0),
    Cell('n64 nonlin', 64, 32, 64, 33, 32, alpha=2.0),
    Cell('bank of 3', 64, 32, 64, 33, 33, S=3, row=(None, 4.0, 2.0, 0.125)),
    Cell('bank of 3 direct inferred', 32, 16, 32, 33, 33, S=3, nH=1),
    Cell('multi 1', 64, 32, 64, 64, 65, NT=1),
    Cell('multi 3', 64, 32, 64, 33, 65, NT=3),
    Cell('multi 8', 256, 128, 128, 100, 130, NT=8, L=1),
    Cell('multi 3 direct', 32, 16, 48, 64, 33, NT=3, od=1),
    Cell('multi 3 all-NaN window', 32, 16, 32, 64, 33, NT=3, silent_right=True, hist_nan=True, L=2),
    Cell('multi 3 inferred', 64, 32, 64, 33, 33, NT=3, nH=1),
    Cell('multi 3 inferred zero frame', 64, 32, 64, 33, 33, NT=3, nH=1, zero_frame=0),
]
# coefficient inference: run with one update, then with two on identical inputs (rule 7)
INFERENCE_CELLS = [
    Cell('n64 inferred', 64, 16, 48, 33, 32, nH=1),
    Cell('n400 inferred', 400, 200, 200, 100, 33, nH=1, mode=0),
    Cell('n1024 inferred', 1024, 512, 512, 64, 32, nH=1),
    Cell('n64 inferred zero frame', 64, 16, 48, 33, 32, nH=1, zero_frame=1),          # a silent frame: no coefficients, mask 0
    Cell('n32 inferred silent right', 32, 16, 48, 64, 33, nH=1, silent_right=True),
]
