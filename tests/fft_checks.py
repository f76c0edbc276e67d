"""Comparison rules of the STFT / iSTFT / PCM stage tests (tests/test_gpu_fft_stages.py), in plain NumPy so that the CPU suite can show
they are sound and sensitive (tests/test_fft_checks.py) without torch or a device.  Every float rule is a worst-case bar per output
element, derived from the arithmetic of csrc/fft.hip and csrc/fft_core.h -- never measured on the code under test.

The radix-2 bar.  One complex transform carries two real signals (forward z = w (xL + j xR); inverse Z = Fa + j Fb, Hermitian-extended),
and every output element of a frame is a sum over that frame's N packed complex inputs z_n, each multiplied by one twiddle per stage.
With u = 2^-24 and no fma (fft.hip is built with -ffp-contract=off), a term picks up per butterfly stage (t = w v; u + t, u - t):
    the float32 twiddle, each component rounded from float64:  |w^ - w| <= u |w|                                   1 u
    the complex product, 4 products and 2 additions:           |fl(w v) - w v| <= sqrt(2) gamma_2 |w| |v|           2 sqrt(2) u   (Higham, ASNA Lemma 3.5)
    the addition u +- t, one rounding per component:           <= u |u +- t| <= u (|u| + |t|)                       1 u
i.e. a relative perturbation of at most (2 + 2 sqrt(2)) u = 4.83 u per stage on the modulus of its contribution, whichever routine orders
the butterflies.  After log2(N) stages every output element is within ((1 + 4.83 u)^log2(N) - 1) sum_n |z_n| of the exact transform of the
exact inputs.  Around the stages there are, not multiplied by log2(N):
    forward: the window product w x (1 u on |z_n|) and the split (Z[k] +- conj(Z[N-k])) / 2 (one addition per component of values bounded
             by sum |z|: sqrt(2) u sum |z|), the halving exact                                                       <= 2.5 u sum |z|
    inverse: the pack Fa + j Fb (one addition per component: 1 u on |z_n|), 1 / N exact (a power of two), the window product (1 u)  <= 2 u sum |z|
With log2(N) >= 6 these are at most 0.42 u per stage, and the second-order terms of (1 + 4.83 u)^12 are below 1e-5 of the first, so
    C_FFT = 6   >=  4.83 + 0.42,       bar = C_FFT log2(N) u sum_n |z_n|     (inverse: times |w[n]| / N for sample n of the frame)
holds for every element, the float64 reference being evaluated from the float32 window and the float32 inputs themselves.  A float32
restatement of the butterflies (fft32 below) measured against numpy.fft in float64 uses at most 0.03 of this bar on the inputs of
tests/test_fft_checks.py: the bar is a worst case, not a typical error, yet a dropped bin, a missing conjugate or a neighbour's frame is
orders of magnitude outside it.

The bar of one channel contains the OTHER channel's magnitude: sum |z_n| = sum w_n hypot(xL_n, xR_n).  That is a property of the
two-in-one transform -- the rounding errors of the loud channel's butterflies land in both halves of the split -- not slack: a quiet
channel beside a loud one is only as accurate, in absolute terms, as the loud one.  The same holds for the two signals of an inverse pair.
A channel that is silent while the other is not therefore need not come out as exact zeros; a frame silent in BOTH channels has bar 0.

|X| and the coherence.  V = hypotf(re, im) of the device's own X.  No statement of hypotf's accuracy for this target was found in the
documentation installed with the toolchain (the device library's sources are not part of it), so HYPOT_U = 4 (u) relative is a STATED
ASSUMPTION, not a derived figure: an error of k ulp is at most 2 k u relative, i.e. the assumption is "hypotf is within 2 ulp".
CC = X0 conj(X1) / |X0| / |X1| of the device's own X, per component:  re = a c + b d (two products, one addition: 2 u (|a c| + |b d|) <=
2 u |X0| |X1|, i.e. 2 u after the divisions), two divisions (2 u on a quotient of modulus <= 1 + ...), two moduli (HYPOT_U u each):
(4 + 2 HYPOT_U) u (1 + 1e-5) absolute, plus the float32 underflow of the products (3 x 2^-149 / (|X0| |X1|)).  Exactly 0 where either
modulus is exactly 0.

Overlap-add and PCM are exact: `istft_ola_kernel` is acc = 0; acc = acc + x in ascending t; acc * gain, all float32 without fma, so the
float32 restatement ola32() of the device's own frames gives the same bits; the PCM pack is the float32 restatement pack_pcm16_32().
"""
import numpy as np

import gcc_checks as C

U32 = 2.0 ** -24
C_FFT = 6.0
HYPOT_U = 4.0
FFT_TB, FFT_TB_4096, ISTFT_TB, ISTFT_SUB = 8, 4, 4, 8      # frames per workgroup: fft_core.h FFT_TB (half of it at n_fft = 4096), fft.hip ISTFT_TB x ISTFT_SUB


def _where(mask):
    return tuple(int(i) for i in np.argwhere(mask)[0])


def ilog2(N):
    l = int(N).bit_length() - 1
    assert 1 << l == N, N
    return l


def twiddles(N):
    """exp(-2j pi k / N), k < N/2, float64 on the host then float32 (engine.fft_twiddles)."""
    return np.exp(-2j * np.pi * np.arange(N // 2, dtype=np.float64) / N).astype(np.complex64)


def bitrev(N):
    logN = ilog2(N)
    i = np.arange(N)
    r = np.zeros(N, np.int64)
    for b in range(logN):
        r |= ((i >> b) & 1) << (logN - 1 - b)
    return r


# ---- float32 restatements ---------------------------------------------------------------------------------------------------------
def fft32(re, im, tw, inverse=False):
    """fft_stages_un of fft_core.h over the last axis in float32, one rounding per operation, the same butterfly expressions in the
    same order: input placed in bit-reversed order, stage s pairs i0 = (grp << s) + pos with i0 + 2^(s-1), w = tw[pos * (N >> s)]
    (conjugated for the inverse), t = w v = (w.x v.x - w.y v.y, w.x v.y + w.y v.x), (u + t, u - t).  No 1/N."""
    re, im = np.asarray(re, np.float32), np.asarray(im, np.float32)
    N = re.shape[-1]
    logN = ilog2(N)
    rev = bitrev(N)
    zr, zi = np.empty_like(re), np.empty_like(im)
    zr[..., rev], zi[..., rev] = re, im                     # z[bitrev(n)] = input n
    twr = np.ascontiguousarray(tw.real).astype(np.float32)
    twi = np.ascontiguousarray(tw.imag).astype(np.float32)
    if inverse:
        twi = -twi
    bf = np.arange(N // 2)
    for s in range(1, logN + 1):
        half = 1 << (s - 1)
        grp, pos = bf >> (s - 1), bf & (half - 1)
        i0 = (grp << s) + pos
        i1 = i0 + half
        wr, wi = twr[pos * (N >> s)], twi[pos * (N >> s)]
        ur, ui, vr, vi = zr[..., i0], zi[..., i0], zr[..., i1], zi[..., i1]
        tr = wr * vr - wi * vi
        ti = wr * vi + wi * vr
        zr[..., i0], zi[..., i0] = ur + tr, ui + ti
        zr[..., i1], zi[..., i1] = ur - tr, ui - ti
    return zr, zi


def frames_of(x, N, hop, T):
    """(..., n) -> (..., T, N): frame t = x[t hop : t hop + N]."""
    idx = np.arange(T)[:, None] * hop + np.arange(N)[None, :]
    return np.asarray(x)[..., idx]


def stft32(x, window, N, hop, T, tw=None):
    """stft_stereo_kernel in float32: x (2, n) float32 -> X (2, F, T) complex64 = conj(fft) of both channels through ONE packed transform."""
    tw = twiddles(N) if tw is None else tw
    w = np.asarray(window, np.float32)
    fr = frames_of(np.asarray(x, np.float32), N, hop, T)                 # (2, T, N)
    zr, zi = fft32(w * fr[0], w * fr[1], tw)
    k = np.arange(N // 2 + 1)
    nk = (N - k) & (N - 1)
    h = np.float32(0.5)
    XL = (h * (zr[:, k] + zr[:, nk])) + 1j * (-h * (zi[:, k] - zi[:, nk]))
    XR = (h * (zi[:, k] + zi[:, nk])) + 1j * (h * (zr[:, k] - zr[:, nk]))
    return np.stack([XL.T, XR.T]).astype(np.complex64)


def stft64(x, window, N, hop, T):
    """float64 reference of the same float32 inputs -> (X (2, F, T) complex128 = conj(rfft(w x)), sum_n |z_n| per frame (T,))."""
    w = np.asarray(window, np.float32).astype(np.float64)
    fr = frames_of(np.asarray(x, np.float32).astype(np.float64), N, hop, T)
    X = np.conj(np.fft.rfft(w * fr, axis=-1))                             # (2, T, F)
    sumabs = np.sum(w * np.hypot(fr[0], fr[1]), axis=-1)
    return np.transpose(X, (0, 2, 1)), sumabs


def stft_bar(sumabs, N, F=None):
    """(F, T) bar of every bin of every frame (both channels): C_FFT log2(N) u sum |z|."""
    bar = C_FFT * ilog2(N) * U32 * np.asarray(sumabs, np.float64)
    return np.broadcast_to(bar[None, :], ((N // 2 + 1) if F is None else F, bar.shape[0]))


def _inverse_inputs(Sa, Sb, dtype, keep_edge_imag=False):
    """(F, T) spectra of a pair -> packed Z (T, N) = Fa + j Fb: the stored conjugate undone, the imaginary parts of the DC and Nyquist
    bins dropped (ifft(...).real keeps only their real part), Hermitian extension."""
    fa, fb = np.conj(np.asarray(Sa)).T.astype(dtype), np.conj(np.asarray(Sb)).T.astype(dtype)      # (T, F)
    if not keep_edge_imag:
        for f in (fa, fb):
            f[:, 0] = f[:, 0].real
            f[:, -1] = f[:, -1].real
    return fa, fb


def istft_frames32(Sa, Sb, window, N, tw=None, keep_edge_imag=False):
    """istft_frames_kernel in float32 -> windowed time frames (2, T, N) of the pair."""
    tw = twiddles(N) if tw is None else tw
    fa, fb = _inverse_inputs(Sa, Sb, np.complex64, keep_edge_imag)
    T, F = fa.shape
    zr, zi = np.zeros((T, N), np.float32), np.zeros((T, N), np.float32)
    zr[:, :F], zi[:, :F] = fa.real - fb.imag, fa.imag + fb.real
    k = np.arange(1, N // 2)
    zr[:, N - k], zi[:, N - k] = fa.real[:, k] + fb.imag[:, k], fb.real[:, k] - fa.imag[:, k]
    vr, vi = fft32(zr, zi, tw, inverse=True)
    w, invN = np.asarray(window, np.float32), np.float32(1.0 / N)
    return np.stack([w * (vr * invN), w * (vi * invN)])


def istft_frames64(Sa, Sb, window, N):
    """float64 reference -> (frames (2, T, N), sum_n |z_n| per frame (T,)) with z = Fa + j Fb over all N bins."""
    fa, fb = _inverse_inputs(np.asarray(Sa, np.complex64), np.asarray(Sb, np.complex64), np.complex128)
    w = np.asarray(window, np.float32).astype(np.float64)
    ext = lambda f: np.concatenate([f, np.conj(f[:, -2:0:-1])], axis=1)
    sumabs = np.sum(np.abs(ext(fa) + 1j * ext(fb)), axis=1)
    return np.stack([w * np.fft.irfft(fa, N, axis=1), w * np.fft.irfft(fb, N, axis=1)]), sumabs


def frames_bar(sumabs, window, N):
    """(T, N) bar of every sample of every frame (both signals of the pair)."""
    w = np.abs(np.asarray(window, np.float32).astype(np.float64))
    return C_FFT * ilog2(N) * U32 * np.asarray(sumabs, np.float64)[:, None] * w[None, :] / N


def ola32(frames, N, hop, first, L, gain, skip=None):
    """istft_ola_kernel in float32: frames (..., T, N) -> (..., L) = samples first .. first+L-1 of the overlap-added stream; every sample
    starts from 0 and adds its frames in ASCENDING t, then * gain.  `skip`: a frame index left out (for the CPU suite)."""
    frames = np.asarray(frames, np.float32)
    T = frames.shape[-2]
    acc = np.zeros(frames.shape[:-2] + (N + hop * (T - 1),), np.float32)
    for t in range(T):
        if t != skip:
            acc[..., t * hop:t * hop + N] = acc[..., t * hop:t * hop + N] + frames[..., t, :]
    return acc[..., first:first + L] * np.float32(gain)


def istft_length(N, hop, T, center):
    trim = N // 2 if center else 0
    return trim, N + hop * (T - 1) - 2 * trim


def fused_write_counts(N, hop, T, center):
    """How often istft_fused_kernel writes each of the L output samples: its hand-out rules restated (a workgroup owns G = ISTFT_TB *
    ISTFT_SUB hops, starts `halo` = ceil(N / hop) - 1 frames early, slides an accumulator of span = N + (ISTFT_TB - 1) hop samples and
    hands out i < min(shift, span) before every sub-batch and the whole span at the end, each only inside its own range).  The contract
    is 1 everywhere."""
    TB, G = ISTFT_TB, ISTFT_TB * ISTFT_SUB
    trim, L = istft_length(N, hop, T, center)
    span, halo = N + hop * (TB - 1), -(-N // hop) - 1
    count = np.zeros(L, np.int64)

    def hand_out(base, n, own_lo, own_hi):
        lo, hi = max(base, own_lo) - trim, min(base + n, own_hi) - trim
        lo, hi = max(lo, 0), min(hi, L)
        if hi > lo:
            count[lo:hi] += 1
    for t0 in range(0, T, G):
        t_end = min(t0 + G, T)
        t_first = max(t0 - halo, 0)
        own_lo, own_hi = t0 * hop, ((T - 1) * hop + N if t_end == T else t_end * hop)
        base = t_first * hop
        for fs in range(t_first, t_end, TB):
            shift = fs * hop - base
            if shift > 0:
                hand_out(base, min(shift, span), own_lo, own_hi)
                base += shift
        hand_out(base, span, own_lo, own_hi)
    return count


def pcm2float32(pcm):
    """wavfile.pcm2float for int16: float32(x) / 32768 (exact)."""
    return np.asarray(pcm, np.int16).astype(np.float32) / np.float32(32768)


def pack_pcm16_32(y, round_instead=False, rescale_from=1.0):
    """gccnmf_pack_pcm16 = wavwrite + float2pcm per group in float32: y (g, 2, L) -> (pcm (g, L, 2) int16, peak image (g,) uint32).
    peak = max |y| over the group, compared as bit images (NaN / Inf images >= 0x7F800000 rank above every finite value); peak >= 1 and
    finite: x / peak * 0.99; then the device's stated policy NaN -> 0 and no rescale in a non-finite group; x * 32768, clipped to
    [-32768, 32767] (so +-Inf clip), truncated toward zero.  `round_instead`, `rescale_from`: the mistakes the CPU suite applies."""
    y = np.ascontiguousarray(y, np.float32)
    g = y.shape[0]
    bits = np.abs(y).view(np.uint32).reshape(g, -1).max(axis=1)
    out = np.empty((g, y.shape[2], 2), np.int16)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(g):
            a = y[i].copy()
            pk = bits[i:i + 1].view(np.float32)[0]
            if bits[i] < 0x7F800000 and pk >= np.float32(rescale_from):
                a = a / pk * np.float32(0.99)
            a = np.where(a == a, a, np.float32(0))
            a = np.minimum(np.maximum(a * np.float32(32768), np.float32(-32768)), np.float32(32767))
            a = np.rint(a) if round_instead else np.trunc(a)
            out[i] = a.astype(np.int32).astype(np.int16).T
    return out, bits


# ---- signals shared by the CPU and the GPU suite -----------------------------------------------------------------------------------
def amplitudes(n):
    """Powers of two from 2^-3 to 2^3, cycling: an exchanged or leaked neighbour is far outside the receiving frame's bar."""
    return (2.0 ** ((np.arange(n) * 3) % 7 - 3)).astype(np.float32)


def stage_signal(N, hop, T, seed, right_scale=1.0, silent=True):
    """(2, (T-1) hop + N) float32 white noise whose amplitude follows amplitudes() per hop; with `silent` (and T >= 3) frame T // 2 is
    wholly silent in both channels: a run of N zeros starting at the multiple (T // 2) hop.  -> (x, silent frame index or None)."""
    n = (T - 1) * hop + N
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((2, n)).astype(np.float32) * np.repeat(amplitudes(-(-n // hop)), hop)[:n]
    x[1] *= np.float32(right_scale)
    ts = T // 2 if (silent and T >= 3) else None
    if ts is not None:
        x[:, ts * hop:ts * hop + N] = 0
    return x, ts


def stage_spectra(nsig, F, T, seed, silent=True):
    """(nsig, F, T) complex64, frame t scaled by amplitudes()[t], non-zero imaginary parts in the DC and Nyquist rows, frame T // 2
    silent (T >= 3)."""
    rng = np.random.RandomState(seed)
    S = (rng.standard_normal((nsig, F, T)) + 1j * rng.standard_normal((nsig, F, T))) * amplitudes(T)[None, None, :]
    ts = T // 2 if (silent and T >= 3) else None
    if ts is not None:
        S[:, :, ts] = 0
    return S.astype(np.complex64), ts


# ---- rules ---------------------------------------------------------------------------------------------------------------------------
def check_bar(got, ref64, bar, what='result'):
    """Every element finite and |got - ref64| <= bar; prints and returns the worst share of the bar (0 / 0 counts as 0)."""
    got, ref64 = np.asarray(got), np.asarray(ref64)
    bar = np.broadcast_to(np.asarray(bar, np.float64), ref64.shape)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    bad = ~np.isfinite(got)
    assert not bad.any(), '%s: %d non-finite elements (first at %s): not written?' % (what, int(bad.sum()), _where(bad))
    err = np.abs(got.astype(np.complex128 if np.iscomplexobj(got) or np.iscomplexobj(ref64) else np.float64) - ref64)
    with np.errstate(divide='ignore', invalid='ignore'):
        share = np.where(err == 0, 0.0, err / bar)
    worst = float(share.max()) if share.size else 0.0
    print('%s: worst share of the bar %.4f' % (what, worst))
    bad = err > bar
    if bad.any():
        i = _where(bad)
        raise AssertionError('%s: %d elements outside the bar, first at %s: got %r, float64 %r, |err| %.3e > %.3e'
                             % (what, int(bad.sum()), i, got[i], ref64[i], err[i], bar[i]))
    return worst


def check_bits(got, want, what='result'):
    """The same bits element by element (NaN images included; -0 differs from +0)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = got.view(view) != want.view(view)
    assert not bad.any(), '%s: %d elements differ in their bits, first at %s: %r vs %r' % (what, int(bad.sum()), _where(bad), got[_where(bad)],
                                                                                       want[_where(bad)])


def check_modulus(V, X, what='V'):
    """V = |X| of the SAME float32 X within HYPOT_U u relative (+ half the smallest subnormal); exactly 0 where X is."""
    X = np.asarray(X)
    ref = np.hypot(X.real.astype(np.float64), X.imag.astype(np.float64))
    worst = check_bar(V, ref, HYPOT_U * U32 * ref + 2.0 ** -150, what)
    zero = ref == 0
    assert not (np.asarray(V)[zero] != 0).any(), '%s: not exactly 0 where X is' % what
    return worst


def check_coherence(CC, X0, X1, V0, V1, what='CC'):
    """CC (complex, from the two planes) = X0 conj(X1) / |X0| / |X1| of the device's own X per component within (4 + 2 HYPOT_U) u (+ the
    underflow term); exactly 0 where either device modulus is exactly 0."""
    X0, X1 = np.asarray(X0).astype(np.complex128), np.asarray(X1).astype(np.complex128)
    a0, a1 = np.abs(X0), np.abs(X1)
    zero = (np.asarray(V0) == 0) | (np.asarray(V1) == 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        ref = np.where(zero, 0.0, X0 * np.conj(X1) / a0 / a1)
        bar = np.where(zero, 0.0, (4 + 2 * HYPOT_U) * U32 * (1 + 1e-5) + 3 * 2.0 ** -149 / (a0 * a1))
    CC = np.asarray(CC)
    C.check_written(CC.real, what)
    C.check_written(CC.imag, what)
    worst = max(check_bar(CC.real, ref.real, bar, what + ' (re)'), check_bar(CC.imag, ref.imag, bar, what + ' (im)'))
    assert not (CC[zero] != 0).any(), '%s: not exactly 0 where a modulus is 0' % what
    return worst


def check_guard(tail, sentinel, what='guard'):
    """The sentinel-filled tail behind an output's logical extent is untouched."""
    tail = np.asarray(tail)
    bad = tail != sentinel
    assert not bad.any(), '%s: %d elements beyond the logical extent changed (first at %s: %r)' % (what, int(bad.sum()), _where(bad),
                                                                                                 tail[_where(bad)])
