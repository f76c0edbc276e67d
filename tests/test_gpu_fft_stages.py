"""-m gpu: every entry point of csrc/fft.hip called directly through the C ABI, element-wise against float64 (tests/fft_checks.py).

Inputs are built on the host at the smallest shapes at which the kernels can go wrong -- none is the workload's.  The valid region of every
output is NaN-filled before each call, scratch holds other garbage, the padding of X, V, CC and spec is zero before the call and must be
zero after it (the kernels write only bins f < F and frames t < T: the padding is the caller's), and a sentinel-filled guard tail behind y,
pcm and frames must be untouched.  Per-hop (forward) or per-frame (inverse) amplitudes cycle over 2^-3 .. 2^3, so that an exchanged or
leaked frame is far outside the receiving frame's bar, and one frame is wholly silent: there X, V and CC must be exactly 0.  Every check
prints its worst share of the bar before it asserts.

Frame counts.  The T edges come from compile-time constants (mirrored in fft_checks: FFT_TB, ISTFT_TB, ISTFT_SUB -- follow them there if
they change): the forward transform and the two-kernel inverse run FFT_TB = 8 frames per workgroup (T = 1, 7, 8, 9, 17: less than one,
one short of, exactly, one more than one, and two workgroups plus one), 4 at n_fft = 4096 (T = 1, 3, 4, 5); the fused inverse owns
ISTFT_TB x ISTFT_SUB = 4 x 8 = 32 hops per workgroup, takes frames 4 at a time and starts ceil(n_fft / hop) - 1 frames early (T = 1, 3, 4, 5,
31, 32, 33, 65).  Every build runs the register-pass FFT (fft_core.h).
"""
import numpy as np
import pytest

import fft_checks as K
import gcc_checks as C

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
GARBAGE, SENTINEL, GUARD = 1e30, -7.0, 1024
NAN = float('nan')


@pytest.fixture(scope='module')
def lib():
    from gcc_nmf_amd import _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def pitches(F, T):
    from gcc_nmf_amd.engine import Geometry
    g = Geometry(F, T, 1)
    return g.Fp, g.Np, g.Tp


_tables = {}


def tables(N, inverse=False):
    """float32 window (Hann; x 2/3 for the inverse, as the reference's default) and twiddles, host and device."""
    key = (N, inverse)
    if key not in _tables:
        from gcc_nmf_amd.engine import fft_twiddles
        w = (np.hanning(N) * (2.0 / 3 if inverse else 1.0)).astype(np.float32)
        tw = fft_twiddles(N)
        assert np.array_equal(tw.view(np.complex64), K.twiddles(N))
        _tables[key] = (w, dev(w), dev(tw))
    return _tables[key]


# ---- forward transform -----------------------------------------------------------------------------------------------------------------
def run_stft(lib, files, N, hop, T, with_V=True, with_CC=True, pcm=False):
    """files: list of (2, n) float32 (or with pcm (n, 2) int16), n = (T-1) hop + N exactly; the device buffer holds them `stride` apart with
    stride > a file's size and ENDS with the last file's last sample.  -> dict of host arrays X (B, 2, Fp, Tp) complex, V (B, Fp, Np),
    CC (B, 2, Fp, Tp)."""
    B, n, F = len(files), (T - 1) * hop + N, N // 2 + 1
    Fp, Np, Tp = pitches(F, T)
    w, dwin, dtw = tables(N)
    if pcm:
        stride = n + 13                                                  # stereo frames between files
        buf = np.full(((B - 1) * stride + n, 2), 12345, np.int16)
        for b, f in enumerate(files):
            assert f.shape == (n, 2) and f.dtype == np.int16
            buf[b * stride:b * stride + n] = f
        entry = lib.gccnmf_stft_stereo_pcm16
    else:
        stride = 2 * n + 24                                              # floats between files
        buf = np.full((B - 1) * stride + 2 * n, GARBAGE, np.float32)
        for b, f in enumerate(files):
            assert f.shape == (2, n) and f.dtype == np.float32
            buf[b * stride:b * stride + 2 * n] = f.reshape(-1)
        entry = lib.gccnmf_stft_stereo
    dx = dev(buf)
    X = torch.zeros((B, 2, Fp, Tp, 2), dtype=torch.float32, device='cuda')
    X[:, :, :F, :T] = NAN
    V = torch.zeros((B, Fp, Np), dtype=torch.float32, device='cuda')
    V[:, :F, :2 * T] = NAN
    CC = torch.zeros((B, 2, Fp, Tp), dtype=torch.float32, device='cuda')
    CC[:, :, :F, :T] = NAN
    rc = entry(ptr(dx), stride, n, N, hop, T, B, ptr(dwin), ptr(dtw), ptr(X), ptr(V) if with_V else 0, ptr(CC) if with_CC else 0, stream())
    assert rc == OK, rc
    Xh = host(X)
    return dict(X=Xh[..., 0] + 1j * Xh[..., 1], Xraw=Xh, V=host(V), CC=host(CC))


def check_stft_file(r, b, x, N, hop, T, silent, with_V=True, with_CC=True, what=''):
    F = N // 2 + 1
    w = tables(N)[0]
    X, V, CC = r['X'][b], r['V'][b], r['CC'][b]
    ref, sumabs = K.stft64(x, w, N, hop, T)
    bar = K.stft_bar(sumabs, N)
    shares = {}
    shares['X'] = max(K.check_bar(X[c, :F, :T].astype(np.complex64), ref[c], bar, '%s X channel %d (file %d)' % (what, c, b)) for c in range(2))
    pad = r['Xraw'][b].copy()
    pad[:, :F, :T] = 0
    C.check_zero(pad, '%s X padding (file %d)' % (what, b))
    Xv = X[:, :F, :T].astype(np.complex64)
    if with_V:
        shares['V'] = max(K.check_modulus(V[:F, c * T:(c + 1) * T], Xv[c], '%s V channel %d (file %d)' % (what, c, b)) for c in range(2))
        pad = V.copy()
        pad[:F, :2 * T] = 0
        C.check_zero(pad, '%s V padding (file %d)' % (what, b))
    else:
        assert np.isnan(V[:F, :2 * T]).all(), 'V was written although NULL was passed'
    if with_CC:
        assert with_V
        cc = (CC[0, :F, :T] + 1j * CC[1, :F, :T]).astype(np.complex64)
        shares['CC'] = K.check_coherence(cc, Xv[0], Xv[1], V[:F, :T], V[:F, T:2 * T], '%s CC (file %d)' % (what, b))
        pad = CC.copy()
        pad[:, :F, :T] = 0
        C.check_zero(pad, '%s CC padding (file %d)' % (what, b))
    if silent is not None:                                               # silent in both channels: exactly 0, not NaN, not a residue
        assert sumabs[silent] == 0
        C.check_zero(r['Xraw'][b][:, :F, silent], '%s X of the silent frame' % what)
        if with_V:
            C.check_zero(V[:F, [silent, T + silent]], '%s V of the silent frame' % what)
        if with_CC:
            C.check_zero(CC[:, :F, silent], '%s CC of the silent frame' % what)
    return shares


def valid_bits(r, b, F, T):
    return [np.ascontiguousarray(r['Xraw'][b][:, :F, :T]), np.ascontiguousarray(r['V'][b][:F, :2 * T]), np.ascontiguousarray(r['CC'][b][:, :F, :T])]


# (n_fft, hop, T, batch, right channel's scale): hops that divide n_fft, one that does not (256 / 100), hop = n_fft; T around 8 frames per
# workgroup (4 at n_fft = 4096); batch 1 or 3; one cell with the left channel 1e3 louder than the right
STFT_CELLS = [(64, 16, 1, 1, 1.0), (64, 16, 17, 3, 1.0), (64, 64, 9, 1, 1.0), (64, 24, 8, 1, 1.0),
              (256, 100, 7, 1, 1.0), (256, 100, 8, 3, 1.0), (256, 256, 9, 1, 1.0), (256, 64, 17, 1, 1e-3),
              (1024, 256, 9, 3, 1.0), (1024, 1024, 1, 1, 1.0), (1024, 300, 8, 1, 1.0), (1024, 256, 7, 1, 1e-3), (1024, 128, 17, 1, 1.0),
              (2048, 512, 17, 1, 1.0), (2048, 2048, 7, 1, 1.0), (2048, 600, 8, 3, 1.0), (2048, 512, 9, 1, 1.0), (2048, 256, 1, 1, 1.0),
              (4096, 1024, 5, 3, 1.0), (4096, 1000, 4, 1, 1.0), (4096, 4096, 3, 1, 1.0), (4096, 1024, 1, 1, 1.0)]


@pytest.mark.parametrize('N,hop,T,batch,right', STFT_CELLS, ids=['n%d-hop%d-T%d-b%d-r%g' % c for c in STFT_CELLS])
def test_stft_against_float64(lib, N, hop, T, batch, right):
    F = N // 2 + 1
    files, silent = [], []
    for b in range(batch):
        x, ts = K.stage_signal(N, hop, T, 100 * N + 10 * T + b, right)
        files.append(x)
        silent.append(ts)
    what = 'stft n_fft=%d hop=%d T=%d' % (N, hop, T)
    r = run_stft(lib, files, N, hop, T)
    shares = [check_stft_file(r, b, files[b], N, hop, T, silent[b], what=what) for b in range(batch)]
    print('%s batch=%d: worst shares X %.4f V %.4f CC %.4f' % (what, batch, max(s['X'] for s in shares), max(s['V'] for s in shares),
                                                            max(s['CC'] for s in shares)))
    # (for the record, not a rule: how many elements differ in their bits from the float32 restatement of the butterflies)
    w = tables(N)[0]
    differ = sum(int((np.ascontiguousarray(K.stft32(files[b], w, N, hop, T)).view(np.uint64)
                      != np.ascontiguousarray(r['X'][b][:, :F, :T].astype(np.complex64)).view(np.uint64)).sum()) for b in range(batch))
    print('%s: %d of %d elements of X differ in their bits from the float32 restatement' % (what, differ, batch * 2 * F * T))
    # V or CC NULL: the other outputs keep their bits, the skipped one is not touched
    noV = run_stft(lib, files, N, hop, T, with_V=False, with_CC=False)
    noC = run_stft(lib, files, N, hop, T, with_CC=False)
    onlyC = run_stft(lib, files, N, hop, T, with_V=False)
    for b in range(batch):
        K.check_bits(noV['Xraw'][b], r['Xraw'][b], what + ' X without V and CC')
        K.check_bits(noC['Xraw'][b], r['Xraw'][b], what + ' X without CC')
        K.check_bits(noC['V'][b], r['V'][b], what + ' V without CC')
        K.check_bits(onlyC['Xraw'][b], r['Xraw'][b], what + ' X without V')
        K.check_bits(onlyC['CC'][b], r['CC'][b], what + ' CC without V')
        assert np.isnan(noV['V'][b][:F, :2 * T]).all() and np.isnan(noV['CC'][b][:, :F, :T]).all() and np.isnan(noC['CC'][b][:, :F, :T]).all()
        assert np.isnan(onlyC['V'][b][:F, :2 * T]).all()
        check_stft_file(noV, b, files[b], N, hop, T, silent[b], with_V=False, with_CC=False, what=what + ' (X only)')
    # a file alone = the same file inside the batch
    for b in sorted({0, batch - 1}) if batch > 1 else []:
        alone = run_stft(lib, [files[b]], N, hop, T)
        for got, want, name in zip(valid_bits(alone, 0, F, T), valid_bits(r, b, F, T), ('X', 'V', 'CC')):
            K.check_bits(got, want, '%s %s of file %d alone' % (what, name, b))
    # frame t of x = frame 0 of x[:, t hop:] (whichever row of whichever workgroup transforms it)
    for t in sorted(t for t in {1, T // 2, T - 1} if 0 < t < T):
        tail = run_stft(lib, [np.ascontiguousarray(files[0][:, t * hop:])], N, hop, T - t)
        whole, part = valid_bits(r, 0, F, T), valid_bits(tail, 0, F, T - t)
        K.check_bits(part[0], np.ascontiguousarray(whole[0][:, :, t:]), '%s X from frame %d on' % (what, t))
        K.check_bits(part[2], np.ascontiguousarray(whole[2][:, :, t:]), '%s CC from frame %d on' % (what, t))
        K.check_bits(part[1], np.ascontiguousarray(np.concatenate([whole[1][:, t:T], whole[1][:, T + t:]], axis=1)), '%s V from frame %d on' % (what, t))


def pcm_file(N, hop, T, seed):
    """(n, 2) int16: noise under the amplitude cycle, with -32768, 32767, 0 and a run of alternating extremes."""
    n = (T - 1) * hop + N
    rng = np.random.RandomState(seed)
    amp = np.repeat(K.amplitudes(-(-n // hop)), hop)[:n] / 8.0
    p = np.clip(rng.standard_normal((n, 2)) * 8000 * amp[:, None], -32768, 32767).astype(np.int16)
    p[0], p[1], p[2] = (-32768, 32767), (32767, -32768), (0, 0)
    k = min(N // 2, n - 8)
    alt = np.where(np.arange(k) % 2 == 0, -32768, 32767).astype(np.int16)
    p[5:5 + k, 0], p[5:5 + k, 1] = alt, -1 - alt                          # (-32768, 32767), (32767, -32768), ...
    p[n - 1] = (32767, -32768)
    return p


PCM_CELLS = [(64, 16, 9, 3), (256, 100, 8, 1), (1024, 256, 9, 3), (2048, 512, 7, 1), (4096, 1024, 5, 3), (4096, 1000, 4, 1)]


@pytest.mark.parametrize('N,hop,T,batch', PCM_CELLS, ids=['n%d-hop%d-T%d-b%d' % c for c in PCM_CELLS])
def test_stft_pcm16_entry_is_bitwise_the_float_entry(lib, N, hop, T, batch):
    """gccnmf_stft_stereo_pcm16 (interleaved int16, frame_stride > n_samples) gives the bits of gccnmf_stft_stereo fed
    pcm.astype(float32) / 32768 -- in X, V and CC -- and both meet the float64 bars on that input (full-scale samples included)."""
    F = N // 2 + 1
    pcms = [pcm_file(N, hop, T, 7 * N + b) for b in range(batch)]
    floats = [np.ascontiguousarray(K.pcm2float32(p).T) for p in pcms]
    a = run_stft(lib, pcms, N, hop, T, pcm=True)
    f = run_stft(lib, floats, N, hop, T)
    what = 'pcm16 stft n_fft=%d hop=%d T=%d' % (N, hop, T)
    for b in range(batch):
        for got, want, name in zip(valid_bits(a, b, F, T), valid_bits(f, b, F, T), ('X', 'V', 'CC')):
            K.check_bits(got, want, '%s %s (file %d)' % (what, name, b))
        check_stft_file(a, b, floats[b], N, hop, T, None, what=what)


# ---- inverse transform -----------------------------------------------------------------------------------------------------------------
def fused_accepts(N, hop):
    return N + (K.ISTFT_TB - 1) * hop <= 2048 and hop <= N


def run_istft(lib, S, N, hop, T, center, gain, fused):
    """S (B, nsig, F, T) complex64 -> (rc, frames (B, nsig, T, N) or None, y (B, nsig, L)); guards checked here."""
    B, nsig, F = S.shape[0], S.shape[1], N // 2 + 1
    Fp, Np, Tp = pitches(F, T)
    w, dwin, dtw = tables(N, inverse=True)
    trim, L = K.istft_length(N, hop, T, center)
    img = np.zeros((B, nsig, Fp, Tp, 2), np.float32)
    img[:, :, :F, :T, 0], img[:, :, :F, :T, 1] = S.real, S.imag
    dS = dev(img)
    ny, nf = B * nsig * L, B * nsig * T * N
    y = torch.full((ny + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
    y[:ny] = NAN
    frames = None
    if not fused:
        frames = torch.full((nf + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
        frames[:nf] = NAN
    rc = lib.gccnmf_istft_ola(ptr(dS), nsig, N, hop, T, B, ptr(dwin), ptr(dtw), gain, center, ptr(frames), ptr(y), stream())
    yh = host(y)
    K.check_guard(yh[ny:], SENTINEL, 'y guard')
    assert np.array_equal(host(dS), img), 'the spectrogram was written to'
    fh = None
    if frames is not None:
        fh = host(frames)
        K.check_guard(fh[nf:], SENTINEL, 'frames guard')
        fh = fh[:nf].reshape(B, nsig, T, N)
    return rc, fh, yh[:ny].reshape(B, nsig, L)


# (n_fft, hop, T, center, nsig, batch): hop in {n_fft / 8, n_fft / 4, a non-divisor, n_fft} and 256 / 300 (hop > n_fft); T around the fused
# kernel's 4-frame sub-batches and 32-hop workgroups and the two-kernel form's 8 (4) frames per workgroup
ISTFT_CELLS = [(64, 8, 65, 1, 2, 1), (64, 16, 33, 0, 6, 3), (64, 64, 5, 1, 2, 1), (64, 20, 32, 1, 2, 1), (64, 16, 1, 0, 2, 1), (64, 8, 4, 1, 2, 3),
               (256, 32, 33, 1, 6, 1), (256, 64, 31, 1, 2, 3), (256, 100, 65, 0, 2, 1), (256, 256, 4, 0, 2, 1), (256, 64, 3, 0, 6, 1),
               (256, 300, 6, 0, 2, 1), (256, 300, 33, 1, 2, 1), (256, 64, 32, 1, 2, 1), (256, 100, 5, 1, 2, 1),
               (1024, 128, 33, 1, 2, 1), (1024, 256, 65, 1, 6, 1), (1024, 256, 3, 1, 2, 3), (1024, 341, 32, 0, 2, 1), (1024, 342, 5, 1, 2, 1),
               (1024, 1024, 4, 0, 2, 1), (1024, 256, 31, 0, 2, 1),
               (2048, 256, 5, 1, 2, 1), (2048, 512, 33, 1, 2, 1), (2048, 2048, 3, 0, 6, 1), (2048, 700, 4, 1, 2, 3),
               (4096, 512, 5, 1, 2, 1), (4096, 1024, 33, 0, 2, 1), (4096, 1000, 4, 1, 2, 3), (4096, 4096, 1, 0, 2, 1), (4096, 1024, 3, 1, 6, 1)]


@pytest.mark.parametrize('N,hop,T,center,nsig,batch', ISTFT_CELLS, ids=['n%d-hop%d-T%d-c%d-s%d-b%d' % c for c in ISTFT_CELLS])
def test_istft_against_float64_and_fused_form_bitwise(lib, N, hop, T, center, nsig, batch):
    F, gain = N // 2 + 1, 1.7
    w = tables(N, inverse=True)[0]
    trim, L = K.istft_length(N, hop, T, center)
    S = np.stack([K.stage_spectra(nsig, F, T, 1000 * N + 10 * T + b)[0] for b in range(batch)])
    silent = T // 2 if T >= 3 else None
    what = 'istft n_fft=%d hop=%d T=%d center=%d' % (N, hop, T, center)
    rc, frames, y = run_istft(lib, S, N, hop, T, center, gain, fused=False)
    assert rc == OK, rc
    worst = 0.0
    for b in range(batch):
        for p in range(nsig // 2):
            ref, sumabs = K.istft_frames64(S[b, 2 * p], S[b, 2 * p + 1], w, N)
            bar = K.frames_bar(sumabs, w, N)
            for c in range(2):
                worst = max(worst, K.check_bar(frames[b, 2 * p + c], ref[c], bar, '%s frames of signal %d (file %d)' % (what, 2 * p + c, b)))
        if silent is not None:
            C.check_zero(frames[b, :, silent], what + ' frames of the silent frame')
    print('%s nsig=%d batch=%d: worst share of the frames %.4f' % (what, nsig, batch, worst))
    # y = the float32 ascending-frame sum of the device's own frames, times the gain: the same bits (every sample written, gaps 0)
    C.check_written(y, what + ' y')
    K.check_bits(y, K.ola32(frames, N, hop, trim, L, gain), what + ' y against the float32 overlap-add of the frames')
    # the fused form: the same bits wherever it accepts the call, GCCNMF_ERR_UNSUPPORTED (and nothing written) elsewhere
    rc, _, yf = run_istft(lib, S, N, hop, T, center, gain, fused=True)
    if fused_accepts(N, hop):
        assert rc == OK, rc
        K.check_bits(yf, y, what + ' fused form against the two-kernel form')
    else:
        assert rc == ERR_UNSUPPORTED, rc
        assert np.isnan(yf).all(), 'an unsupported call wrote to y'


def test_ola_frames_halo_is_bitwise_the_unsplit_overlap_add(lib):
    """The frames of a two-kernel run, cut into `prev` (halo = 0 or 3 frames) and `frames` at several places of the stream, windows of
    the stream shorter than it (first_sample >= 0), nsig 1 or 6: the same bits as the unsplit call on the concatenated frames and as the
    float32 restatement; nothing beyond y[nsig][L] changes."""
    for N, hop, T in ((256, 64, 14), (256, 100, 11), (64, 64, 9), (1024, 256, 10)):
        S = K.stage_spectra(6, N // 2 + 1, T, N + hop)[0][None]
        rc, frames, _ = run_istft(lib, S, N, hop, T, 0, 1.0, fused=False)
        assert rc == OK
        frames = frames[0]                                               # (6, T, N)
        for nsig in (1, 6):
            for halo in (0, 3):
                for s0, Tc in ((0, T - halo), (2, T - halo - 2), (4, 3), (T - halo - 1, 1)):
                    if Tc < 1 or s0 + halo + Tc > T:
                        continue
                    seq = np.ascontiguousarray(frames[:nsig, s0:s0 + halo + Tc])
                    total = N + hop * (halo + Tc - 1)
                    for first, L in ((0, total), (0, total - 1), (N // 2, total - N), (hop + 3, min(257, total - hop - 3)), (total - 1, 1)):
                        if L < 1:
                            continue
                        gain = 0.6
                        want = K.ola32(seq, N, hop, first, L, gain)
                        outs = []
                        for prev, cur, h in ((seq[:, :halo], seq[:, halo:], halo), (None, seq, 0)):
                            dprev = dev(prev) if h else None
                            dcur = dev(cur)
                            y = torch.full((nsig * L + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
                            y[:nsig * L] = NAN
                            rc = lib.gccnmf_ola_frames_halo(ptr(dprev), h, ptr(dcur), nsig, N, hop, cur.shape[1], first, L, gain, ptr(y), stream())
                            assert rc == OK, rc
                            yh = host(y)
                            K.check_guard(yh[nsig * L:], SENTINEL, 'y guard')
                            outs.append(yh[:nsig * L].reshape(nsig, L))
                        tag = 'ola_frames_halo n_fft=%d hop=%d nsig=%d halo=%d frames %d..%d first=%d L=%d' % (N, hop, nsig, halo, s0, s0 + halo + Tc, first, L)
                        K.check_bits(outs[0], want, tag + ' (split) against the restatement')
                        K.check_bits(outs[1], want, tag + ' (unsplit) against the restatement')


# ---- PCM egress ------------------------------------------------------------------------------------------------------------------------
def pcm_group(kind, L, rng):
    """(2, L) float32 of one group (= one wavwrite call).  Special samples go to fixed places modulo L, the later ones winning at L = 1."""
    one, below = np.float32(1), np.nextafter(np.float32(1), np.float32(0))
    y = rng.uniform(-0.5, 0.5, (2, L)).astype(np.float32)
    put = lambda c, i, v: y.__setitem__((c, i % L), np.float32(v))
    if kind == 'quiet':
        pass
    elif kind == 'peak1':
        put(1, L // 2, one)
    elif kind == 'below1':                                               # peak one ulp below 1: not rescaled, and that sample clips to 32767
        put(0, L // 3, below)
    elif kind == 'loud40':
        y *= np.float32(60)
        put(1, L - 1, -40.0)                                            # (the noise is below 30: the peak is exactly 40)
    elif kind == 'steps':                                                # k / 32768 -+ 1 ulp around the truncation steps
        k = rng.randint(-32767, 32767, (2, L)).astype(np.float32) / np.float32(32768)
        y = np.where(rng.rand(2, L) < 0.5, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-2))).astype(np.float32)
        y[0, 0] = k[0, 0]
    elif kind == 'nan':                                                  # no rescale in a non-finite group: -1.0 -> -32768, just below 1 -> 32767
        put(0, 1, 30.0)
        put(1, 2, -1.0)
        put(1, 3, below)
        put(0, 0, np.nan)
    elif kind == 'inf':
        put(1, 1, -1.0)
        put(0, 2, below)
        put(0, 3, -np.inf)
        put(1, 0, np.inf)
    else:
        raise ValueError(kind)
    return y


PCM_KINDS = ('quiet', 'peak1', 'below1', 'loud40', 'steps', 'nan', 'inf')
PCM_CALLS = [(k,) for k in PCM_KINDS] + [('loud40', 'nan', 'quiet', 'inf', 'peak1'), ('below1', 'steps', 'inf', 'loud40', 'quiet')]


@pytest.mark.parametrize('L', [1, 255, 256, 257, 20000])
def test_pack_pcm16_is_exactly_the_float32_restatement(lib, L):
    """groups 1 or 5; 2 L = 40000 exceeds the 64 x 256 threads of the peak kernel's first sweep.  NaN and Inf groups ride in the same call as
    a loud finite group and a quiet one, which they must not affect."""
    rng = np.random.RandomState(L)
    for kinds in PCM_CALLS:
        g = len(kinds)
        y = np.stack([pcm_group(k, L, rng) for k in kinds])
        want, bits = K.pack_pcm16_32(y)
        dy = dev(y)
        pcm = torch.full((g * L * 2 + GUARD,), 12345, dtype=torch.int16, device='cuda')
        peak = torch.full((g + 16,), 0x7FC12345, dtype=torch.int32, device='cuda')           # scratch: garbage before the call
        assert lib.gccnmf_pack_pcm16(ptr(dy), g, L, ptr(peak), ptr(pcm), stream()) == OK
        ph, pk = host(pcm), host(peak).view(np.uint32)
        tag = 'pack_pcm16 L=%d groups %s' % (L, '/'.join(kinds))
        K.check_guard(ph[g * L * 2:], 12345, tag + ' pcm guard')
        K.check_guard(pk[g:], 0x7FC12345, tag + ' peak guard')
        assert np.array_equal(host(dy).view(np.uint32), y.view(np.uint32)), 'y was written to'
        got = ph[:g * L * 2].reshape(g, L, 2)
        for i, k in enumerate(kinds):
            K.check_bits(got[i], want[i], '%s, group %d (%s)' % (tag, i, k))
            if k in ('nan', 'inf'):
                assert pk[i] >= 0x7F800000, (tag, i, hex(pk[i]))
                assert not np.isfinite(y[i]).all()
            else:
                assert pk[i] == np.max(np.abs(y[i])).view(np.uint32) == bits[i], (tag, i, hex(pk[i]))
        # what the kinds are for
        for i, k in enumerate(kinds):
            peakv = np.max(np.abs(y[i])) if np.isfinite(y[i]).all() else None
            if k == 'peak1':
                assert peakv == 1 and np.abs(got[i]).max() == int(np.float32(0.99) * np.float32(32768))
            if k == 'below1':
                assert peakv < 1 and got[i].max() == 32767
            if k == 'loud40':
                assert peakv >= 40 and np.abs(got[i]).max() == int(np.float32(0.99) * np.float32(32768))
            if k == 'nan' and L >= 4:
                assert got[i][0, 0] == 0 and got[i][2, 1] == -32768 and got[i][3, 1] == 32767 and got[i][1, 0] == 32767
            if k == 'inf' and L >= 4:
                assert got[i][0, 1] == 32767 and got[i][3, 0] == -32768 and got[i][1, 1] == -32768 and got[i][2, 0] == 32767


# ---- any n_fft: the DFT as a GEMM ----------------------------------------------------------------------------------------------------
def dft_tables(N, Fp, inverse=False):
    from gcc_nmf_amd import librosaSTFT as Ls
    w = np.hanning(N) * (2.0 / 3 if inverse else 1.0)
    return (Ls.idft_basis(w, N, Fp) if inverse else Ls.dft_basis(w, N, Fp))


# (n_fft, hop, T, nsig); T around the GEMM's 64-column tiles; hop > n_fft at 30 / 40
DFT_FORWARD_CELLS = [(30, 7, 65, 3), (30, 40, 64, 1), (375, 125, 63, 2), (400, 100, 2, 2), (400, 100, 1, 1), (1000, 250, 64, 3), (1536, 384, 65, 1),
                     (1000, 300, 1, 2)]


@pytest.mark.parametrize('N,hop,T,nsig', DFT_FORWARD_CELLS, ids=['n%d-hop%d-T%d-s%d' % c for c in DFT_FORWARD_CELLS])
def test_stft_dft_against_float64(lib, N, hop, T, nsig):
    F, n = N // 2 + 1, (T - 1) * hop + N
    Fp, Np, Tp = pitches(F, T)
    basis = dft_tables(N, Fp)
    rng = np.random.RandomState(N + T)
    x = (rng.standard_normal((nsig, n)) * np.repeat(K.amplitudes(-(-n // hop)), hop)[:n]).astype(np.float32)
    if T >= 3:
        x[:, (T // 2) * hop:(T // 2) * hop + N] = 0
    stride = n + 11
    buf = np.full((nsig - 1) * stride + n, GARBAGE, np.float32)
    for s in range(nsig):
        buf[s * stride:s * stride + n] = x[s]
    dx, dbasis = dev(buf), dev(basis)
    nws = lib.gccnmf_dft_workspace_floats(N, T, nsig)
    assert nws > 0
    runs = []
    for fill in (NAN, GARBAGE):
        ws = torch.full((nws + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
        ws[:nws] = fill
        X = torch.zeros((nsig, Fp, Tp, 2), dtype=torch.float32, device='cuda')
        X[:, :F, :T] = NAN
        assert lib.gccnmf_stft_dft(ptr(dx), stride, n, N, hop, T, nsig, ptr(dbasis), ptr(ws), ptr(X), stream()) == OK
        K.check_guard(host(ws)[nws:], SENTINEL, 'workspace guard')
        runs.append(host(X))
    K.check_bits(runs[1], runs[0], 'stft_dft over another workspace')
    Xh = runs[0]
    pad = Xh.copy()
    pad[:, :F, :T] = 0
    C.check_zero(pad, 'stft_dft X padding')
    b64 = basis[:N].astype(np.float64)
    fr = K.frames_of(x.astype(np.float64), N, hop, T)                    # (nsig, T, N)
    for s in range(nsig):
        for part, col in ((0, slice(0, F)), (1, slice(Fp, Fp + F))):
            ref = np.dot(b64[:, col].T, fr[s].T)                         # (F, T)
            absprod = np.dot(np.abs(b64[:, col]).T, np.abs(fr[s]).T)
            C.check_gemm_like(Xh[s, :F, :T, part], ref, absprod, N, what='stft_dft n_fft=%d signal %d %s' % (N, s, 're' if part == 0 else 'im'))
            with np.errstate(divide='ignore', invalid='ignore'):
                share = np.nanmax(np.where(absprod > 0, np.abs(Xh[s, :F, :T, part] - ref) / C.gemm_bound(absprod, N), 0.0))
            print('stft_dft n_fft=%d hop=%d T=%d signal %d part %d: worst share of the bound %.4f' % (N, hop, T, s, part, share))
        if T >= 3:
            C.check_zero(Xh[s, :F, T // 2], 'stft_dft X of the silent frame')
        # and it IS the transform: conj(rfft(w x)) to the table's own float32 rounding
        w = np.hanning(N)
        true = np.conj(np.fft.rfft(w * fr[s], axis=-1)).T
        got = Xh[s, :F, :T, 0] + 1j * Xh[s, :F, :T, 1]
        C.check_gemm_like(got, true, np.sqrt(2) * np.dot(np.abs(w)[None, :], np.abs(fr[s]).T) * np.ones((F, 1)), N, what='stft_dft against rfft')


DFT_INVERSE_CELLS = [(30, 7, 65, 3, 1), (30, 40, 64, 1, 0), (400, 100, 2, 2, 1), (400, 100, 1, 1, 0), (1000, 250, 64, 3, 0), (1536, 384, 65, 1, 1),
                     (1000, 300, 63, 2, 1)]


@pytest.mark.parametrize('N,hop,T,nsig,center', DFT_INVERSE_CELLS, ids=['n%d-hop%d-T%d-s%d-c%d' % c for c in DFT_INVERSE_CELLS])
def test_istft_dft_against_float64(lib, N, hop, T, nsig, center):
    F, gain = N // 2 + 1, 1.7
    Fp, Np, Tp = pitches(F, T)
    ibasis = dft_tables(N, Fp, inverse=True)
    trim, L = K.istft_length(N, hop, T, center)
    S = K.stage_spectra(nsig, F, T, N + T)[0]
    img = np.zeros((nsig, Fp, Tp, 2), np.float32)
    img[:, :F, :T, 0], img[:, :F, :T, 1] = S.real, S.imag
    dS, dib = dev(img), dev(ibasis)
    nws = lib.gccnmf_dft_workspace_floats(N, T, nsig)
    off = nsig * 2 * Fp * Tp                                             # planes | frames
    assert nws >= off + nsig * T * N
    runs = []
    for fill in (NAN, GARBAGE):
        ws = torch.full((nws + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
        ws[:nws] = fill
        y = torch.full((nsig * L + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
        y[:nsig * L] = NAN
        assert lib.gccnmf_istft_dft(ptr(dS), nsig, N, hop, T, ptr(dib), gain, center, ptr(ws), ptr(y), stream()) == OK
        wh, yh = host(ws), host(y)
        K.check_guard(wh[nws:], SENTINEL, 'workspace guard')
        K.check_guard(yh[nsig * L:], SENTINEL, 'y guard')
        runs.append((wh[off:off + nsig * T * N].reshape(nsig, T, N), yh[:nsig * L].reshape(nsig, L)))
    K.check_bits(runs[1][1], runs[0][1], 'istft_dft over another workspace')
    frames, y = runs[0]
    ib64 = ibasis.astype(np.float64)
    for s in range(nsig):
        re, im = img[s, :F, :T, 0].astype(np.float64).T, img[s, :F, :T, 1].astype(np.float64).T           # (T, F)
        ref = np.dot(re, ib64[:F, :N]) + np.dot(im, ib64[Fp:Fp + F, :N])
        absprod = np.dot(np.abs(re), np.abs(ib64[:F, :N])) + np.dot(np.abs(im), np.abs(ib64[Fp:Fp + F, :N]))
        C.check_gemm_like(frames[s], ref, absprod, 2 * Fp, what='istft_dft n_fft=%d frames of signal %d' % (N, s))
        with np.errstate(divide='ignore', invalid='ignore'):
            share = np.nanmax(np.where(absprod > 0, np.abs(frames[s] - ref) / C.gemm_bound(absprod, 2 * Fp), 0.0))
        print('istft_dft n_fft=%d hop=%d T=%d signal %d: worst share of the bound %.4f' % (N, hop, T, s, share))
    C.check_written(y, 'istft_dft y')
    K.check_bits(y, K.ola32(frames, N, hop, trim, L, gain), 'istft_dft y against the float32 overlap-add of its frames')
