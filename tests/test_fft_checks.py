"""CPU: the comparison rules of the STFT / iSTFT / PCM stage tests (tests/fft_checks.py) are sound and sensitive.  A float32 restatement
of the kernels' arithmetic stays inside every bar on every input the GPU tests use (so an honest implementation cannot flake), and each
typical kernel mistake, applied to that restatement, falls outside its rule -- so the GPU tests that use these rules are not vacuous."""
import numpy as np
import pytest

import fft_checks as K

SIZES = (64, 256, 1024, 4096)
T = 6


def _inputs(N, hop):
    """name -> (2, n) float32: the inputs named by the stage tests' design."""
    n = (T - 1) * hop + N
    rng = np.random.RandomState(N)
    noise = rng.standard_normal((2, n)).astype(np.float32)
    quiet_right = noise.copy()
    quiet_right[1] *= np.float32(1e-4)
    quiet_frame = noise.copy()
    quiet_frame[:, 2 * hop:2 * hop + N] *= np.float32(1e-3)         # (with overlap: the frame and the overlapped part of its neighbours)
    return {'white noise': noise, 'all ones': np.ones((2, n), np.float32),
            'random signs': np.sign(rng.standard_normal((2, n))).astype(np.float32),
            'right channel 1e-4 of the left': quiet_right, 'one frame 1e-3 of its neighbours': quiet_frame,
            'stage signal': K.stage_signal(N, hop, T, N + 1)[0], 'stage signal, left 1e3 louder': K.stage_signal(N, hop, T, N + 2, 1e-3)[0]}


@pytest.mark.parametrize('N', SIZES)
def test_float32_restatement_stays_inside_every_bar(N):
    """Forward and inverse, every element of every frame, every input; prints the worst share (an honest float32 FFT uses a few
    hundredths of the worst-case bar)."""
    w = np.hanning(N).astype(np.float32)
    worst_f = worst_i = 0.0
    for hop in (N // 4, N):
        for name, x in _inputs(N, hop).items():
            ref, sumabs = K.stft64(x, w, N, hop, T)
            got = K.stft32(x, w, N, hop, T)
            assert got.shape == ref.shape == (2, N // 2 + 1, T)
            for c in range(2):
                worst_f = max(worst_f, K.check_bar(got[c], ref[c], K.stft_bar(sumabs, N), 'stft N=%d hop=%d %s ch %d' % (N, hop, name, c)))
            # the inverse of that spectrogram (a quiet signal beside a loud one included) and of the stage tests' random spectra
            for Sa, Sb in ((got[0], got[1]), tuple(K.stage_spectra(2, N // 2 + 1, T, N + hop)[0])):
                fr64, sa = K.istft_frames64(Sa, Sb, w, N)
                fr32 = K.istft_frames32(Sa, Sb, w, N)
                assert fr32.shape == fr64.shape == (2, T, N)
                for c in range(2):
                    worst_i = max(worst_i, K.check_bar(fr32[c], fr64[c], K.frames_bar(sa, w, N), 'istft N=%d %s sig %d' % (N, name, c)))
    print('N = %d: worst share forward %.4f, inverse %.4f' % (N, worst_f, worst_i))
    assert 0 < worst_f < 0.5 and 0 < worst_i < 0.5          # sound with room to spare -- and the bar is of the error's own order, not 1e3 above


def test_a_frame_silent_in_both_channels_is_exactly_zero_and_a_silent_channel_meets_the_bar():
    N, hop = 256, 64
    w = np.hanning(N).astype(np.float32)
    x, ts = K.stage_signal(N, hop, 7, 3)
    X = K.stft32(x, w, N, hop, 7)
    ref, sumabs = K.stft64(x, w, N, hop, 7)
    assert ts == 3 and sumabs[ts] == 0 and not X[:, :, ts].any() and X[:, :, ts - 1].all()
    K.check_bar(X[0], ref[0], K.stft_bar(sumabs, N))
    # one silent channel: the rule asks only for the bar (which holds the loud channel's magnitude), not for exact zeros -- the split is
    # (Z[k] -+ conj(Z[N-k])) / 2 of rounded values.  (This restatement happens to give exact zeros: with a zero imaginary input its
    # butterflies keep Z[N-k] the bitwise conjugate of Z[k].  A routine that orders them otherwise need not.)
    x[1] = 0
    X = K.stft32(x, w, N, hop, 7)
    ref, sumabs = K.stft64(x, w, N, hop, 7)
    assert not ref[1].any() and sumabs[ts - 1] > 0
    K.check_bar(X[1], ref[1], K.stft_bar(sumabs, N))
    residue = X[1].copy()
    residue[5, 2] = np.float32(1e-7) * np.abs(X[0, 5, 2])      # a residue of the loud channel's rounding size passes ...
    K.check_bar(residue, ref[1], K.stft_bar(sumabs, N))
    residue[5, 2] = np.float32(1e-3) * np.abs(X[0]).max()      # ... a leak of the loud channel does not
    with pytest.raises(AssertionError):
        K.check_bar(residue, ref[1], K.stft_bar(sumabs, N))


def _forward_case(N=256, hop=64, right_scale=1.0):
    w = np.hanning(N).astype(np.float32)
    x, _ = K.stage_signal(N, hop, T, 11, right_scale)
    ref, sumabs = K.stft64(x, w, N, hop, T)
    return x, w, N, hop, ref, K.stft_bar(sumabs, N)


def _forward_mutations():
    def nyquist_bin_zeroed(x, w, N, hop):
        X = K.stft32(x, w, N, hop, T)
        X[:, -1] = 0
        return X

    def nyquist_bin_dropped(x, w, N, hop):
        X = K.stft32(x, w, N, hop, T)
        X[:, -1] = X[:, -2]
        return X

    def bins_k_and_n_minus_k_exchanged(x, w, N, hop):
        return np.conj(K.stft32(x, w, N, hop, T))               # the missing conjugate

    def neighbouring_frames_exchanged(x, w, N, hop):
        X = K.stft32(x, w, N, hop, T)
        X[:, :, [3, 4]] = X[:, :, [4, 3]]
        return X

    def channels_exchanged(x, w, N, hop):
        return K.stft32(x, w, N, hop, T)[::-1].copy()

    def window_shifted_by_one(x, w, N, hop):
        return K.stft32(x, np.roll(w, 1), N, hop, T)

    def frame_started_one_sample_late(x, w, N, hop):
        X = K.stft32(x, w, N, hop, T)
        late = np.concatenate([x[:, 1:], np.zeros((2, 1), np.float32)], axis=1)
        X[:, :, 4] = K.stft32(late, w, N, hop, T)[:, :, 4]
        return X

    def a_frame_not_written(x, w, N, hop):
        X = K.stft32(x, w, N, hop, T)
        X[:, :, T - 1] = np.nan
        return X

    def leak_of_the_loud_neighbour(x, w, N, hop):
        X = K.stft32(x, w, N, hop, T)
        loud, quiet = int(np.argmax(np.abs(X[0]).sum(0))), int(np.argmin(np.abs(X[0]).sum(0) + 1e9 * (np.abs(X[0]).sum(0) == 0)))
        X[:, :, quiet] += np.float32(1e-4) * X[:, :, loud]
        return X
    return [nyquist_bin_zeroed, nyquist_bin_dropped, bins_k_and_n_minus_k_exchanged, neighbouring_frames_exchanged, channels_exchanged,
            window_shifted_by_one, frame_started_one_sample_late, a_frame_not_written, leak_of_the_loud_neighbour]


@pytest.mark.parametrize('right_scale', [1.0, 1e-3])
@pytest.mark.parametrize('mutate', _forward_mutations(), ids=lambda f: f.__name__)
def test_forward_bar_catches(mutate, right_scale):
    x, w, N, hop, ref, bar = _forward_case(right_scale=right_scale)
    good = K.stft32(x, w, N, hop, T)
    for c in range(2):
        K.check_bar(good[c], ref[c], bar)
    got = mutate(x, w, N, hop)
    with pytest.raises(AssertionError):
        for c in range(2):
            K.check_bar(got[c], ref[c], bar)


def _inverse_case(N=256, hop=64):
    w = (np.hanning(N) * 2 / 3).astype(np.float32)
    S, _ = K.stage_spectra(2, N // 2 + 1, T, 5)
    fr64, sumabs = K.istft_frames64(S[0], S[1], w, N)
    return S, w, N, hop, fr64, K.frames_bar(sumabs, w, N)


def _inverse_mutations():
    def edge_imaginary_parts_kept(S, w, N):
        return K.istft_frames32(S[0], S[1], w, N, keep_edge_imag=True)

    def nyquist_imaginary_part_kept(S, w, N):
        S2 = S.copy()
        S2[:, 0] = S2[:, 0].real
        return K.istft_frames32(S2[0], S2[1], w, N, keep_edge_imag=True)

    def dc_imaginary_part_kept(S, w, N):
        S2 = S.copy()
        S2[:, -1] = S2[:, -1].real
        return K.istft_frames32(S2[0], S2[1], w, N, keep_edge_imag=True)

    def stored_conjugate_not_undone(S, w, N):
        return K.istft_frames32(np.conj(S[0]), np.conj(S[1]), w, N)

    def nyquist_bin_dropped(S, w, N):
        S2 = S.copy()
        S2[:, -1] = 0
        return K.istft_frames32(S2[0], S2[1], w, N)

    def signals_of_the_pair_exchanged(S, w, N):
        return K.istft_frames32(S[1], S[0], w, N)

    def neighbouring_frames_exchanged(S, w, N):
        fr = K.istft_frames32(S[0], S[1], w, N)
        fr[:, [1, 2]] = fr[:, [2, 1]]
        return fr

    def window_shifted_by_one(S, w, N):
        return K.istft_frames32(S[0], S[1], np.roll(w, 1), N)
    return [edge_imaginary_parts_kept, nyquist_imaginary_part_kept, dc_imaginary_part_kept, stored_conjugate_not_undone, nyquist_bin_dropped,
            signals_of_the_pair_exchanged, neighbouring_frames_exchanged, window_shifted_by_one]


@pytest.mark.parametrize('mutate', _inverse_mutations(), ids=lambda f: f.__name__)
def test_inverse_bar_catches(mutate):
    S, w, N, hop, fr64, bar = _inverse_case()
    good = K.istft_frames32(S[0], S[1], w, N)
    for c in range(2):
        K.check_bar(good[c], fr64[c], bar)
    got = mutate(S, w, N)
    with pytest.raises(AssertionError):
        for c in range(2):
            K.check_bar(got[c], fr64[c], bar)


def test_overlap_add_rule_is_exact_and_catches_a_missing_frame_and_a_wrong_trim():
    S, w, N, hop, fr64, bar = _inverse_case()
    fr = K.istft_frames32(S[0], S[1], w, N)
    gain = 1.7
    gain32 = float(np.float32(gain))
    for center in (0, 1):
        trim, L = K.istft_length(N, hop, T, center)
        y = K.ola32(fr, N, hop, trim, L, gain)
        assert y.shape == (2, L) and y.dtype == np.float32
        # the restatement is the float64 overlap-add to within the additions' roundings: ceil(N / hop) additions and the gain per sample
        ref = np.zeros((2, N + hop * (T - 1)))
        mag = np.zeros_like(ref)
        for t in range(T):
            ref[:, t * hop:t * hop + N] += fr[:, t].astype(np.float64)
            mag[:, t * hop:t * hop + N] += np.abs(fr[:, t].astype(np.float64))
        assert np.all(np.abs(y.astype(np.float64) - gain32 * ref[:, trim:trim + L]) <= (-(-N // hop) + 1) * K.U32 * gain32 * mag[:, trim:trim + L])
        K.check_bits(y, y.copy())
        for skip in (0, 2, T - 1):                                                # one frame left out (frame 3 is the silent one)
            with pytest.raises(AssertionError):
                K.check_bits(K.ola32(fr, N, hop, trim, L, gain, skip=skip), y)
        for off in (-1, 1):                                                       # trimmed by n_fft / 2 -+ 1 (center = 0: by 1; a short result is caught too)
            if trim + off >= 0:
                with pytest.raises(AssertionError):
                    K.check_bits(K.ola32(fr, N, hop, trim + off, L, gain), y)
        with pytest.raises(AssertionError):                                      # frames added in descending order: other roundings
            K.check_bits(_descending_ola(fr, N, hop, trim, L, gain), y)
        with pytest.raises(AssertionError):                                      # the gain applied per frame instead of once
            K.check_bits(K.ola32(fr * np.float32(gain), N, hop, trim, L, 1.0), y)


def _descending_ola(frames, N, hop, first, L, gain):
    Tn = frames.shape[-2]
    acc = np.zeros(frames.shape[:-2] + (N + hop * (Tn - 1),), np.float32)
    for t in range(Tn - 1, -1, -1):
        acc[..., t * hop:t * hop + N] = acc[..., t * hop:t * hop + N] + frames[..., t, :]
    return acc[..., first:first + L] * np.float32(gain)


def test_overlap_add_leaves_zeros_between_frames_further_apart_than_their_length():
    fr = np.ones((1, 6, 256), np.float32)
    y = K.ola32(fr, 256, 300, 0, 256 + 300 * 5, 2.0)
    assert np.all(y[0, 256:300] == 0) and np.all(y[0, 1156:1200] == 0) and np.all(y[0, 1200:1456] == 2)


def test_fused_hand_out_covers_every_sample_once_unless_hop_exceeds_n_fft():
    """The hand-out rules of istft_fused_kernel restated (fft_checks.fused_write_counts): with hop <= n_fft every output sample is written
    exactly once, at every frame count around the workgroup's 4 x 8 frames.  With hop > n_fft the hop - n_fft samples behind every fourth
    frame of a workgroup are written by nobody -- at n_fft = 256, hop = 300, T = 6, center = 0: samples 1156 .. 1199 -- which is why
    gccnmf_istft_ola answers GCCNMF_ERR_UNSUPPORTED for the fused form there."""
    for N, hops in ((64, (8, 16, 20, 63, 64)), (256, (32, 64, 100, 255, 256)), (1024, (128, 256, 300, 341))):
        for hop in hops:
            for Tn in (1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 97):
                for center in (0, 1):
                    if K.istft_length(N, hop, Tn, center)[1] < 1:
                        continue
                    count = K.fused_write_counts(N, hop, Tn, center)
                    assert np.all(count == 1), (N, hop, Tn, center, np.flatnonzero(count != 1)[:4])
    count = K.fused_write_counts(256, 300, 6, 0)
    assert np.flatnonzero(count == 0).tolist() == list(range(1156, 1200)) and count.max() == 1
    for N, hop, Tn, center in ((256, 300, 33, 1), (64, 65, 5, 0), (256, 257, 9, 1)):
        count = K.fused_write_counts(N, hop, Tn, center)
        assert (count == 0).sum() > 0 and count.max() == 1, (N, hop, Tn, center)


def _pcm_groups(L=300):
    rng = np.random.RandomState(L)
    one, below = np.float32(1), np.nextafter(np.float32(1), np.float32(0))
    quiet = rng.uniform(-0.5, 0.5, (2, L)).astype(np.float32)
    peak1, below1, loud = quiet.copy(), quiet.copy(), (quiet * 80).astype(np.float32)
    peak1[0, L // 2] = one
    below1[1, L // 3] = -below
    k = rng.randint(-32767, 32767, (2, L)).astype(np.float32) / np.float32(32768)
    steps = np.where(rng.rand(2, L) < 0.5, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-2))).astype(np.float32)
    steps[0, :3] = k[0, :3]
    return dict(quiet=quiet, peak1=peak1, below1=below1, loud=loud, steps=steps)


def test_pcm_restatement_is_the_host_wavwrite_and_catches_rounding_and_an_early_rescale():
    from gcc_nmf_amd import wavfile as Wf
    g = _pcm_groups()
    names = list(g)
    y = np.stack([g[n] for n in names])
    pcm, bits = K.pack_pcm16_32(y)
    for i, n in enumerate(names):
        x = g[n]
        peak = np.max(np.abs(x))
        assert bits[i] == peak.view(np.uint32), n
        scaled = (x / peak * np.float32(0.99)).astype(np.float32) if peak >= 1 else x       # wavfile.wavwrite
        assert scaled.dtype == np.float32
        K.check_bits(pcm[i], Wf.float2pcm(scaled).T.copy(), n)
    assert np.abs(pcm[names.index('loud')]).max() == int(0.99 * 32768) and np.abs(pcm[names.index('peak1')]).max() == int(np.float32(0.99) * 32768)
    assert pcm[names.index('below1')].min() == -32767
    with pytest.raises(AssertionError):
        K.check_bits(K.pack_pcm16_32(y, round_instead=True)[0], pcm, 'rounding')
    for n in ('quiet', 'steps', 'loud'):
        i = names.index(n)
        with pytest.raises(AssertionError):
            K.check_bits(K.pack_pcm16_32(y[i:i + 1], round_instead=True)[0], pcm[i:i + 1], n)
    i = names.index('below1')                          # a peak one ulp below 1 is NOT rescaled
    with pytest.raises(AssertionError):
        K.check_bits(K.pack_pcm16_32(y[i:i + 1], rescale_from=np.nextafter(np.float32(1), np.float32(0)))[0], pcm[i:i + 1])
    # edges and the non-finite policy
    e = np.zeros((3, 2, 4), np.float32)
    e[0, 0] = [-1.0, np.nextafter(np.float32(1), np.float32(0)), np.nan, 0.25]
    e[1, 0] = [np.inf, -np.inf, 0.5, -1.0]
    e[2, 0] = [40.0, -20.0, 1.0, 0.0]
    pcm, bits = K.pack_pcm16_32(e)
    assert pcm[0, :, 0].tolist() == [-32768, 32767, 0, 8192] and bits[0] >= 0x7F800000
    assert pcm[1, :, 0].tolist() == [32767, -32768, 16384, -32768] and bits[1] == 0x7F800000
    assert pcm[2, :, 0].tolist() == [int(0.99 * 32768), -int(0.99 * 16384), int(np.float32(1) / np.float32(40) * np.float32(0.99) * np.float32(32768)), 0]
    assert np.array_equal(K.pcm2float32(np.array([-32768, 32767, 0, 1], np.int16)), np.array([-1, 32767 / 32768, 0, 1 / 32768], np.float32))
    assert np.array_equal(K.pcm2float32(np.arange(-32768, 32768).astype(np.int16)), Wf.pcm2float(np.arange(-32768, 32768).astype(np.int16)))


def test_modulus_and_coherence_rules():
    rng = np.random.RandomState(4)
    X = (rng.standard_normal((2, 33, 9)) + 1j * rng.standard_normal((2, 33, 9))).astype(np.complex64)
    X[:, :, 4] = 0
    X[1, 7, 2] = 0
    V = np.abs(X).astype(np.float32)
    K.check_modulus(V[0], X[0])
    with np.errstate(invalid='ignore', divide='ignore'):
        num = X[0] * np.conj(X[1])
        cc = np.where((V[0] > 0) & (V[1] > 0), num / V[0] / V[1], 0).astype(np.complex64)
    K.check_coherence(cc, X[0], X[1], V[0], V[1])
    bad = V[0].copy()
    bad[3, 3] *= np.float32(1 + 1e-6)
    with pytest.raises(AssertionError):
        K.check_modulus(bad, X[0])
    with pytest.raises(AssertionError):
        K.check_modulus(V[1], X[0])                       # the other channel's modulus
    for mutate in (np.conj, lambda c: c * np.float32(1 + 2e-6), lambda c: np.where(np.arange(9)[None, :] == 4, np.nan, c),
                   lambda c: np.where(np.arange(9)[None, :] == 4, 1e-30, c)):
        with pytest.raises(AssertionError):
            K.check_coherence(mutate(cc).astype(np.complex64), X[0], X[1], V[0], V[1])


def test_guard_and_bits_rules():
    K.check_guard(np.full(64, -7.0, np.float32), -7.0)
    with pytest.raises(AssertionError):
        K.check_guard(np.array([-7.0, 0.0, -7.0], np.float32), -7.0)
    a = np.array([0.0, 1.0, np.nan], np.float32)
    K.check_bits(a, a.copy())
    with pytest.raises(AssertionError):
        K.check_bits(np.array([-0.0, 1.0, np.nan], np.float32), a)
