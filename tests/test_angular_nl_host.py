"""GCC-NONLIN localisation (gccPHATNLEnabled / gccPHATNLAlpha) without a device: the NumPy restatement against closed forms and on the
six committed mixtures, the argument checks of the engines / named functions / real-time processor, the packed form of the C call, and
the margins the streaming GPU test relies on."""
import ctypes
import inspect
import warnings

import numpy as np
import pytest

import angular_nl_restatement as NL
from oracle import gccnmf_oracle as O
from oracle import rt_oracle as R

BAD_ALPHAS = (0, 0.0, -1, -0.5, float('nan'), float('inf'), -float('inf'), '2', None, [2.0], True, 1e-45)


def test_restatement_closed_forms():
    F, D, T = 65, 33, 4
    freqs, tdoas = O.getFrequenciesInHz(16000, F), O.getTDOAsInSeconds(1.0, D)
    for i in (0, 7, D - 1):
        C = np.repeat(np.exp(2j * np.pi * freqs * tdoas[i])[:, None], T, axis=1)          # re = 1 at tau_i for every f
        for alpha in (0.5, 2.0, 8.0):
            A = NL.angular_spectrogram_nl(C, freqs, tdoas, alpha)
            assert A.shape == (D, T) and np.all(A >= 0) and np.all(A <= F)
            assert np.all(np.abs(A[i] - F) < 1e-5 * alpha), (i, alpha, A[i])              # sqrt(1e-16) alpha per bin at most
            assert np.all(np.argmax(A, axis=0) == i)
        # alpha -> infinity keeps only exact matches: f = 0 matches every tau, the other bins only tau_i (1e6: re = 1 - 1e-16 in float64
        # still counts, 0.99; the nearest miss, 1 - re = 1e-2 at the first bin of the neighbouring tau, does not)
        A = NL.angular_spectrogram_nl(C, freqs, tdoas, 1e6)
        others = np.delete(A, i, axis=0)
        assert np.all(A[i] > 0.95 * F) and np.all(np.abs(others - 1) < 1e-6), (i, A[i], others.max())
    # max(0, .) is part of the definition: re above 1 by a rounding error gives phi = 1, never NaN; NaN terms stay NaN
    assert NL.phi(np.float64(1 + 1e-12), 2.0) == 1.0 and NL.phi(np.float32(1.0000001), 2.0) == 1.0
    assert np.isnan(NL.phi(np.float64('nan'), 2.0))
    assert abs(NL.phi(np.float64(0.0), 2.0) - (1 - np.tanh(2.0))) < 1e-15                 # a zero coherence bin: the constant 1 - tanh(alpha)
    # 1 - tanh(y) = 2 / (1 + e^{2y}), the device's form
    y = np.linspace(0, 12, 1000)
    assert np.abs((1 - np.tanh(y)) - 2 / (1 + np.exp(2 * y))).max() < 1e-15
    # streaming: nanmean skips NaN bins and does not count them; a frame of NaN only is NaN
    Cs = np.exp(2j * np.pi * freqs * tdoas[5])[:, None].repeat(2, axis=1)
    cosT, sinT = NL.tables(freqs, tdoas)
    g = NL.gccphat_nl(Cs, cosT, sinT, 2.0)
    Cn = Cs.copy()
    Cn[3:9, 0] = np.nan
    Cn[:, 1] = np.nan
    gn = NL.gccphat_nl(Cn, cosT, sinT, 2.0)
    keep = np.r_[0:3, 9:F]
    want = NL.phi((Cs[keep, :1, None] * np.exp(-2j * np.pi * np.outer(freqs, tdoas))[keep, None, :]).real, 2.0).mean(axis=0)[0]
    # (at tau_5 itself re = 1 - O(1e-16) in either evaluation, and the square root makes 1e-8 of that)
    assert np.abs(gn[:, 0] - want).max() < 1e-7 and np.isnan(gn[:, 1]).all() and np.all((g >= 0) & (g <= 1))
    assert abs(g[5, 0] - 1) < 1e-6


def test_restatement_pure_delay_mixture_peaks_where_phat_does():
    """synthetic file 0 (delays +27, +3, -20 samples) localises at [27, 59, 91]."""
    from gcc_nmf_amd.synthetic import synthetic_mixture
    X = O.computeComplexMixtureSpectrogram(synthetic_mixture(0, numSamples=48000), 1024, 256, np.hanning)
    C = NL.offline_coherence(X)
    freqs, tdoas = O.getFrequenciesInHz(16000, 513), O.getTDOAsInSeconds(1.0, 128)
    idx, m, A = NL.localise(C, freqs, tdoas, 2.0, 3)
    assert idx == [27, 59, 91] and np.all(A >= 0) and np.all(A <= 513)
    assert idx == O.estimateTargetTDOAIndexesFromAngularSpectrum(np.mean(O.getAngularSpectrogram(C, freqs, 1.0, 128), axis=-1), 1.0, 128, 3)


@pytest.mark.parametrize('name', list(NL.MIXTURES))
def test_restatement_on_the_committed_mixtures(name):
    """alpha = 2, n_fft 1024, hop 256, D = 128, d = 1 m: exactly the index lists the feature was specified with, in float64 and in the
    float32 evaluation; the margins that make exact indexes a safe demand of the device."""
    S, want, phat = NL.MIXTURES[name]
    C, freqs, sr = NL.mixture_coherence(name)
    tdoas = O.getTDOAsInSeconds(1.0, 128)
    barA, barM, A64, eA, eM = NL.measured_bar(C, freqs, tdoas, 2.0)
    m = A64.mean(axis=-1)
    assert NL.pick_peaks(m, S) == want
    A32 = NL.angular_spectrogram_nl(C, freqs, tdoas, 2.0, np.float32)
    assert NL.pick_peaks(A32.astype(np.float64).mean(axis=-1), S) == want
    assert O.estimateTargetTDOAIndexesFromAngularSpectrum(np.mean(O.getAngularSpectrogram(C, freqs, 1.0, 128), axis=-1), 1.0, 128, S) == phat
    chosen, neighbour, runner_up = NL.peak_margins(m, S)
    print('%s: float32 error %.3g on A in [%.1f, %.1f], %.3g on the mean; margins %.3g / %.3g' % (name, eA, A64.min(), A64.max(), eM,
                                                                                                neighbour, runner_up))
    assert chosen == want and neighbour > 3e-3 and runner_up > 3.0 and 10 * barM < neighbour        # ten bars of room at the narrowest peak
    assert 0 < eA < 5e-3 and np.all(A64 >= 0) and np.all(A64 <= 513)


def test_alpha_is_validated_without_a_device():
    from gcc_nmf_amd import _hip, engine, realtime as rt
    from gcc_nmf_amd import gccNMFFunctions as G
    assert engine.check_gcc_phat_nl(False, 2.0) == (False, 2.0) and engine.check_gcc_phat_nl(1, np.float32(0.5)) == (True, 0.5)
    assert engine.check_gcc_phat_nl(True, 3) == (True, 3.0)
    for bad in BAD_ALPHAS:
        for enabled in (False, True):
            with pytest.raises(ValueError):
                engine.check_gcc_phat_nl(enabled, bad)
        with pytest.raises(ValueError):                      # before the engines look for a device or allocate anything
            engine.GCCNMFEngine(16000, gccPHATNLEnabled=True, gccPHATNLAlpha=bad)
        with pytest.raises(ValueError):
            engine.GCCNMFEngine(lengths=[16000, 20000], gccPHATNLEnabled=True, gccPHATNLAlpha=bad)
        with pytest.raises(ValueError):
            G.getAngularSpectrogram(np.ones((5, 3), np.complex64), np.linspace(0, 8000, 5), 1.0, 8, True, bad)
        with pytest.raises(ValueError):
            G.getTargetTDOAEstimates(np.ones((2, 5, 3), np.complex64), 16000, 1.0, 8, 1, gccPHATNLEnabled=True, gccPHATNLAlpha=bad)
        W = np.ones((513, 8), np.float32)
        with pytest.raises(ValueError):                      # the constructor checks before it looks for a device
            rt.GCCNMFProcessor(16000, 1024, 1, {'P': {8: W}}, 'P', 8, 0, 0.1, True, 6, gccPHATNLAlpha=bad)
        p = object.__new__(rt.GCCNMFProcessor)               # attributes set later are checked by reset() through the same helper
        p.gccPHATNLEnabled, p.gccPHATNLAlpha = True, bad
        with pytest.raises(ValueError):
            p._gcc_phat_nl()
    p = object.__new__(rt.GCCNMFProcessor)
    p.gccPHATNLEnabled, p.gccPHATNLAlpha = False, 2.0
    assert p._gcc_phat_nl() == 0.0                           # word 6 of the target row: 0 = PHAT
    p.gccPHATNLEnabled = True
    assert p._gcc_phat_nl() == 2.0 and p._gcc_phat_nl().dtype == np.float32
    # the bank's per-stream setter checks before it touches the device
    bk = object.__new__(rt.StreamingGCCNMFBank)
    bk.numStreams, bk.device = 2, 'cpu'
    with pytest.raises(ValueError):
        rt.StreamingGCCNMFBank.setGCCPHATNL.__wrapped__(bk, 0, True, -1.0)
    with pytest.raises(IndexError):
        rt.StreamingGCCNMFBank.setGCCPHATNL.__wrapped__(bk, 2, True, 2.0)


def test_reference_named_functions_keep_their_positional_signatures():
    from gcc_nmf_amd import gccNMFFunctions as G
    from gcc_nmf_amd import engine, realtime as rt
    a = inspect.signature(G.getAngularSpectrogram).parameters
    assert list(a) == ['spectralCoherenceV', 'frequenciesInHz', 'microphoneSeparationInMetres', 'numTDOAs', 'gccPHATNLEnabled',
                       'gccPHATNLAlpha']
    t = inspect.signature(G.getTargetTDOAEstimates).parameters
    assert list(t)[:5] == ['complexMixtureSpectrogram', 'sampleRate', 'microphoneSeparationInMetres', 'numTDOAs', 'numSources']
    assert list(t)[5:] == ['gccPHATNLEnabled', 'gccPHATNLAlpha']
    for params in (a, t, inspect.signature(engine.GCCNMFEngine.__init__).parameters,
                   inspect.signature(engine.RaggedGCCNMFEngine.__init__).parameters,
                   inspect.signature(rt.GCCNMFProcessor.__init__).parameters):
        assert params['gccPHATNLEnabled'].default is False and params['gccPHATNLAlpha'].default == 2.0
    # the reference's constructor arguments still lead the processor's signature (gccNMFProcessor.py:168-171)
    assert list(inspect.signature(rt.GCCNMFProcessor.__init__).parameters)[1:11] == [
        'sampleRate', 'windowSize', 'numTimePerChunk', 'dictionariesW', 'dictionaryType', 'dictionarySize', 'numHUpdates',
        'microphoneSeparationInMetres', 'localizationEnabled', 'localizationWindowSize']
    from gcc_nmf_amd import distributed
    src = inspect.getsource(distributed)
    assert 'gccPHATNL' not in src                            # out of scope there: nothing that could silently ignore the keywords


def _bits(alpha):
    return ctypes.c_uint32.from_buffer_copy(ctypes.c_float(alpha)).value


def test_packed_alpha_of_the_c_call():
    """GCC-NONLIN is a mode of gccnmf_angular_spectrogram: the float32 bits of alpha in the upper halves of D and batch, both zero =
    PHAT.  Every check comes before the first HIP call, so the rejections are testable here."""
    from gcc_nmf_amd import _hip
    lib = _hip.lib()
    for D, B, alpha in ((128, 64, 2.0), (3, 1, 0.5), (4096, 65535, 8.0), (200, 5, 0.3), (64, 3, 1e-30), (64, 3, 3e38)):
        Dw, Bw = _hip.angular_nl_words(D, B, alpha)
        assert -2 ** 31 <= Dw < 2 ** 31 and -2 ** 31 <= Bw < 2 ** 31
        assert (Dw & 0xffff, Bw & 0xffff) == (D, B)
        assert ((Dw & 0xffff0000) | ((Bw >> 16) & 0xffff)) == _bits(alpha)
    assert _hip.angular_nl_words(128, 64, 2.0) == (128 | 0x40000000, 64)
    for D, B in ((0, 1), (65536, 1), (128, 0), (128, 65536)):
        with pytest.raises(ValueError):
            _hip.angular_nl_words(D, B, 2.0)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ERR_ARG = 1

    def call(D, B, alpha_bits, CC=p):
        Dw = ctypes.c_int32((D | (alpha_bits & 0xffff0000)) & 0xffffffff).value
        Bw = ctypes.c_int32((B | ((alpha_bits & 0xffff) << 16)) & 0xffffffff).value
        return lib.gccnmf_angular_spectrogram(CC, p, 513, 10, Dw, Bw, p, None, None)
    for bad in (-2.0, -0.0, float('nan'), float('inf'), -float('inf'), 1e-45, 1e-39):      # alpha <= 0, not finite, subnormal
        assert call(128, 1, _bits(bad)) == ERR_ARG, bad
    assert call(128, 1, _bits(2.0), CC=None) == ERR_ARG                                   # ... and whatever the PHAT form rejects
    assert call(0, 1, _bits(2.0)) == ERR_ARG and call(128, 0, _bits(2.0)) == ERR_ARG
    assert lib.gccnmf_angular_spectrogram(p, p, 1, 10, _hip.angular_nl_words(128, 1, 2.0)[0], 1, p, None, None) == ERR_ARG     # F < 2
    assert lib.gccnmf_angular_spectrogram(p, p, 513, 10, -5, 1, p, None, None) == ERR_ARG    # negative sizes stay errors
    assert lib.gccnmf_angular_spectrogram(p, p, 513, 10, 5, -1, p, None, None) == ERR_ARG
    # the header's macros are the same packing
    import os
    import re
    from conftest import REPO
    src = open(os.path.join(REPO, 'include', 'gccnmf_hip.h')).read()
    assert re.search(r'#define GCCNMF_ANGULAR_NL_D\(D, alpha_bits\) \(\(int\)\(\(unsigned\)\(D\) \| \(\(unsigned\)\(alpha_bits\) & 0xffff0000u\)\)\)', src)
    assert re.search(r'#define GCCNMF_ANGULAR_NL_BATCH\(batch, alpha_bits\) \(\(int\)\(\(unsigned\)\(batch\) \| \(\(unsigned\)\(alpha_bits\) << 16\)\)\)', src)


def test_row8_bit_of_the_streaming_call():
    """frames_mode bit 24 (the single-stream target row has word 6 = gccPHATNLAlpha) is an error together with the bank or multi-target
    layouts, whose rows always have the word; nothing above bit 24."""
    from gcc_nmf_amd import _hip
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(bits, mode=2):
        return _hip.lib().gccnmf_rt_process_block_ll(*([p] * 23), 1024, 512, 512, 128, 128, 64, 64, 128, mode, 1, 1, 6, bits, 0, 2, None)
    assert _hip.RT_ROW8_LAYOUT == 1 << 24 == _hip.rt_mode_word(nl_row=True)
    for bits, mode in (((1 << 24) | 8, 2), ((1 << 24) | (1 << 20), 1), (1 << 25, 2), ((1 << 24) | (1 << 25), 2), ((1 << 24) | (3 << 21), 2)):
        assert call(bits, mode) == 1, bits


# ---- the streaming margins the GPU test relies on ---------------------------------------------------------------------------------
FS, SPACING, DELAYS = 16000, 1.0, (-20, 3, 27)
# name: (windowSize, hopSize, blockSize, D, asymmetric synthesis size or None): config 5's shape and one odd window size
STREAMS = {'config5': (512, 64, 64, 64, 128), 'direct_sum_ws400': (400, 100, 100, 48, None)}
ALPHA, L_WINDOW, N_BLOCKS, WARMUP = 2.0, 24, 60, 32


def restated_stream(name, seed=0):
    """The synthetic three-talker stream of the multi-target tests through the reference's framing (oracle.rt_oracle) and the restated
    GCC-NONLIN localisation: per block (gccPHAT in float64, its float32 evaluation's distance, window mean)."""
    from gcc_nmf_amd.realtime import asymmetricWindows
    from gcc_nmf_amd.synthetic import synthetic_mixture
    ws, hop, B, D, syn = STREAMS[name]
    x = synthetic_mixture(seed, numSamples=N_BLOCKS * B, sampleRate=FS, delays=DELAYS)
    window = asymmetricWindows(ws, syn)[0] if syn else np.sqrt(np.hamming(ws).astype(np.float32))
    f32 = np.linspace(0, FS / 2, ws // 2 + 1).astype(np.float32)
    t32 = np.linspace(-SPACING / R.SPEED_OF_SOUND_IN_METRES_PER_SECOND, SPACING / R.SPEED_OF_SOUND_IN_METRES_PER_SECOND, D).astype(np.float32)
    cos64, sin64 = NL.tables(f32, t32)                       # the float32 grids of gccNMFProcessor.py:245-248, exact angles
    ola = R.OverlapAddOracle(2, ws, hop, B, B // hop)
    tracker = NL.StreamTracker(D, 128, L_WINDOW)
    out = []
    for b in range(N_BLOCKS):
        ola.processFrames(x[:, b * B:(b + 1) * B], lambda w: np.zeros_like(w))
        X = np.fft.rfft(ola.windowedSamples * window[:, None], axis=1).astype(np.complex64)
        with np.errstate(invalid='ignore', divide='ignore'):
            C = (X[0] * X[1].conj() / np.abs(X[0]) / np.abs(X[1])).astype(np.complex64)
        g64 = NL.gccphat_nl(C, cos64, sin64, ALPHA)
        g32 = NL.gccphat_nl(C, cos64.astype(np.float32), sin64.astype(np.float32), ALPHA, np.float32)
        with np.errstate(invalid='ignore'):
            err = float(np.nanmax(np.abs(g32.astype(np.float64) - g64))) if np.isfinite(g64).any() else 0.0
        out.append((g64, err, tracker.push(g64)))
    return out


def separated(windowMean, bar, n=3):
    """(arg-max, the n largest peaks) of a restated window mean when every margin -- maximum over runner-up, each chosen peak over its
    neighbours, the last chosen peak over the next candidate -- is above 100 bars; None otherwise.  Decided by the restatement alone."""
    i, m1 = NL.argmax_margin(windowMean)
    chosen, neighbour, runner_up = NL.peak_margins(windowMean, n)
    if chosen is None or min(m1, neighbour, runner_up) <= 100 * bar:
        return None
    return i, chosen


@pytest.mark.parametrize('name', list(STREAMS))
def test_stream_margins_are_100_bars(name):
    """The stream is not stationary (the talkers' envelopes move, one talker sits between two grid points), so a window mean passes
    through ties now and then.  After the warm-up most window means of the restated stream separate their arg-max from the runner-up,
    and their three largest peaks from their neighbours and from the fourth, by more than 100 x the measured bar (4 x the float32
    evaluation's error on gccPHAT): on those blocks the device is asked for exactly the restatement's indexes (the tracked indexes of a
    block depend on the history alone, not on earlier decisions)."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        blocks = restated_stream(name)
    bar = NL.BAR_FACTOR * max(e for _, e, _ in blocks)
    assert 0 < bar < 2e-5, bar                               # values in [0, 1]: a few float32 ulp through the square root
    good = 0
    for b in range(WARMUP, N_BLOCKS):
        g, _, wm = blocks[b]
        assert np.all((g >= 0) & (g <= 1))
        good += separated(wm, bar) is not None
    print('%s: bar %.3g, %d of %d blocks separated by 100 bars' % (name, bar, good, N_BLOCKS - WARMUP))
    assert good >= (N_BLOCKS - WARMUP) // 2, good
