"""CPU checks of the time-varying TDOA tracks: the NumPy restatement (tests/tdoa_tracks_restatement.py) on hand-built
angular spectrograms and on the moving-talker mixture, and the argument validation of the engine and the drop-in functions, which runs
without a device."""
import numpy as np
import pytest

import angular_nl_restatement as NL
import tdoa_tracks_restatement as R
from oracle import gccnmf_oracle as O


def spectrogram(D, T, peaks_per_frame):
    """(D, T) zeros with the given {index: height} peaks in every frame (a dict, or one dict per frame)."""
    A = np.zeros((D, T))
    for t in range(T):
        for i, h in (peaks_per_frame[t] if isinstance(peaks_per_frame, list) else peaks_per_frame).items():
            A[i, t] = h
    return A


def test_windows_are_centred_and_truncated_at_both_ends():
    T, L = 10, 4                                                     # lo = t - 2, hi = t + 2
    assert [R.window_bounds(t, L, T) for t in (0, 1, 2, 5, 8, 9)] == [(0, 2), (0, 3), (0, 4), (3, 7), (6, 10), (7, 10)]
    assert [R.window_bounds(t, 5, T) for t in (0, 9)] == [(0, 3), (7, 10)]          # odd L: t - 2 .. t + 2
    assert R.window_bounds(3, 1, T) == (3, 4)
    A = np.arange(3 * T, dtype=np.float64).reshape(3, T) ** 2
    Abar = R.windowed_mean(A, L)
    for t in range(T):
        lo, hi = R.window_bounds(t, L, T)
        assert np.array_equal(Abar[:, t], A[:, lo:hi].sum(axis=1) / (hi - lo)), t      # a truncated window divides by its own length
    # a peak that exists in frame 0 alone is seen by exactly the frames whose window reaches frame 0
    A = spectrogram(9, T, [{2: 5.0, 6: 1.0}] + [{4: 1.0, 6: 1.0}] * (T - 1))
    tracks, status, _ = R.tdoa_tracks(A, 2, L)
    assert status.tolist() == [0] * T
    assert tracks[:, 0].tolist() == [2, 6] and tracks[:, 1].tolist() == [2, 6]         # windows [0, 2) and [0, 3): mean 2.5 / 1.67 at 2
    assert tracks[:, 2].tolist() == [2, 6]                                              # window [0, 4): 1.25 at 2, 0.75 at 4, 1 at 6
    assert tracks[:, 3].tolist() == [4, 6] and tracks[:, 9].tolist() == [4, 6]


def test_ties_keep_the_larger_index():
    A = spectrogram(12, 6, {2: 1.0, 5: 1.0, 8: 1.0, 10: 2.0})
    for L in (1, 3, 11):
        tracks, status, _ = R.tdoa_tracks(A, 2, L)
        assert np.array_equal(tracks, np.repeat([[8], [10]], 6, axis=1)) and not status.any()
        tracks, _, _ = R.tdoa_tracks(A, 3, L)
        assert np.array_equal(tracks, np.repeat([[5], [8], [10]], 6, axis=1))


def test_short_frames_carry_the_previous_set_and_leading_frames_take_the_first():
    one, two, other = {3: 1.0}, {3: 1.0, 7: 2.0}, {2: 1.0, 9: 2.0}
    A = spectrogram(12, 8, [one, one, two, one, other, one, one, two])
    tracks, status, _ = R.tdoa_tracks(A, 2, 1)                       # L = 1: every frame on its own
    assert status.tolist() == [1, 1, 0, 1, 0, 1, 1, 0]
    assert tracks.T.tolist() == [[3, 7], [3, 7], [3, 7], [3, 7], [2, 9], [2, 9], [2, 9], [3, 7]]
    with pytest.raises(ValueError, match='no frame has 2 peaks'):
        R.tdoa_tracks(spectrogram(12, 5, one), 2, 3)
    with pytest.raises(ValueError):
        R.tdoa_tracks(np.zeros((12, 5)), 1, 3)                       # no strict maximum anywhere


@pytest.mark.parametrize('name', list(NL.MIXTURES))
def test_whole_file_window_is_the_static_estimate_on_the_committed_mixtures(name):
    """L >= 2T - 1: every window is the whole file, the tracks are constant and equal the oracle's
    estimateTargetTDOAIndexesFromAngularSpectrum on the time mean."""
    S, _, phat = NL.MIXTURES[name]
    C, freqs, sr = NL.mixture_coherence(name)
    A = O.getAngularSpectrogram(C.astype(np.complex128), freqs, 1.0, 128)
    T = A.shape[1]
    want = O.estimateTargetTDOAIndexesFromAngularSpectrum(A.mean(axis=-1), 1.0, 128, S)
    assert [int(i) for i in want] == phat
    assert all(R.window_bounds(t, 2 * T - 1, T) == (0, T) for t in range(T)) and R.window_bounds(0, 2 * T - 2, T) == (0, T - 1)
    for L in (2 * T - 1, 5 * T):
        tracks, status, _ = R.tdoa_tracks(A, S, L)
        assert not status.any() and np.array_equal(tracks, np.repeat(np.array(want)[:, None], T, axis=1)), L


@pytest.mark.parametrize('seed', [1, 2])
def test_moving_mixture_tracks_follow_the_jump(seed):
    """The talker who changes seat (gcc_nmf_amd.synthetic.moving_source_mixture): 6 s at 16 kHz, source 0 at index 97 throughout, source
    1 at 56 / 57 before the midpoint and at 23 after it.  With a centred window of 48 frames the tracks sit within one index of those
    values outside L frames around the jump, no frame is short of peaks, and the whole-file estimate is [56, 97]."""
    from gcc_nmf_amd.synthetic import moving_source_mixture
    L, S = 48, 2
    x = moving_source_mixture(seed)
    assert x.shape == (2, 96000) and x.dtype == np.float32
    X = O.computeComplexMixtureSpectrogram(x, 1024, 256, np.hanning)
    C = O.spectralCoherence(X)
    A = O.getAngularSpectrogram(C, O.getFrequenciesInHz(16000, 513), 1.0, 128)
    T = A.shape[1]
    assert [int(i) for i in O.estimateTargetTDOAIndexesFromAngularSpectrum(A.mean(axis=-1), 1.0, 128, S)] == [56, 97]
    tracks, status, _ = R.tdoa_tracks(A, S, L)
    jump = (x.shape[1] // 2 - 512) / 256.0                           # the frame centred on the jump
    before, after = np.arange(T) < jump - L, np.arange(T) > jump + L
    print('seed %d: T = %d, jump at frame %.1f; moving talker %s -> %s, static talker %s, short frames %d'
          % (seed, T, jump, np.unique(tracks[0, before]), np.unique(tracks[0, after]), np.unique(tracks[1]), status.sum()))
    assert before.sum() > 100 and after.sum() > 100
    assert not status[before | after].any()
    assert np.all(np.abs(tracks[1, before | after] - 97) <= 1)
    assert np.all(np.abs(tracks[0, before] - 56.5) <= 1.5) and np.all(np.abs(tracks[0, after] - 23) <= 1)


def test_moving_mixture_generator_is_seeded_and_leaves_synthetic_mixture_alone():
    from gcc_nmf_amd.synthetic import moving_source_mixture, synthetic_mixture
    x, images = moving_source_mixture(3, numSamples=32000, returnSources=True)
    assert np.array_equal(x, moving_source_mixture(3, numSamples=32000)) and not np.array_equal(x, moving_source_mixture(4, numSamples=32000))
    assert images.shape == (2, 32000) and np.array_equal(np.round(x * 32768), x * 32768) and np.abs(x).max() <= 0.1 + 1.0 / 32768
    assert np.abs(x[0] - images.sum(axis=0)).std() < 0.02 * x[0].std()          # left channel = the two images + sensor noise
    assert synthetic_mixture(0, numSamples=2000).shape == (2, 2000)


def test_tracking_arguments_are_validated_without_a_device():
    from gcc_nmf_amd import _hip
    from gcc_nmf_amd import gccNMFFunctions as G
    from gcc_nmf_amd.engine import GCCNMFEngine, RaggedGCCNMFEngine, check_tdoa_tracking
    assert check_tdoa_tracking(False, None, 3) == (False, None) and check_tdoa_tracking(True, 48, 2) == (True, 48)
    assert check_tdoa_tracking(False, 7, None) == (False, 7) and check_tdoa_tracking(True, np.int64(5), np.int32(2)) == (True, 5)
    for L in (0, -3, 2.5, 48.0, '48', True):
        with pytest.raises(ValueError, match='localizationWindowSize'):
            check_tdoa_tracking(False, L, 2)                            # a bad window does not wait for the switch
    with pytest.raises(ValueError, match='localizationWindowSize'):
        check_tdoa_tracking(True, None, 2)
    for S in (None, 0, 256, 2.0, True):
        with pytest.raises(ValueError, match='number of sources'):
            check_tdoa_tracking(True, 48, S)
    # the engines validate in front of everything that needs the library or a device
    for make in (lambda **kw: GCCNMFEngine(16000, **kw), lambda **kw: GCCNMFEngine(lengths=[16000, 20000], **kw),
                 lambda **kw: RaggedGCCNMFEngine([16000], **kw)):
        with pytest.raises(ValueError, match='localizationWindowSize'):
            make(tdoaTracking=True)
        with pytest.raises(ValueError, match='localizationWindowSize'):
            make(tdoaTracking=True, localizationWindowSize=0)
        with pytest.raises(ValueError, match='number of sources'):
            make(tdoaTracking=True, localizationWindowSize=48, numTargets=None)
    # the word the library reads: S in the low byte, bit 8, min(L, 2T - 1) from bit 9
    assert _hip.peaks_tracks_word(2, 48, 372) == 2 | 0x100 | (48 << 9)
    assert _hip.peaks_tracks_word(3, 10 ** 9, 372) == 3 | 0x100 | (743 << 9) == _hip.peaks_tracks_word(3, 743, 372)
    assert 0 < _hip.peaks_tracks_word(255, 1 << 40, (1 << 21) - 1) < 1 << 31
    for bad in ((0, 4, 10), (256, 4, 10), (2, 0, 10), (2, 4, 0), (2, 4, 1 << 21)):
        with pytest.raises(ValueError):
            _hip.peaks_tracks_word(*bad)
    # drop-in functions
    A = np.zeros((128, 50))
    a32, S, L = G.check_angular_spectrogram_for_tracks(A, 128, 2, 16)
    assert a32.dtype == np.float32 and a32.shape == (128, 50) and (S, L) == (2, 16)
    for args in ((A, 64, 2, 16), (A, 128, 0, 16), (A, 128, 2, 0), (A, 128, 2, None), (A[0], 128, 2, 16), (A[:2], 2, 1, 16),
                 (A.astype(complex), 128, 2, 16), (A[:, :0], 128, 2, 16)):
        with pytest.raises(ValueError):
            G.check_angular_spectrogram_for_tracks(*args)
        with pytest.raises(ValueError):
            G.estimateTargetTDOATracksFromAngularSpectrogram(args[0], 1.0, *args[1:])
    idx, tracks = G.check_target_tdoa_indexes([47, np.int64(72), 107], 50)
    assert idx.dtype == np.int32 and idx.tolist() == [47, 72, 107] and not tracks
    idx, tracks = G.check_target_tdoa_indexes(np.repeat([[47], [72]], 50, axis=1), 50)
    assert idx.shape == (2, 50) and idx.flags.c_contiguous and tracks
    for bad in ([], np.zeros((2, 49), int), np.zeros((2, 50, 1), int), [1.5, 2.0], np.zeros((256, 50), int), 5):
        with pytest.raises(ValueError):
            G.check_target_tdoa_indexes(bad, 50)
    import inspect
    assert list(inspect.signature(G.estimateTargetTDOATracksFromAngularSpectrogram).parameters) == \
        ['angularSpectrogram', 'microphoneSeparationInMetres', 'numTDOAs', 'numSources', 'localizationWindowSize']


def test_frame_margin_and_image_sdr_helpers():
    v = np.zeros(12)
    v[[2, 5, 8]] = [3.0, 1.0, 2.5]
    assert R.frame_margin(v, 2) == 1.5 and R.frame_margin(v, 1) == 0.5 and R.frame_margin(v, 3) == 1.0
    v[5] = 2.5
    assert R.frame_margin(v, 2) == 0.0                               # a tie at the boundary
    n = 20000
    rng = np.random.RandomState(0)
    s = rng.standard_normal(n)
    est = s[512:] + 0.1 * rng.standard_normal(n - 512)               # the separated waveform starts windowSize / 2 into the mixture
    assert abs(R.image_sdr(est, s, 1024, 0, n - 1024) - 20.0) < 0.3
    assert R.image_sdr(est, np.roll(s, 7), 1024, 0, n - 1024) < 0
