"""numSources='auto' without a device: the NumPy restatement of the talker count against scikit-learn's KMeans
on the committed mean angular spectra and on built cases, the mode words and wrapper tuples of the two C calls, the argument checks,
and the float64 oracle pipeline counting the talkers of synthetic mixtures."""
import logging
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import source_count_restatement as SC
from conftest import REPO, golden
from oracle import gccnmf_oracle as O

GOLDENS = ['dev1_female3_liverec_130ms_1m_hop128_K128', 'dev1_hop256_K128', 'dev_A_1_2_3_4_hop256_K128', 'dev_B_1_8_9_16_hop256_K128',
           'dev_C_2_7_10_15_hop256_K128', 'dev_D_13_14_15_16_hop256_K128', 'dev_Sq1_Co_A_hop256_K128', 'synthetic0_hop256_K128']
GOLDEN_COUNTS = [3, 3, 1, 5, 1, 5, 2, 3]
# delays (samples at 16 kHz) -> the peaks of the 128-TDOA grid they land on; the talkers of synthetic_mixture(i, 32000, 16000, delays)
MIXTURES = [((12,), [47]), ((-20, 27), [27, 91]), ((-20, 3, 27), [27, 59, 91]), ((-30, -10, 8, 27), [27, 53, 77, 104]),
            ((-32, -16, 0, 14, 30), None)]
STREAM = 0x5eed


def count(v, Smax=8):
    idx, status = SC.count_sources(v, Smax)
    assert len(idx) == Smax and idx[sum(i >= 0 for i in idx):] == [-1] * sum(i < 0 for i in idx)
    return [i for i in idx if i >= 0], status


def spectrum(heights, gap=0.0):
    """Peaks of the given heights at 1, 3, 5, ... over a floor of ``gap``."""
    v = np.full(2 * len(heights) + 1, gap, np.float64)
    v[1::2] = heights
    return v


def test_restatement_is_kmeans_on_the_committed_spectra():
    pytest.importorskip('sklearn')
    counts = []
    for name in GOLDENS:
        v = golden(name)['meanA']
        kept, status = count(v)
        assert status == 0
        assert kept == SC.kmeans_upper_cluster(v, n_init=10, random_state=0), name
        counts.append(len(kept))
    assert counts == GOLDEN_COUNTS
    dev1 = golden('dev1_hop256_K128')
    assert count(dev1['meanA'])[0] == dev1['idx'].tolist()            # three talkers, and the three peaks the fixed count keeps


def test_worked_ties_and_degenerate_spectra():
    # {3, 2, 1}: b_1 = b_2 = 13.5 exactly -> the smaller j
    assert SC.split_scores([3.0, 2.0, 1.0]).tolist() == [13.5, 13.5]
    assert count(spectrum([3.0, 2.0, 1.0])) == ([1], 0)
    assert count(spectrum([1.0, 3.0, 2.0])) == ([3], 0)
    # {2, 2, 2, 0}: equal heights, the larger index first -- the split falls behind the three of them
    assert count(spectrum([2.0, 2.0, 0.0, 2.0], gap=-1.0)) == ([1, 3, 7], 0)
    # all peaks equal: every b_j is P h^2 up to rounding; whichever j wins, the kept ones are the LAST ones (larger index first)
    kept, status = count(spectrum([1.0] * 4), Smax=8)
    assert status == 0 and kept == [1, 3, 5, 7][-len(kept):]
    # P = 0 (monotone, plateau, D = 3 without a peak) and P = 1
    for v in (np.arange(9.0), np.array([0.0, 1.0, 1.0, 0.0]), np.array([1.0, 1.0, 0.0]), np.zeros(5)):
        assert count(v, 3) == ([], 1)
    assert count(np.array([0.0, 1.0, 0.0]), 3) == ([1], 0) and count(np.array([0.0, 1.0, 0.0]), 1) == ([1], 0)
    # NaN: never a peak, never greater than a neighbour
    v = spectrum([5.0, 4.0, 1.0, 0.5])
    v[3] = np.nan                                                     # the second peak goes, and its neighbours cannot beat NaN
    assert count(v) == ([1], 0)
    v = spectrum([5.0, 1.0, 0.9])
    v[0] = np.nan                                                     # v[1] > NaN is false: the highest peak is none
    assert count(v) == ([3], 0)
    # a non-finite peak: the sum of heights is not finite -> nothing counted
    assert count(spectrum([np.inf, 1.0, 0.5])) == ([], 1)
    assert count(spectrum([1e308, 1e308, 1.0])) == ([], 1)
    assert count(spectrum([np.inf])) == ([1], 0)                      # one peak is one talker: the sum is not looked at
    # the cap: five in the upper cluster, the Smax highest kept (ties: the larger index), status 2
    v = spectrum([9.0, 9.5, 9.0, 9.2, 9.1, 1.0, 1.1])
    assert count(v, 8) == ([1, 3, 5, 7, 9], 0)
    assert count(v, 5) == ([1, 3, 5, 7, 9], 0)
    assert count(v, 3) == ([3, 7, 9], 2)
    assert count(v, 2) == ([3, 7], 2)
    assert count(spectrum([9.0, 9.0, 9.0, 1.0]), 2) == ([3, 5], 2)


def test_mode_words_are_the_header_macros(tmp_path):
    from gcc_nmf_amd import _hip
    header = os.path.join(REPO, 'include', 'gccnmf_hip.h')
    src = open(header).read()
    assert re.search(r'#define GCCNMF_PEAKS_COUNT_BIT \(1 << 30\)', src)
    assert re.search(r'#define GCCNMF_PEAKS_COUNT\(Smax\) \(\(Smax\) \| GCCNMF_PEAKS_COUNT_BIT\)', src)
    assert re.search(r'#define GCCNMF_SCORES_COUNTED 0x800\b', src)
    assert _hip.GCCNMF_PEAKS_COUNT_BIT == 1 << 30 and _hip.GCCNMF_SCORES_COUNTED == 0x800
    sizes = (1, 4, 8, 255)
    assert [_hip.peaks_count_word(s) for s in sizes] == [s | 1 << 30 for s in sizes]
    for bad in (0, 256, -1, 2.0, True, None, '4'):
        with pytest.raises(ValueError):
            _hip.peaks_count_word(bad)
    # the new words collide with none of the existing modes: bit 8 marks a tracks word, 0x100 / 0x200 / 0x400 the scores' modes
    assert not _hip.peaks_count_word(255) & 0x3fffff00 and _hip.peaks_count_word(255) > 0
    assert not _hip.GCCNMF_SCORES_COUNTED & (_hip.GCCNMF_SCORES_TRACKS | _hip.GCCNMF_SCORES_ATOM_TDOA | _hip.GCCNMF_SCORES_ENHANCEMENT_MASKS | 0xff)
    # ... and the macros themselves, through the host C compiler where there is one
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    if cc:
        prog = tmp_path / 'words.c'
        prog.write_text('#include <stdio.h>\n#include "%s"\nint main(void) { printf("%%d %%d %%d %%d %%d\\n", GCCNMF_PEAKS_COUNT(1), '
                        'GCCNMF_PEAKS_COUNT(4), GCCNMF_PEAKS_COUNT(8), GCCNMF_PEAKS_COUNT(255), GCCNMF_SCORES_COUNTED); return 0; }\n' % header)
        exe = str(tmp_path / 'words')
        subprocess.check_call([cc, str(prog), '-o', exe])
        out = subprocess.check_output([exe]).decode().split()
        assert [int(w) for w in out] == [_hip.peaks_count_word(s) for s in sizes] + [_hip.GCCNMF_SCORES_COUNTED]


class StubLibrary(object):
    """Every attribute is an entry point that records (name, args) and returns 0 (the stub of tests/test_stage_words_host.py)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def test_wrappers_pass_the_documented_tuples(monkeypatch):
    from gcc_nmf_amd import _hip
    stub = StubLibrary()
    monkeypatch.setattr(_hip, '_lib', stub)
    _hip.count_tdoa_peaks(1, 128, 192, 4, 8, 2, 3, stream=STREAM)
    assert stub.calls[-1] == ('gccnmf_pick_tdoa_peaks', (1, 128, 192, 4 | 1 << 30, 8, 2, 3, STREAM))
    _hip.target_scores_masks_counted(1, 2, 3, 4, 513, 40, 16, 128, 4, 8, 5, 6, 7, counted=True, stream=STREAM)
    assert stub.calls[-1] == ('gccnmf_target_scores_masks', (1, 2, 3, 4, 513, 40, 16, 128, 4 | 0x800, 8, 5, 6, 7, STREAM))
    _hip.target_scores_masks_counted(1, 2, 3, 4, 513, 40, 16, 128, 4, 8, 5, 6, None, stream=STREAM)
    assert stub.calls[-1] == ('gccnmf_target_scores_masks', (1, 2, 3, 4, 513, 40, 16, 128, 4, 8, 5, 6, 0, STREAM))
    # the existing wrappers pass what they passed
    _hip.pick_tdoa_peaks(1, 128, 192, 3, 8, 2, 3, stream=STREAM)
    assert stub.calls[-1] == ('gccnmf_pick_tdoa_peaks', (1, 128, 192, 3, 8, 2, 3, STREAM))
    _hip.target_scores_masks(1, 2, 3, 4, 513, 40, 16, 128, 3, 8, 5, 6, 7, stream=STREAM)
    assert stub.calls[-1] == ('gccnmf_target_scores_masks', (1, 2, 3, 4, 513, 40, 16, 128, 3, 8, 5, 6, 7, STREAM))
    n = len(stub.calls)
    for bad in (0, 256):
        with pytest.raises(ValueError):
            _hip.count_tdoa_peaks(1, 128, 192, bad, 8, 2, 3, stream=STREAM)
        with pytest.raises(ValueError):
            _hip.target_scores_masks_counted(1, 2, 3, 4, 513, 40, 16, 128, bad, 8, 5, 6, 7, counted=True, stream=STREAM)
    assert len(stub.calls) == n                                        # rejected before the library is called


def test_argument_checks_need_no_device():
    from gcc_nmf_amd import _hip, engine
    from gcc_nmf_amd import gccNMFFunctions as G
    assert G.MAX_AUTO_SOURCES == _hip.MAX_AUTO_SOURCES == 8
    assert _hip.check_auto_sources('auto', 8) is True and _hip.check_auto_sources('auto', 1) is True and _hip.check_auto_sources('auto', 255) is True
    for fixed in (3, 1, None, 0, 0.0, False, np.int64(2)):                # not a string: the callers' own rules decide
        assert _hip.check_auto_sources(fixed, 8) is False
    for bad in ('Auto', '', 'none', '3', b'auto'.decode() + ' '):
        with pytest.raises(ValueError):
            _hip.check_auto_sources(bad, 8)
    for bad in (0, 256, -1, 4.0, True, None, '4'):
        with pytest.raises(ValueError):
            _hip.check_auto_sources('auto', bad)
    # falsy counts keep raising in the named function, before any device work
    for falsy in (None, 0, 0.0, False, [], ''):
        with pytest.raises(ValueError):
            G.estimateTargetTDOAIndexesFromAngularSpectrum(np.zeros(8), 1.0, 8, falsy)
    with pytest.raises(ValueError):
        G.estimateTargetTDOAIndexesFromAngularSpectrum(np.zeros(8), 1.0, 8, 'all')
    with pytest.raises(ValueError):
        G.estimateNumSourcesFromAngularSpectrum(np.zeros(8), 0)
    with pytest.raises(ValueError):
        G.getTargetTDOAEstimates(np.ones((2, 5, 3), np.complex64), 16000, 1.0, 8, 'all')
    # the engines: (auto, slots)
    assert _hip.check_auto_targets('auto', None) == (True, 4) and _hip.check_auto_targets('auto', 8) == (True, 8)
    assert _hip.check_auto_targets(3, None) == (False, 3) and _hip.check_auto_targets(3, None, True) == (False, 3)
    for kw in (dict(numTargets='auto', tdoaTracking=True, localizationWindowSize=9), dict(numTargets='auto', maxTargets=9),
               dict(numTargets='auto', maxTargets=0), dict(numTargets='auto', maxTargets=2.0), dict(numTargets='auto', maxTargets=True),
               dict(numTargets=3, maxTargets=4), dict(maxTargets=4), dict(numTargets='three')):
        with pytest.raises(ValueError):                                 # before the constructors look for a device
            engine.GCCNMFEngine(32000, **kw)
        with pytest.raises(ValueError):
            engine.GCCNMFEngine(lengths=[32000, 48000], **kw)
    with pytest.raises(TypeError):
        engine.GCCNMFEnhancementEngine(32000, numTargets='auto')


def oracle_mean_spectrum(i, delays):
    from gcc_nmf_amd.synthetic import synthetic_mixture
    X = O.computeComplexMixtureSpectrogram(synthetic_mixture(i, 32000, 16000, delays=delays), 1024, 256, np.hanning)
    ang = O.getAngularSpectrogram(O.spectralCoherence(X), O.getFrequenciesInHz(16000, 513), 1.0, 128)
    return np.mean(ang, axis=-1)


def test_oracle_pipeline_counts_the_talkers():
    for delays, peaks in MIXTURES[:4]:
        v = oracle_mean_spectrum(0, delays)
        kept, status = count(v)
        assert (kept, status) == (peaks, 0), delays
        # the decision is not a near-tie: the best split leads the runner-up by several per cent
        if len(SC.peak_indexes(v)) > 2:
            order = np.sort(v[SC.peak_indexes(v)])[::-1]
            b = np.sort(SC.split_scores(order))
            assert b[-1] > 1.05 * b[-2], (delays, b[-2:])
    v = oracle_mean_spectrum(0, MIXTURES[4][0])
    five, status = count(v, 8)
    assert len(five) == 5 and status == 0
    four, status = count(v, 4)
    assert status == 2 and len(four) == 4
    by_height = sorted(five, key=lambda p: v[p])[-4:]
    assert four == sorted(by_height)


def test_info_lines_of_the_named_function(monkeypatch, caplog):
    """Status 1 raises the reference's "didn't find enough peaks", status 2 is logged only (no device: the count is stubbed)."""
    from gcc_nmf_amd import gccNMFFunctions as G
    answers = iter([(3, [np.int64(5), np.int64(9), np.int64(20)], 0), (8, [np.int64(i) for i in range(1, 17, 2)], 2), (0, [], 1)])
    monkeypatch.setattr(G, 'estimateNumSourcesFromAngularSpectrum', lambda spectrum, maxSources=8: next(answers))
    with caplog.at_level(logging.INFO):
        assert G.estimateTargetTDOAIndexesFromAngularSpectrum(np.zeros(32), 1.0, 32, 'auto') == [5, 9, 20]
        assert 'numSources not provided, found 3 sources' in caplog.text
        assert len(G.estimateTargetTDOAIndexesFromAngularSpectrum(np.zeros(32), 1.0, 32, 'auto')) == 8
        assert 'keeping the 8 highest' in caplog.text
    with pytest.raises(ValueError, match="didn't find enough peaks"):
        G.estimateTargetTDOAIndexesFromAngularSpectrum(np.zeros(32), 1.0, 32, 'auto')
