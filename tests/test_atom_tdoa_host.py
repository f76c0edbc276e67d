"""No device: the float64 restatement of the offline-enhancement stages (tests/atom_tdoa_restatement.py) against a brute-force loop,
its tie / NaN rules and mask formulas at their edges; every ValueError of the wrappers, the reference-style functions and the engine,
raised before any device work; and the algorithm itself on synthetic.speech_in_noise_mixture -- the float64 pipeline must raise the SDR
of a 0 dB mixture."""
import numpy as np
import pytest

import atom_tdoa_restatement as A


def tiny(seed, F=9, T=4, K=5, D=7):
    rng = np.random.default_rng(seed)
    C = np.exp(1j * rng.uniform(-np.pi, np.pi, (F, T))).astype(np.complex64)
    ang = rng.uniform(-np.pi, np.pi, (F, D))
    return C, np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32), rng.uniform(0, 1, (F, K)).astype(np.float32)


def test_restatement_against_brute_force():
    C, cos, sin, W = tiny(0)
    idx, S64, Sabs = A.atom_tdoa(C, cos, sin, W)
    assert idx.shape == (5, 4) and S64.shape == (5, 7, 4) and Sabs.shape == (5, 4)
    assert np.array_equal(idx, A.brute_force_index(C, cos, sin, W))
    k, d, t = 3, 2, 1
    terms = [float(W[f, k]) * (float(C[f, t].real) * float(cos[f, d]) + float(C[f, t].imag) * float(sin[f, d])) for f in range(9)]
    assert abs(S64[k, d, t] - sum(terms)) < 1e-12
    assert (Sabs >= np.abs(S64).max(axis=1) - 1e-12).all()
    assert abs(Sabs[k, t] - max(sum(abs(float(W[f, k])) * abs(float(C[f, t].real) * float(cos[f, dd]) + float(C[f, t].imag) * float(sin[f, dd]))
                                    for f in range(9)) for dd in range(7))) < 1e-12
    part, _ = A.scores(C, cos, sin, W, frames=[2])
    assert np.abs(part[:, :, 0] - S64[:, :, 2]).max() < 1e-12


def test_tie_nan_and_all_nan_rules():
    C, cos, sin, W = tiny(1)
    cos[:, 5], sin[:, 5] = cos[:, 2], sin[:, 2]                    # identical columns: the lower index wins
    idx = A.atom_tdoa(C, cos, sin, W)[0]
    assert not (idx == 5).any()
    assert np.array_equal(idx, A.brute_force_index(C, cos, sin, W))
    silent = C.copy()
    silent[:, 1] = 0
    assert (A.atom_tdoa(silent, cos, sin, W)[0][:, 1] == 0).all()
    nan = C.copy()
    nan[4, 3] = np.nan
    got = A.atom_tdoa(nan, cos, sin, W)[0]
    assert (got[:, 3] == 0).all() and np.array_equal(got[:, :3], idx[:, :3])
    assert np.array_equal(got, A.brute_force_index(nan, cos, sin, W))
    S = np.array([[np.nan, 1.0, 3.0, 3.0], [np.nan] * 4, [2.0, np.nan, 2.0, 1.0]])
    assert A.nan_argmax_first(S, axis=1).tolist() == [2, 0, 0]


def test_mask_formulas_at_the_edges():
    index = np.array([[10, 12, 14, 15, 6, 5]])
    im, m = A.masks(index, 10, 0, 4.0)
    assert im.tolist() == [[0, 0, 1, 1, 1, 1]], '|i - target| = eps is noise: the comparison is strict'
    assert m[0].tolist() == [[1, 1, 0, 0, 0, 0]] and np.array_equal(m[1], 1 - m[0])
    for beta in (1.0, 2.0):
        for nf in (0.0, 0.25):
            im, m = A.masks(index, 10, 1, 4.0, beta, nf)
            dist = np.abs(index - 10.0)
            assert np.allclose(m[0], np.exp(-(dist / 4.0) ** beta) / (1 + nf) + nf, rtol=0, atol=1e-15)
            assert m[0][0, 0] == 1 / (1 + nf) + nf and abs(m[0][0, 2] - (np.exp(-1.0) / (1 + nf) + nf)) < 1e-15
            assert np.array_equal(m[1], 1 - m[0]) and im.tolist() == [[0, 0, 1, 1, 1, 1]]
    assert A.masks(index, 10, 1, 4.0, 2.0, 0.5)[1][0].max() > 1, 'the window mask is not clamped: 1 / (1 + nf) + nf > 1 for nf < 1'
    per_frame = A.masks(index, np.array([10, 12, 14, 15, 6, 5]), 0, 1.0)[0]
    assert per_frame.tolist() == [[0] * 6]


def test_value_errors_before_any_device_work(monkeypatch):
    """the checks run with the library and the device out of reach"""
    import torch
    from gcc_nmf_amd import _hip, engine, gccNMFFunctions as G

    def unreachable(*a, **k):
        raise AssertionError('device work before the argument check')
    monkeypatch.setattr(_hip, 'lib', unreachable)
    monkeypatch.setattr(G, '_device', unreachable)
    monkeypatch.setattr(torch.cuda, 'is_available', unreachable)
    ok = (0, 4.0, 2.0, 0.0)
    assert _hip.check_enhancement_target(*ok) == (0, 4.0, 2.0, 0.0)
    assert _hip.check_enhancement_target('window', 5, 1, 0.5) == (1, 5.0, 1.0, 0.5)
    assert _hip.check_enhancement_target(_hip.TARGET_MODE_WINDOW_FUNCTION, 5, 1, 0)[0] == 1
    from gcc_nmf_amd import realtime
    assert (_hip.TARGET_MODE_BOXCAR, _hip.TARGET_MODE_WINDOW_FUNCTION) == (realtime.TARGET_MODE_BOXCAR, realtime.TARGET_MODE_WINDOW_FUNCTION)
    for bad in ((realtime.TARGET_MODE_MULTIPLE, 4.0, 2.0, 0.0), ('soft', 4.0, 2.0, 0.0), (True, 4.0, 2.0, 0.0), (0, 0.0, 2.0, 0.0),
                (0, -1.0, 2.0, 0.0), (0, float('nan'), 2.0, 0.0), (0, 4.0, 0.0, 0.0), (0, 4.0, float('inf'), 0.0), (0, 4.0, 2.0, -0.1),
                (0, 4.0, 2.0, None), (0, '4', 2.0, 0.0), (0, 1e-60, 2.0, 0.0)):
        with pytest.raises(ValueError):
            _hip.check_enhancement_target(*bad)
    with pytest.raises(ValueError):
        _hip.enhancement_masks(1, 2, 10, 4, 1, 3, 4, window=2)
    C, cos, sin, W = tiny(2)
    f = np.linspace(0, 8000, 9)
    for args in ((C[0], 1.0, 7, f, W), (C, 1.0, 0, f, W), (C, 1.0, 1025, f, W), (C, 1.0, 7.5, f, W), (C, 1.0, 7, f[:-1], W), (C, 1.0, 7, f, W[:-1]),
                 (C, 1.0, 7, f, W[:, :0]), (C, 1.0, 7, f, W.astype(np.complex64)), (C[:1], 1.0, 7, f[:1], W[:1])):
        with pytest.raises(ValueError):
            G.getAtomTDOAIndexes(*args)
    idx = np.zeros((5, 4), np.int64)
    for args in ((idx[0], 3), (idx.astype(np.float32), 3), (idx - 1, 3), (idx + 70000, 3), (idx, [1, 2, 3]), (idx, 2.5), (idx, np.zeros((2, 4))),
                 (idx, float('nan')), (idx[:, :0], 3)):
        with pytest.raises(ValueError):
            G.getEnhancementCoefficientMasks(*args)
    for kw in (dict(targetMode='soft'), dict(targetTDOAEpsilon=0), dict(targetTDOABeta=-1), dict(targetTDOANoiseFloor=-1)):
        with pytest.raises(ValueError):
            G.getEnhancementCoefficientMasks(idx, 3, **kw)
    E = engine.GCCNMFEnhancementEngine
    for kw in (dict(lengths=[16000, 12000]), dict(targetMode='soft'), dict(targetTDOAEpsilon=0.0), dict(targetTDOABeta=float('nan')),
               dict(targetTDOANoiseFloor=-0.5), dict(targetTDOAIndex=128), dict(targetTDOAIndex=-1), dict(targetTDOAIndex=[3, 4]),
               dict(targetTDOAIndex=2.5), dict(targetTDOAIndex=[[3]]), dict(numTDOAs=1025), dict(numTDOAs=2), dict(reconstruction='wiener'),
               dict(tdoaTracking=True), dict(numFreeAtoms=4), dict(tolerance=2.0)):
        with pytest.raises(ValueError):
            E(16000, **kw)
    with pytest.raises(TypeError):
        E(16000, numTargets=2)
    assert engine.check_enhancement_target_index(5, 3, 128).tolist() == [5, 5, 5]
    assert engine.check_enhancement_target_index([1, 2, 3], 3, 128).tolist() == [1, 2, 3] and engine.check_enhancement_target_index(None, 3, 128) is None


def test_the_float64_pipeline_raises_the_sdr_at_0_db():
    from gcc_nmf_amd.synthetic import speech_in_noise_mixture
    x, clean = speech_in_noise_mixture(0, 0.0, numSamples=32000)
    assert x.shape == (2, 32000) and x.dtype == np.float32 and clean.shape == (2, 32000)
    assert np.array_equal(x, np.round(x * 32768) / 32768), 'int16-representable samples'
    again = speech_in_noise_mixture(0, 0.0, numSamples=32000)[0]
    assert np.array_equal(x, again) and not np.array_equal(x, speech_in_noise_mixture(1, 0.0, numSamples=32000)[0])
    sdr_in, sdr_out, target = A.float64_enhancement(x, clean, K=32, iterations=60)
    print('0 dB mixture: input SDR %.2f dB, output SDR %.2f dB, talker at index %d' % (sdr_in, sdr_out, target))
    assert abs(sdr_in) < 0.5
    assert sdr_out > sdr_in


def test_stage_words_of_the_two_wrappers(monkeypatch):
    """the exact integers that reach gccnmf_target_scores_masks for the two modes (no device, no library: a recording stub)"""
    import ctypes
    from gcc_nmf_amd import _hip
    calls = []

    class Stub(object):
        def gccnmf_target_scores_masks(self, *args):
            params = None
            if args[8] & _hip.GCCNMF_SCORES_ENHANCEMENT_MASKS:          # the three host floats are read during the call
                params = list(ctypes.cast(args[1], ctypes.POINTER(ctypes.c_float))[0:3])
            calls.append((args, params))
            return 0
    monkeypatch.setattr(_hip, '_lib', Stub())
    _hip.atom_tdoa_indexes(1, 2, 4, 513, 40, 16, 128, 8, 7, 6, stream=0x5eed)
    assert calls[-1] == ((1, 2, 0, 4, 513, 40, 16, 128, 0x200, 8, 0, 6, 7, 0x5eed), None)
    _hip.atom_tdoa_indexes(1, 2, 4, 513, 40, 16, 128, 8, 7, stream=0x5eed)
    assert calls[-1][0][11:13] == (0, 7)
    _hip.enhancement_masks(1, 3, 40, 16, 8, 7, 6, window=1, eps=2.5, beta=1.0, noise_floor=0.25, per_frame=True, stream=0x5eed)
    args, params = calls[-1]
    assert args[0] == 1 and args[2:] == (3, 0, 0, 40, 16, 0, 0x400 | 0x100 | 1, 8, 0, 6, 7, 0x5eed) and params == [2.5, 1.0, 0.25]
    _hip.enhancement_masks(1, 3, 40, 16, 8, 7, None, stream=0x5eed)
    args, params = calls[-1]
    assert args[8] == 0x400 and args[11:13] == (0, 7) and params == [5.0, 2.0, 0.0], 'the defaults are realtime/config.py:56-58, boxcar'
