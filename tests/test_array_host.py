"""CPU-only checks of the microphone-array feature: the float64 restatement tests/array_restatement.py against the
stereo restatements and the oracle at M = 2; the geometry helpers; the restatement's peaks on a synthetic 4-microphone line and on the
mixtures of the engine tests at 5 to 8 microphones; planted mistakes against the float64 checks the device tests use, at the stacked cells
of tests/stacked_pairs.py among them; the constructor's argument rules (no device needed); header, ctypes table and exported symbols of
libgccnmf_array.so; every argument rule of its C entry points (decided before any launch, so dummy pointers do)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

import array_restatement as A
import fft_checks as K
import gcc_checks as C
import ratio_restatement as R
import stacked_pairs as SP
from oracle import gccnmf_oracle as O

HEADER = os.path.join(REPO, 'include', 'gccnmf_array.h')
LINE = np.array([[0.0, 0, 0], [0.2, 0, 0], [0.5, 0, 0], [1.0, 0, 0]])
SOUND = 340.29


def random_problem(M, F, T, K, S, seed):
    rng = np.random.RandomState(seed)
    X = (rng.uniform(0.5, 2.0, (M, F, T)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (M, F, T)))).astype(np.complex64)
    W = rng.uniform(0.01, 1.0, (F, K)).astype(np.float32)
    H = rng.uniform(0.01, 1.0, (K, M * T)).astype(np.float32)
    am = rng.randint(0, S, (K, T)).astype(np.uint8)
    masks = rng.uniform(0.0, 1.0, (S, K, T)).astype(np.float32)
    return X, W, H, am, masks


def line_spectrogram(seed=0, n=16000, n_fft=1024, hop=256):
    from gcc_nmf_amd.synthetic import array_mixture
    x = array_mixture(seed, LINE, [40, 90, 130], n, 16000)
    T = 1 + (n - n_fft) // hop
    w = np.hanning(n_fft).astype(np.float32)
    X = np.concatenate([K.stft64(x[c:c + 2], w, n_fft, hop, T)[0] for c in (0, 2)])
    return x, X.astype(np.complex64)


# ---- M = 2 is the stereo path ------------------------------------------------------------------------------------------------------------
def test_restatement_at_two_channels_is_the_stereo_restatement():
    F, T, Kk, S, D = 33, 20, 7, 3, 16
    X, W, H, am, masks = random_problem(2, F, T, Kk, S, 1)
    X[0, 3, 4] = 0
    assert np.array_equal(A.ratio_one_hot(W, H, am, S, X), R.ratio_one_hot(W, H, am, S, X))
    assert np.array_equal(A.ratio_soft(W, H, masks, X), R.ratio_soft(W, H, masks, X))
    assert np.array_equal(A.denominators(W, H, 2, argmax=am, S=S), R.denominators(W, H, argmax=am, S=S))
    V, Cs = A.features(X)
    assert Cs.shape == (1, F, T) and Cs[0, 3, 4] == 0
    with np.errstate(invalid='ignore', divide='ignore'):
        ref = O.spectralCoherence(X)
    ok = np.isfinite(ref)
    assert not ok[3, 4] and ok.sum() == F * T - 1
    assert np.abs(Cs[0][ok] - ref[ok]).max() < 1e-6
    assert np.allclose(V, O.magnitudeSpectrogramV(X), rtol=1e-6, atol=0)
    freqs = O.getFrequenciesInHz(16000, F)
    tau = O.getTDOAsInSeconds(1.0, D)[None]
    ang, absprod = A.angular(Cs, freqs, tau)
    ref = O.getAngularSpectrogram(Cs[0], freqs, 1.0, D)
    assert np.abs(ang - ref).max() < 1e-10 and (absprod >= np.abs(ang) - 1e-12).all()
    idx = [2, 7, 11]
    G, absG = A.scores(Cs, W, freqs, tau, idx)
    ref = O.getTargetTDOAGCCNMFs(Cs[0], 1.0, D, freqs, idx, W, np.zeros((2, Kk, T)))
    assert np.abs(G - ref).max() < 1e-5 and (absG >= np.abs(G) - 1e-12).all()
    assert np.array_equal(A.argmax(G), np.argmax(O.getTargetCoefficientMasks(ref, 3), axis=0))
    peaks, status = A.peaks(ang.mean(axis=1), 2)
    assert status == 0 and peaks == O.estimateTargetTDOAIndexesFromAngularSpectrum(ang.mean(axis=1), 1.0, D, 2)


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------
def test_geometry_helpers():
    from gcc_nmf_amd.array import pairTDOAsFromGeometry, azimuthDirections
    from gcc_nmf_amd import _array
    assert _array.pairs(4) == A.pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)] and _array.num_pairs(8) == 28
    # two microphones 1 m apart along x, directions whose cosines are the stereo grid: the stereo TDOAs
    D = 128
    cosines = np.linspace(-1.0, 1.0, D)
    u = np.stack([cosines, np.sqrt(1 - cosines ** 2), np.zeros(D)], axis=1)
    tau = pairTDOAsFromGeometry([[0, 0, 0], [1, 0, 0]], u, SOUND)
    assert tau.shape == (1, D) and np.allclose(tau[0], O.getTDOAsInSeconds(1.0, D), rtol=1e-13, atol=1e-18)
    # the helpers are the restatement's
    dirs = azimuthDirections(181)
    assert np.array_equal(dirs, A.azimuth_directions(181)) and np.allclose((dirs ** 2).sum(axis=1), 1)
    assert np.allclose(dirs[0], [1, 0, 0]) and np.allclose(dirs[90], [0, 1, 0], atol=1e-15) and np.allclose(dirs[180], [-1, 0, 0], atol=1e-15)
    t = pairTDOAsFromGeometry(LINE, dirs, SOUND)
    assert t.shape == (6, 181) and np.array_equal(t, A.pair_tdoas_from_geometry(LINE, dirs, SOUND))
    assert np.allclose(t[2], np.cos(np.deg2rad(np.arange(181))) / SOUND)                  # pair (0, 3): 1 m
    # antisymmetric under swapping a pair: microphones in reverse order give pair (M-1-b, M-1-a) = -(a, b)
    rev = pairTDOAsFromGeometry(LINE[::-1], dirs, SOUND)
    for p, (a, b) in enumerate(A.pairs(4)):
        q = A.pairs(4).index((3 - b, 3 - a))
        assert np.array_equal(rev[q], -t[p])
    for bad in (dict(directions=dirs * 1.01), dict(directions=dirs[:, :2]), dict(microphonePositions=LINE[:1]),
                dict(microphonePositions=np.zeros((9, 3))), dict(microphonePositions=LINE * np.nan), dict(speedOfSound=0)):
        kw = dict(microphonePositions=LINE, directions=dirs, speedOfSound=SOUND)
        kw.update(bad)
        with pytest.raises(ValueError):
            pairTDOAsFromGeometry(**kw)


def test_steering_tables_are_stacked_by_pair():
    from gcc_nmf_amd.array import array_steering_tables
    from gcc_nmf_amd.engine import steering_tables
    F, Fp, D, Dp = 33, 48, 9, 64
    freqs = np.linspace(0, 8000, F)
    tau = A.pair_tdoas_from_geometry(LINE[:3], A.azimuth_directions(D), SOUND)
    trig = array_steering_tables(freqs, tau, Fp, Dp)
    assert trig.shape == (2, 3 * Fp, Dp) and trig.dtype == np.float32
    E = A.steering(freqs, tau)
    for p in range(3):
        blk = trig[:, p * Fp:(p + 1) * Fp]
        assert np.array_equal(blk, steering_tables(freqs, tau[p], Fp, Dp))
        assert np.abs(blk[0, :F, :D] - E[p].real).max() < 1e-7 and np.abs(blk[1, :F, :D] + E[p].imag).max() < 1e-7
        assert (blk[:, F:] == 0).all() and (blk[:, :, D:] == 0).all()


# ---- the synthetic line array ---------------------------------------------------------------------------------------------------------------
def test_array_mixture_and_the_restatements_peaks():
    from gcc_nmf_amd.synthetic import array_mixture
    x, images = array_mixture(0, LINE, [40, 90, 130], 16000, 16000, returnImages=True)
    assert x.shape == (4, 16000) and x.dtype == np.float32 and images.shape == (3, 4, 16000)
    assert np.array_equal(x * 32768, np.round(x * 32768)), 'int16-representable'
    assert np.array_equal(x, array_mixture(0, LINE, [40, 90, 130], 16000, 16000))
    assert not np.array_equal(x, array_mixture(1, LINE, [40, 90, 130], 16000, 16000))
    resid = x - images.sum(axis=0)
    assert np.std(resid) < 0.03 * np.std(x), 'the images add up to the mixture up to the sensor noise'
    # broadside talker (90 degrees): every microphone of a line along x hears the same signal
    assert np.abs(images[1] - images[1][0]).max() < 1e-12
    # end-fire component of the delay: microphone 3 (x = 1 m) hears the 40-degree talker EARLIER by cos(40) / c
    n = 16000
    shift = np.cos(np.deg2rad(40)) / SOUND
    f = np.fft.rfftfreq(n, 1 / 16000.0)
    moved = np.fft.irfft(np.fft.rfft(images[0][0]) * np.exp(2j * np.pi * f * shift), n)
    assert np.abs(moved - images[0][3]).max() < 1e-9
    _, X = line_spectrogram(0)
    _, Cs = A.features(X)
    tau = A.pair_tdoas_from_geometry(LINE, A.azimuth_directions(181), SOUND)
    freqs = np.linspace(0, 8000, 513)
    ang, _ = A.angular(Cs, freqs, tau)
    assert A.peaks(ang.mean(axis=1), 3) == ([40, 90, 130], 0)
    assert A.peaks(A.angular(Cs, freqs, -tau)[0].mean(axis=1), 3) == ([50, 90, 140], 0), 'the opposite sign mirrors the scan'


# ---- planted mistakes against the checks the device tests use --------------------------------------------------------------------------------
def test_planted_mistakes_fail_the_float64_checks():
    M, F, T, Kk, S, D = 3, 33, 20, 6, 3, 31
    Pn = 3
    X, W, H, am, masks = random_problem(M, F, T, Kk, S, 5)
    freqs = np.linspace(0, 8000, F)
    tau = A.pair_tdoas_from_geometry(LINE[:3], A.azimuth_directions(D), SOUND)
    _, Cs = A.features(X)
    ang, absprod = A.angular(Cs, freqs, tau)
    idx = [5, 14, 22]
    G, absG = A.scores(Cs, W, freqs, tau, idx)
    f32 = lambda a: np.asarray(a).astype(np.float32)
    C.check_gemm_like(f32(ang), ang, absprod, 2 * Pn * F, what='angular')
    C.check_gemm_like(f32(G), G, absG, Pn * F, what='scores')
    wrong_features = [A.features(X, A.pairs(M)[:-1])[1],                              # a pair left out
                      A.features(X, [(0, 2), (0, 1), (1, 2)])[1]]                     # pairs in another order
    wrong_features[0] = np.concatenate([wrong_features[0], np.zeros((1, F, T))])
    for name, Cw, tw in (('pair left out', wrong_features[0], tau), ('opposite sign', Cs, -tau), ('pair order', wrong_features[1], tau)):
        with pytest.raises(AssertionError):
            C.check_gemm_like(f32(A.angular(Cw, freqs, tw)[0]), ang, absprod, 2 * Pn * F, what=name)
        with pytest.raises(AssertionError):
            C.check_gemm_like(f32(A.scores(Cw, W, freqs, tw, idx)[0]), G, absG, Pn * F, what=name)
    # the reconstruction: |err| <= 2 (K + 4) u |X| (tests/test_gpu_array_stages.py states why)
    ref = A.ratio_one_hot(W, H, am, S, X)
    bound = np.broadcast_to(np.abs(X)[None], ref.shape)
    C.check_gemm_like(ref.astype(np.complex64), ref, bound, Kk, what='ratio')
    Tp = 64
    Hp = np.zeros((Kk, M * Tp), np.float32)
    Hp[:, :M * T] = H
    with pytest.raises(AssertionError):
        C.check_gemm_like(A.ratio_one_hot(W, Hp, am, S, X, stride=Tp).astype(np.complex64), ref, bound, Kk, what='H_c at c Tp')
    with pytest.raises(AssertionError):
        C.check_gemm_like(A.ratio_one_hot(W, H, am, S, X, targets=[0, 1]).astype(np.complex64), ref, bound, Kk, what='den over two targets')
    # the waveform check: a spectrogram slot swapped is outside the bar
    w = np.hanning(64).astype(np.float32)
    spec = (np.random.RandomState(2).randn(4, 33, 9) + 1j * np.random.RandomState(3).randn(4, 33, 9)).astype(np.complex64)
    y, bar = A.istft(spec, w, 64, 16, 0.5)
    assert y.shape == (4, 16 * 8) and (np.abs(y.astype(np.float32) - y) <= bar).all()
    assert not (np.abs(A.istft(spec[[1, 0, 2, 3]], w, 64, 16, 0.5)[0] - y) <= bar).all()
    ref_y = O.istft(spec[2], 16, 64, w) * 0.5
    assert np.abs(ref_y - y[2]).max() < 1e-5


# ---- the stacked cells of tests/test_gpu_stacked_pairs.py see the mistakes they are for --------------------------------------------------------
def failing(out, f, cell):
    """The names of the checks of stacked_pairs.checks() -- the functions the device test calls -- that `out` does not pass."""
    names = []
    for name, check in SP.checks(out, f, *cell[:6]):
        try:
            check()
        except AssertionError:
            names.append(name)
    return names


# cells 1, 3 and 4: the ring kernel with a k-tail, a scores reduction beyond the ring, no k-tail
PLANTED_CELLS = [(8, 33, 33, 3, 70, 5, 1, 2, 1), (7, 257, 33, 3, 64, 5, 1, 2, 1), (6, 41, 200, 4, 129, 65, 1, 1, 1)]


@pytest.mark.parametrize('cell', PLANTED_CELLS, ids=['M%d-F%d' % c[:2] for c in PLANTED_CELLS])
def test_stacked_cells_see_the_mistakes_they_are_for(cell):
    from gcc_nmf_amd.array import array_steering_tables
    assert SP.kernels(*cell) == SP.CELLS[cell]
    M, F, D, S, K, T = cell[:6]
    Pn, Fp, Fs = SP.shapes(M, F)
    assert Fp > F, 'a pitch of F differs from the pitch Fp'
    f = SP.host_file(M, F, D, S, K, T, 7 * F + M)
    trig = array_steering_tables(SP.frequencies(F), SP.pair_tdoas(M, D), Fp, SP.rup(D, 64))
    CC, Ws = SP.stacked_operands(f, Fp, SP.rup(K, 64), SP.rup(T, 64))
    assert CC.shape[1] == Pn * Fp == SP.rup(Fs, 16)
    run = lambda CC, Ws: failing(SP.evaluate(CC, trig, Ws, f['tdoa'], D, S, K, T), f, cell)
    assert run(CC, Ws) == [], 'the float64 evaluation of the stacked buffers, rounded to float32, passes every check'
    both = ['angular', 'steering', 'scores']
    # 1. two pairs exchanged (the second and the last)
    a, b = Fp, (Pn - 1) * Fp
    wrong = CC.copy()
    wrong[:, a:a + Fp], wrong[:, b:b + Fp] = CC[:, b:b + Fp], CC[:, a:a + Fp]
    assert run(wrong, Ws) == both
    # 2. pair blocks pitched by F where Fp is meant: the second block starts in the first one's padding rows (which stay zero in the
    #    steering products: the steering table is zero there)
    wrong = np.zeros_like(CC)
    for p in range(Pn):
        wrong[:, p * F:(p + 1) * F] = CC[:, p * Fp:p * Fp + F]
    assert run(wrong, Ws) == both
    # 3. the last pair's Nyquist bin dropped from the scores (the rank-1 k-tail term where the cell has one)
    wrong = Ws.copy()
    wrong[(Pn - 1) * Fp + F - 1] = 0
    assert run(CC, wrong) == ['scores']
    # 4. W copied under P - 1 of the P blocks
    wrong = Ws.copy()
    wrong[(Pn - 1) * Fp:] = 0
    assert run(CC, wrong) == ['scores']


def test_a_reused_second_accumulator_fails_the_ratio_check_at_five_targets():
    """tests/test_gpu_array_stages.py at S = 4 ... 7: target 4 of the row that carries targets g and g + 4 takes target 0's numerator."""
    M, F, T, Kk, S = 3, 33, 20, 16, 5
    X, W, H, am, masks = random_problem(M, F, T, Kk, S, 9)
    for form, mk, den in (('one-hot', A.one_hot(am, S), A.denominators(W, H, M, argmax=am, S=S)),
                          ('soft', masks, A.denominators(W, H, M, masks=masks))):
        num = A.numerators(W, H, mk, M)
        ref = A.ratio_one_hot(W, H, am, S, X) if form == 'one-hot' else A.ratio_soft(W, H, masks, X)
        bound = np.broadcast_to(np.abs(X)[None], ref.shape)
        assert np.array_equal(X[None] * (num / den[None]), ref)
        C.check_gemm_like(ref.astype(np.complex64), ref, bound, Kk, what=form)
        num[4] = num[0]
        wrong = (X[None] * (num / den[None])).astype(np.complex64)
        C.check_gemm_like(wrong[:4], ref[:4], bound[:4], Kk, what=form)
        with pytest.raises(AssertionError):
            C.check_gemm_like(wrong, ref, bound, Kk, what=form)


# ---- the mixtures of the engine tests at 5 to 8 microphones -------------------------------------------------------------------------------------
CASES_5_TO_8 = [(c, SP.ENGINE_CASES[c], SP.ENGINE_SHAPE) for c in SP.ENGINE_CASES] + [(SP.CORNER_CASE, SP.CORNER_SEED, SP.CORNER_SHAPE)]


@pytest.mark.parametrize('case,seed,shape', CASES_5_TO_8, ids=['M%d-b%d-S%d-n_fft%d' % (c + (s['n_fft'],)) for c, _, s in CASES_5_TO_8])
def test_the_restatement_alone_finds_the_talkers_of_the_engine_mixtures(case, seed, shape):
    """tests/test_gpu_array_engine.py asserts status == 0 for these files: a condition on the inputs, settled here without a device.  Every
    chosen peak stands above both neighbours by more than 2 % of the mean spectrum's range -- the float32 spectrogram is within
    2 (2 P F + 4) 2^-24 of the sum of moduli, a thousand times less."""
    M, B, S = case
    tau = SP.pair_tdoas(M, shape['D'])
    assert len({tuple(np.round(row * 1e9).astype(np.int64)) for row in np.concatenate([tau, -tau])}) == M * (M - 1), 'no two pair vectors are equal'
    xs = SP.engine_mixtures(M, B, S, seed, shape['n'])
    assert xs.shape == (B, M, shape['n'])
    for b in range(B):
        idx, status, clear = SP.reference_peaks(xs[b], shape['n_fft'], shape['hop'], shape['D'], S)
        print('M = %d file %d: peaks %s, the least clear one by %.3f of the range' % (M, b, idx, clear))
        assert status == 0 and idx == [13, 30, 43][:S] and clear > 0.02


# ---- the engine's argument rules: ValueError before a device is looked for ------------------------------------------------------------------
def test_constructor_argument_rules_need_no_device():
    from gcc_nmf_amd.array import GCCNMFArrayEngine, azimuthDirections
    dirs = azimuthDirections(31)
    tau4 = A.pair_tdoas_from_geometry(LINE, dirs, SOUND)
    ok = dict(n_samples=4096, numChannels=4, pairTDOAs=tau4, windowSize=256, hopSize=64, numTargets=2, dictionarySize=8, numIterations=2)
    bad = [dict(numChannels=1), dict(numChannels=9), dict(numChannels=2.0), dict(numChannels=True),
           dict(pairTDOAs=tau4[:5]), dict(pairTDOAs=tau4[0]), dict(pairTDOAs=np.where(np.arange(31) == 3, np.nan, tau4)),
           dict(pairTDOAs=np.where(np.arange(31) == 3, np.inf, tau4)), dict(pairTDOAs=tau4[:, :2]), dict(pairTDOAs=np.zeros((6, 4097))),
           dict(pairTDOAs=None), dict(pairTDOAs=None, microphonePositions=LINE), dict(pairTDOAs=None, directions=dirs),
           dict(pairTDOAs=None, microphonePositions=LINE[:3], directions=dirs),
           dict(pairTDOAs=None, microphonePositions=LINE, directions=dirs * 1.1),
           dict(pairTDOAs=None, microphonePositions=LINE, directions=dirs[:2]),
           dict(microphonePositions=LINE, directions=dirs),
           dict(numTargets=0), dict(numTargets=9), dict(numTargets=2.5), dict(numTargets='auto'),
           dict(windowSize=32), dict(windowSize=8192), dict(windowSize=1000), dict(windowSize=256.0),
           dict(n_samples=300)]
    for kw in bad:
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError):
            GCCNMFArrayEngine(**args)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        return                                       # (with a device the engine is exercised by the gpu tests)
    from gcc_nmf_amd.array import GCCNMFArrayEngine, azimuthDirections
    from gcc_nmf_amd._hip import HipLibraryError
    from gcc_nmf_amd import _array
    with pytest.raises(HipLibraryError):
        GCCNMFArrayEngine(4096, numChannels=4, microphonePositions=LINE, directions=azimuthDirections(31), windowSize=256, hopSize=64)
    with pytest.raises(HipLibraryError):
        _array.require_device()


# ---- the library --------------------------------------------------------------------------------------------------------------------------
def declared_functions(path):
    src = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(?:int|long)\s+(gccnmf_\w+)\s*\(', src)))


def test_header_ctypes_table_and_exported_symbols_agree():
    from gcc_nmf_amd import _array, _hip
    names = declared_functions(HEADER)
    assert names == sorted(_array.SIGNATURES) and len(names) == 3
    handle = ctypes.CDLL(_array.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), n
    image = open(_array.LIB_PATH, 'rb').read()
    exported = set(m.decode() for m in re.findall(rb'gccnmf_array_\w+', image))
    assert exported == set(names), 'libgccnmf_array.so carries other gccnmf_array_ names than its header declares: %s' % sorted(exported ^ set(names))
    assert b'gccnmf_set_tuning' not in image, 'the array library takes nothing from the separation library'
    assert not set(names) & set(_hip.SIGNATURES), 'the separation ABI stays as it is'
    assert _array.lib().gccnmf_array_version() >= 100
    src = open(HEADER).read()
    assert int(re.search(r'#define GCCNMF_ARRAY_MIN_CHANNELS (\d+)', src).group(1)) == _array.MIN_CHANNELS
    assert int(re.search(r'#define GCCNMF_ARRAY_MAX_CHANNELS (\d+)', src).group(1)) == _array.MAX_CHANNELS
    assert int(re.search(r'#define GCCNMF_ARRAY_MAX_TARGETS (\d+)', src).group(1)) == _array.MAX_TARGETS


def test_separation_header_still_declares_46_entry_points():
    """The product build's entry points, counted as tests/test_host.py counts them (without the GCCNMF_EXPERIMENTS blocks)."""
    from gcc_nmf_amd import _hip
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'gccnmf_hip.h')).read(), flags=re.S)
    src = re.sub(r'#ifdef GCCNMF_EXPERIMENTS.*?#endif', '', src, flags=re.S)
    names = sorted(set(re.findall(r'\b(?:int|long|gccnmf_allreduce_fn)\s+(gccnmf_\w+)\s*\(', src)))
    assert len(names) == 46 and names == sorted(_hip.SIGNATURES)
    assert not [n for n in names if n.startswith('gccnmf_array_')]


def test_array_source_includes_no_gemm_header():
    includes = lambda name: set(re.findall(r'#include\s+"([^"]+)"', open(os.path.join(REPO, 'gcc_nmf_amd', 'csrc', name)).read()))
    assert includes('array.hip') == {'common.h', 'ratio_kernel.h', 'phat.h', '../../include/gccnmf_array.h'}
    # the two headers it shares with the separation library bring in nothing else
    assert includes('ratio_kernel.h') == includes('phat.h') == {'common.h'}


ARG, UNSUPPORTED = 1, 3
PTR = 4096            # a non-null dummy: every rule is decided before the first HIP call


def test_features_argument_rules():
    from gcc_nmf_amd import _array
    f = _array.lib().gccnmf_array_features
    ok = dict(X=PTR, M=4, F=33, T=5, batch=2, V=PTR, CC=PTR)
    call = lambda **kw: f(*[dict(ok, **kw)[k] for k in ('X', 'M', 'F', 'T', 'batch', 'V', 'CC')], 0)
    for kw in (dict(M=1), dict(M=9), dict(M=0), dict(M=-2), dict(X=0), dict(V=0, CC=0), dict(F=1), dict(F=0), dict(T=0), dict(T=-1),
               dict(batch=0), dict(batch=-3)):
        assert call(**kw) == ARG, kw
    for kw in (dict(batch=65536), dict(M=8, F=4097), dict(T=(1 << 29))):
        assert call(**kw) == UNSUPPORTED, kw


def test_reconstruct_argument_rules():
    from gcc_nmf_amd import _array
    f = _array.lib().gccnmf_array_reconstruct
    ok = dict(W=PTR, H=PTR, argmax=PTR, masks=0, X=PTR, M=3, F=33, T=5, K=4, S=2, batch=2, pitch=6, spec=PTR)
    order = ('W', 'H', 'argmax', 'masks', 'X', 'M', 'F', 'T', 'K', 'S', 'batch', 'pitch', 'spec')
    call = lambda **kw: f(*[dict(ok, **kw)[k] for k in order], 0)
    for kw in (dict(W=0), dict(H=0), dict(argmax=0), dict(X=0), dict(spec=0), dict(M=1), dict(M=9), dict(F=1), dict(T=0), dict(K=0),
               dict(batch=0), dict(pitch=5), dict(pitch=0), dict(S=3)):
        assert call(**kw) == ARG, kw
    for kw in (dict(S=0), dict(S=9, pitch=27), dict(S=-1), dict(batch=21846), dict(T=(1 << 30))):
        assert call(**kw) == UNSUPPORTED, kw
