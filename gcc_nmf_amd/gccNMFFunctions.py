"""Drop-in replacement for the reference's ``gccNMF/gccNMFFunctions.py`` on MI355X.

Same function names, positional order, defaults, return shapes and dtypes as the
reference (each docstring cites the reference lines it replaces); NumPy arrays in,
NumPy arrays out.  The arithmetic of every function on the hot path runs in
libgccnmf_hip.so (hand-written gfx950 kernels, C ABI in include/gccnmf_hip.h);
there is no CPU fallback -- without the library or a GPU the functions raise
``HipLibraryError``.  Each call uploads its arguments and downloads its result;
use ``gcc_nmf_amd.engine.GCCNMFEngine`` to keep a whole batch resident in HBM.

The module-level NumPy names below are part of the interface: the reference's
driver does ``from gccNMFFunctions import *`` and then uses ``hanning``,
``linspace``, ``float32``, ``concatenate``, ``array``, ``hsplit``, ``mean`` ...
without importing them (gccNMF/runGCCNMF.py:27-46).
"""
import logging
from os.path import basename, join

import numpy as np
import torch
from numpy import hanning, array, squeeze, arange, concatenate, sqrt, sum, dot, newaxis, linspace, \
    exp, outer, pi, einsum, argsort, mean, hsplit, zeros, empty, min, max, isnan, all, nanargmax, empty_like, \
    where, zeros_like, angle, arctan2, int16, float32, complex64, argmax, take
from numpy.random import random, seed
from scipy.signal import argrelmax

from . import _hip, _staging
from .engine import (Geometry, padded, fft_twiddles, steering_tables, check_reconstruction, check_iterations, converge_klnmf,
                     klnmf_divergence, check_dictionary, semi_supervised_initial_factors)
from .librosaSTFT import stft, istft, ParameterError, _window_vector, _istft_device, _stft_device
from .wavfile import wavread, wavwrite

SPEED_OF_SOUND_IN_METRES_PER_SECOND = 340.29


def _device():
    if not torch.cuda.is_available():
        raise _hip.HipLibraryError('no ROCm device visible: gcc_nmf_amd has no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


# ---- pass-throughs (gccNMF/gccNMFFunctions.py:40-59) ------------------------------------------------
def getMixtureFileName(mixtureFileNamePrefix):
    return mixtureFileNamePrefix + '_mix.wav'


def getSourceEstimateFileName(mixtureFileNamePrefix, targetIndex):
    return mixtureFileNamePrefix + '_sim_%d.wav' % (targetIndex + 1)


def loadMixtureSignal(mixtureFileName):
    return wavread(mixtureFileName)


def getMaxTDOA(microphoneSeparationInMetres):
    return microphoneSeparationInMetres / SPEED_OF_SOUND_IN_METRES_PER_SECOND


def getTDOAsInSeconds(microphoneSeparationInMetres, numTDOAs):
    maxTDOA = getMaxTDOA(microphoneSeparationInMetres)
    return linspace(-maxTDOA, maxTDOA, numTDOAs)


def getFrequenciesInHz(sampleRate, numFrequencies):
    return linspace(0, sampleRate / 2, numFrequencies)


# ---- hot path ------------------------------------------------------------------------------------------
def set_resident(on):
    """Opt-in resident mode (``dropin.install(resident=True)``): every array a named function returns comes back READ-ONLY and the
    device image behind it is kept while the array lives; when the same object is passed to a later named function (X, W, the scores,
    the masks, the spectrogram estimates in runGCCNMF.py:36-52) its re-upload is skipped.  Default (off): writable outputs, every
    argument uploaded.  Same kernels, same results either way."""
    return _staging.set_resident(on)


def _trig_table(frequenciesInHz, microphoneSeparationInMetres, numTDOAs, g, dev):
    f = np.ascontiguousarray(frequenciesInHz, dtype=np.float64)
    key = ('trig', f.tobytes(), float(microphoneSeparationInMetres), int(numTDOAs), g.Fp, g.Dp)
    return _staging.constant(key, lambda: steering_tables(f, getTDOAsInSeconds(microphoneSeparationInMetres, numTDOAs), g.Fp, g.Dp), dev)


def computeComplexMixtureSpectrogram(stereoSamples, windowSize, hopSize, windowFunction, fftSize=None):
    """gccNMF/gccNMFFunctions.py:61-67.  Like the reference, ``windowFunction`` is ignored
    (numpy.hanning is hard-coded at :65), ``windowSize`` is the FFT length and ``fftSize`` the
    window length.  Returns (2, F, T) complex64.  Both channels share one packed complex FFT."""
    if fftSize is None:
        fftSize = windowSize
    chans = [np.ascontiguousarray(np.squeeze(stereoSamples[c])) for c in range(2)]       # (:64 copies each channel too)
    return _stft_device(chans[0], chans[1], windowSize, hopSize, fftSize, hanning, center=False, remember=True)


def performKLNMF(V, dictionarySize, numIterations, sparsityAlpha, epsilon=1e-16, seedValue=0):
    """gccNMF/gccNMFFunctions.py:69-83.  The initial W, H come from NumPy's GLOBAL legacy
    MT19937 exactly as in the reference (seed(seedValue); W first; :70-73) -- including the
    side effect on the global RNG state; the iteration loop (:75-81) runs on the GPU."""
    V = np.asarray(V)
    F, N = V.shape
    K = int(dictionarySize)
    lib, dev = _hip.lib(), _device()
    if N > LARGE_N_COLUMNS:
        return _performKLNMF_column_blocks(V, K, int(numIterations), float(sparsityAlpha), float(epsilon), seedValue, dev)
    init = _klnmf_initial_factors(F, N, K, epsilon, seedValue, dev)
    with _staging.Scope(dev) as sc:
        dV, dW, dH, ws = _klnmf_buffers(sc, lib, V, K, init)
        _hip.klnmf(dV, dW, dH, ws, F, N, K, 1, int(numIterations), float(sparsityAlpha), float(epsilon))
        W = sc.remember(sc.download(dW[:F, :K]), 'W', dict(W=dW), dict(F=F, K=K))
        H = sc.download(dH[:K, :N])
    return W, H


def performBetaNMF(V, dictionarySize, numIterations, beta, sparsityAlpha=0, epsilon=1e-16, seedValue=0):
    """NMF under one of the three classic beta-divergences (not in the reference, whose performKLNMF is beta = 1):
    ``beta`` = 0 or 'is' (Itakura-Saito), 1 or 'kl' (Kullback-Leibler), 2 or 'euclidean'.  Plain multiplicative updates in
    performKLNMF's structure -- with P = W.H:  H <- H o W^T(V o P^(beta-2)) / (W^T P^(beta-1) + sparsityAlpha + epsilon), the same for W
    without alpha and epsilon, then the unit-norm atoms and the compensating scale of H (gccNMFFunctions.py:75-81).  The initial factors
    are those performKLNMF draws (with its side effect on NumPy's global generator); beta = 1 IS performKLNMF, bit for bit.
    V is any non-negative (F, N) matrix: a magnitude spectrogram as everywhere in GCC-NMF, or -- the local Gaussian model behind
    Itakura-Saito NMF -- the power spectrogram |X|^2; that choice is the caller's.  IS needs V > 0 where the model is to fit (a zero of V
    pulls nothing: R = 0 there).  Returns float32 (W, H).  beta = 0, 2: F <= 2049, dictionarySize <= 1024, at most LARGE_N_COLUMNS
    columns (ValueError otherwise: the column-block path of a larger V is KL only)."""
    V = np.asarray(V)
    if V.ndim != 2:
        raise ValueError('V must be (F, N)')
    F, N = V.shape
    K = int(dictionarySize)
    d = _hip.check_divergence(beta, F, K)
    if d == 'kl':
        return performKLNMF(V, dictionarySize, numIterations, sparsityAlpha, epsilon, seedValue)
    if N > LARGE_N_COLUMNS:
        raise ValueError('performBetaNMF with beta = %r runs V as one call: at most %d columns, got %d (the column-block path is KL only)'
                         % (beta, LARGE_N_COLUMNS, N))
    lib, dev = _hip.lib(), _device()
    init = _klnmf_initial_factors(F, N, K, epsilon, seedValue, dev)
    with _staging.Scope(dev) as sc:
        dV, dW, dH, ws = _klnmf_buffers(sc, lib, V, K, init, d)
        _hip.klnmf(dV, dW, dH, ws, F, N, K, 1, int(numIterations), float(sparsityAlpha), float(epsilon), divergence=d)
        W = sc.remember(sc.download(dW[:F, :K]), 'W', dict(W=dW), dict(F=F, K=K))
        H = sc.download(dH[:K, :N])
    return W, H


def performTemporalKLNMF(V, dictionarySize, numIterations, sparsityAlpha, temporalContinuity, numSegments=1, epsilon=1e-16, seedValue=0):
    """performKLNMF with Virtanen's temporal-continuity term on H (IEEE TASLP 2007; not in the reference): the columns
    of V are ``numSegments`` (1 | 2: [L | R]) equal runs of frames, and inside each run every atom's gains pay
    ``temporalContinuity`` * T * sum_t (h_t - h_{t-1})^2 / sum_t h_t^2 -- an ABSOLUTE weight, in units of V -- beside the KL divergence and
    sparsityAlpha * sum H.  The H update is H <- H o (W^T(V / WH) + b Gm) / (colsum W + sparsityAlpha + b Gp + epsilon) with Gp - Gm the
    gradient of the cost; the W update and the normalisation are performKLNMF's.  The initial factors are those performKLNMF draws (with
    its side effect on NumPy's global generator); a weight of 0 IS performKLNMF, bit for bit.  Returns float32 (W, H).  A weight above 0:
    F <= 2049, dictionarySize <= 1024, an even column count for two segments (ValueError) and at most LARGE_N_COLUMNS columns
    (NotImplementedError: the column-block path of a larger V is plain KL only)."""
    V = np.asarray(V)
    if V.ndim != 2:
        raise ValueError('V must be (F, N)')
    F, N = V.shape
    K = int(dictionarySize)
    weight, segments = _hip.check_continuity(temporalContinuity, numSegments)
    if weight == 0:
        return performKLNMF(V, dictionarySize, numIterations, sparsityAlpha, epsilon, seedValue)
    if N > LARGE_N_COLUMNS:
        raise NotImplementedError('performTemporalKLNMF runs V as one call: at most %d columns, got %d (the column-block path is plain KL only)'
                                  % (LARGE_N_COLUMNS, N))
    _hip._continuity_words(weight, segments, F, N, K, 1, 0, False)      # the envelope, before a device is looked for
    lib, dev = _hip.lib(), _device()
    init = _klnmf_initial_factors(F, N, K, epsilon, seedValue, dev)
    with _staging.Scope(dev) as sc:
        dV, dW, dH, ws = _klnmf_buffers(sc, lib, V, K, init, continuity=True)
        _hip.klnmf(dV, dW, dH, ws, F, N, K, 1, int(numIterations), float(sparsityAlpha), float(epsilon), continuity=weight, segments=segments)
        W = sc.remember(sc.download(dW[:F, :K]), 'W', dict(W=dW), dict(F=F, K=K))
        H = sc.download(dH[:K, :N])
    return W, H


def getTemporalContinuity(H, numSegments=1):
    """The temporal-continuity cost of performTemporalKLNMF, summed over the atoms and segments of H (K, N) on the host in float64:
    sum of T * sum_t (h_t - h_{t-1})^2 / sum_t h_t^2 with T = N / numSegments; an all-zero row contributes 0."""
    H = np.asarray(H, np.float64)
    _, segments = _hip.check_continuity(0.0, numSegments)
    if H.ndim != 2 or H.shape[1] % segments:
        raise ValueError('H must be (K, N) with N a multiple of numSegments')
    K, N = H.shape
    h = H.reshape(K, segments, N // segments)
    E = (h * h).sum(2)
    D = (np.diff(h, axis=2) ** 2).sum(2)
    return float(((N // segments) * D[E > 0] / E[E > 0]).sum())


def _klnmf_initial_factors(F, N, K, epsilon, seedValue, dev):
    """Device images of performKLNMF's initial W and H (gccNMF/gccNMFFunctions.py:70-73), with the reference's side effect on the
    GLOBAL generator."""
    # The initial factors depend on (seedValue, F, K, N, epsilon) only, and so does the state the reference leaves the GLOBAL generator
    # in (seeded, advanced by F*K + K*N draws).  Drawn once per shape: later calls copy the device images and put the generator into
    # that same state (1.8 M MT19937 draws and 7 MB of upload are 5 ms of a 15 ms call at K = 1024).
    init_key = (F, N, K, repr(seedValue), float(epsilon), dev.index)
    init = _KLNMF_INIT.get(init_key) if seedValue is not None else None      # seed(None) draws fresh entropy: never cached
    if init is None:
        seed(seedValue)
        W = random((F, K)).astype(float32) + epsilon
        H = random((K, N)).astype(float32) + epsilon
        init = dict(W=torch.from_numpy(W.astype(float32)).to(dev), H=torch.from_numpy(H.astype(float32)).to(dev), state=np.random.get_state())
        if seedValue is not None:
            while len(_KLNMF_INIT) >= 4:
                _KLNMF_INIT.pop(next(iter(_KLNMF_INIT)))
            _KLNMF_INIT[init_key] = init
    else:
        np.random.set_state(init['state'])
    return init


def _klnmf_buffers(sc, lib, V, K, init, divergence='kl', continuity=False):
    """The padded device buffers of one batch-1 NMF call, loaded with V and the initial factors: (dV, dW, dH, workspace)."""
    F, N = V.shape
    g = Geometry(F, 1, K)
    Np = -(-N // 64) * 64
    # pooled padded buffers: the padding is zero and stays zero (uploads write the corner, the kernels never write beyond it)
    dV = sc.dev('V', (g.Fp, Np), corner=(F, N))
    dW = sc.dev('W', (g.Fp, g.Kp), corner=(F, K))
    dH = sc.dev('H', (g.Kp, Np), corner=(K, N))
    ws = sc.dev('ws_klnmf', (_hip.klnmf_continuity_workspace_floats(F, N, K, 1) if continuity else
                             _hip.klnmf_divergence_workspace_floats(F, N, K, 1, divergence),))
    dV[:F, :N].copy_(sc.upload(V, 'V', float32))
    dW[:F, :K].copy_(init['W'])
    dH[:K, :N].copy_(init['H'])
    return dV, dW, dH, ws


def performKLNMFUntilConverged(V, dictionarySize, maxIterations, sparsityAlpha, tolerance=1e-4, checkEvery=10, epsilon=1e-16, seedValue=0):
    """performKLNMF with a stopping rule (not in the reference, which runs a fixed count and never evaluates its objective; DESIGN
    section 2a): the same initial W and H (and the same side effect on the global generator), the same updates, run in chunks of
    ``checkEvery`` iterations -- the last one shorter where ``maxIterations`` cuts it -- with the KL divergence
    D(V || W.H) = sum V log(V / WH) - V + WH (a zero of V contributes WH alone) evaluated on the GPU after each.  The run stops at the
    first check with D_prev - D < tolerance * D_prev or D <= 0, D_prev of the first check being the divergence of the initial factors.
    A RISE of D stops the run too: that is intended for sparsityAlpha > 0, where the updates minimise D + alpha * sum(H) and D alone
    may go up.  A non-finite D stops nothing.  Returns (W, H, info), info = {'iterations': n, 'divergences': [(iteration, D), ...]}
    starting with (0, D of the initial factors).  W and H agree with performKLNMF(V, dictionarySize, n, ...) to round-off, not to the
    bit (H is rescaled by the atom norms in place between chunks instead of lazily).  One call's worth of columns only: V of more
    than LARGE_N_COLUMNS columns raises NotImplementedError.  (performBetaNMFUntilConverged is the same under the Itakura-Saito or the
    Euclidean divergence.)"""
    return _nmf_until_converged(V, dictionarySize, maxIterations, sparsityAlpha, tolerance, checkEvery, epsilon, seedValue, 'kl',
                                'performKLNMFUntilConverged', 'performKLNMF')


def performBetaNMFUntilConverged(V, dictionarySize, maxIterations, beta, sparsityAlpha=0, tolerance=1e-4, checkEvery=10, epsilon=1e-16,
                                 seedValue=0):
    """performKLNMFUntilConverged under the divergence ``beta`` names (performBetaNMF states the values): performBetaNMF's updates, stopped
    by THAT divergence (getBetaDivergence; for Itakura-Saito over the elements with V > 0) under the same rule.  beta = 1 is
    performKLNMFUntilConverged.  Returns (W, H, info) likewise."""
    return _nmf_until_converged(V, dictionarySize, maxIterations, sparsityAlpha, tolerance, checkEvery, epsilon, seedValue,
                                _hip.check_divergence(beta, np.shape(V)[0] if np.ndim(V) == 2 else None, int(dictionarySize)),
                                'performBetaNMFUntilConverged', 'performBetaNMF')


def _nmf_until_converged(V, dictionarySize, maxIterations, sparsityAlpha, tolerance, checkEvery, epsilon, seedValue, divergence, name, fixed_name):
    tolerance, checkEvery, maxIterations = _hip.check_convergence(tolerance, checkEvery, maxIterations)
    if tolerance is None:
        raise ValueError('%s needs a tolerance; %s runs a fixed number of iterations' % (name, fixed_name))
    V = np.asarray(V)
    F, N = V.shape
    K = int(dictionarySize)
    if N > LARGE_N_COLUMNS:
        raise NotImplementedError('%s runs V as one call: at most %d columns, got %d (performKLNMF takes such a V '
                                  'as column blocks, without a stopping rule)' % (name, LARGE_N_COLUMNS, N))
    lib, dev = _hip.lib(), _device()
    init = _klnmf_initial_factors(F, N, K, epsilon, seedValue, dev)
    with _staging.Scope(dev) as sc:
        dV, dW, dH, ws = _klnmf_buffers(sc, lib, V, K, init, divergence)

        def launch(n, first):
            _hip.klnmf(dV, dW, dH, ws, F, N, K, 1, n, float(sparsityAlpha), float(epsilon), divergence=divergence)
        iterations, trace = converge_klnmf(launch, lambda: klnmf_divergence(dV, dW, dH, ws, F, N, K, 1, divergence=divergence).cpu().numpy(),
                                           [dW.unsqueeze(0), dH.unsqueeze(0)], maxIterations, tolerance, checkEvery)
        W = sc.remember(sc.download(dW[:F, :K]), 'W', dict(W=dW), dict(F=F, K=K))
        H = sc.download(dH[:K, :N])
    checks = check_iterations(trace, checkEvery, maxIterations)      # (this module's min / max are NumPy's: the reference's star import)
    return W, H, dict(iterations=int(iterations[0]), divergences=[(it, float(d[0])) for it, d in zip(checks, trace)])


def performSemiSupervisedKLNMF(V, dictionaryW, numFreeAtoms, numIterations, sparsityAlpha, epsilon=1e-16, seedValue=0):
    """Semi-supervised KL-NMF (not in the reference): performKLNMF's iteration with the pre-trained ``dictionaryW``
    (F, K_fixed) kept as it is -- bit for bit, not normalised -- in the first columns of W, and ``numFreeAtoms`` free atoms learned from
    V beside it, with the coefficients of all K = K_fixed + numFreeAtoms atoms (gccnmf_klnmf with GCCNMF_FLAG_FREE_ATOMS).  The
    initial factors are the engine's (GCCNMFEngine(dictionaryW=, numFreeAtoms=)): with W0, H0 = klnmf_initial_factors(F, N, K, epsilon,
    seedValue), the free atoms start as W0[:, K_fixed:] and H as H0 (a generator of its own: no side effect on NumPy's global one).
    Returns float32 (W, H) of shapes (F, K) and (K, N).  K_fixed a multiple of 16, numFreeAtoms in [1, 128], K <= 1024, F <= 2049, else
    ValueError.  One call's worth of columns only: V of more than LARGE_N_COLUMNS columns raises NotImplementedError."""
    V = np.asarray(V)
    if V.ndim != 2:
        raise ValueError('V must be (F, N)')
    F, N = V.shape
    Wfix = check_dictionary(dictionaryW, F)
    n = _hip.check_free_atoms(numFreeAtoms, Wfix.shape[1], F)
    if n == 0:
        raise ValueError('performSemiSupervisedKLNMF needs at least one free atom (inferKLNMFCoefficients takes a dictionary alone)')
    if N > LARGE_N_COLUMNS:
        raise NotImplementedError('performSemiSupervisedKLNMF runs V as one call: at most %d columns, got %d' % (LARGE_N_COLUMNS, N))
    K = Wfix.shape[1] + n
    lib, dev = _hip.lib(), _device()
    W0, H0 = semi_supervised_initial_factors(Wfix, n, N, epsilon, seedValue)
    init = dict(W=torch.from_numpy(W0).to(dev), H=torch.from_numpy(H0).to(dev))
    with _staging.Scope(dev) as sc:
        dV, dW, dH, ws = _klnmf_buffers(sc, lib, V, K, init)
        _hip.klnmf(dV, dW, dH, ws, F, N, K, 1, int(numIterations), float(sparsityAlpha), float(epsilon), free_atoms=n)
        W = sc.remember(sc.download(dW[:F, :K]), 'W', dict(W=dW), dict(F=F, K=K))
        H = sc.download(dH[:K, :N])
    return W, H


def getKLDivergence(V, W, H):
    """The objective of performKLNMF, which the reference never evaluates: D(V || W.H) = sum V log(V / WH) - V + WH over every element
    (a zero of V contributes WH alone), as a float64 scalar.  W.H runs in float32 on the matrix cores and is never stored; the terms
    are summed in float64 (gccnmf_klnmf_stage, stage 7: csrc/divergence.hip).  V (F, N), W (F, K), H (K, N)."""
    return _beta_divergence(V, W, H, 'kl', 'getKLDivergence')


def getBetaDivergence(V, W, H, beta):
    """The objective of performBetaNMF as a float64 scalar, with R = W.H in float32 on the matrix cores (never stored) and the terms
    summed in float64 (gccnmf_klnmf_stage, stage 7).  ``beta`` = 1 / 'kl': getKLDivergence.  0 / 'is': sum of V / R - log(V / R) - 1 over
    the elements with V > 0 -- IS is +infinity at a zero of V, so such an element contributes NOTHING and the value is the divergence over
    the support of V.  2 / 'euclidean': sum of (V - R)^2 / 2.  V (F, N), W (F, K), H (K, N)."""
    return _beta_divergence(V, W, H, _hip.check_divergence(beta), 'getBetaDivergence')


def _beta_divergence(V, W, H, divergence, name):
    V, H = np.asarray(V), np.asarray(H)
    if V.ndim != 2 or np.ndim(W) != 2 or H.ndim != 2 or np.shape(W) != (V.shape[0], H.shape[0]) or H.shape[1] != V.shape[1]:
        raise ValueError('%s takes V (F, N), W (F, K) and H (K, N), got %s, %s, %s' % (name, V.shape, np.shape(W), H.shape))
    F, N = V.shape
    K = H.shape[0]
    lib, dev = _hip.lib(), _device()
    g = Geometry(F, 1, K)
    Np = -(-N // 64) * 64
    with _staging.Scope(dev) as sc:
        dV = sc.dev('V', (g.Fp, Np), corner=(F, N))
        dH = sc.dev('H', (g.Kp, Np), corner=(K, N))
        ws = sc.dev('ws_klnmf', (lib.gccnmf_klnmf_workspace_floats(F, N, K, 1),))
        dV[:F, :N].copy_(sc.upload(V, 'V', float32))
        dH[:K, :N].copy_(sc.upload(H, 'H', float32))
        dW = _device_W(sc, W, g, dev)                      # the image behind W if performKLNMF returned it (resident mode)
        out = sc.download(klnmf_divergence(dV, dW, dH, ws, F, N, K, 1, divergence=divergence))
    return np.float64(out[0])


_KLNMF_INIT = {}             # (F, N, K, seed, epsilon, device) -> device images of the initial factors + the generator state, a few shapes

# One BIG matrix (the dictionary pre-training set, gccNMF/realtime/gccNMFPretraining.py:79-80: performKLNMF on thousands of frames):
# beyond this many columns the launch fills the chip by itself, and the columns are handed to the batched throughput kernels IN PLACE
# as column blocks of one matrix (gccnmf_klnmf_shared_run with ld > 0 -- the machinery of the time-sharded mode, one rank, no
# collective) instead of the one-mixture latency path.  Same update (gccNMFFunctions.py:75-81): W's numerator sums over all blocks.
LARGE_N_COLUMNS = 4096


def _performKLNMF_column_blocks(V, K, numIterations, sparsityAlpha, epsilon, seedValue, dev):
    from .distributed import HipSharedColumns
    F, N = V.shape
    g = Geometry(F, 1, K)
    ld = -(-N // 64) * 64
    seed(seedValue)                                     # the reference's draws, W before H, and its side effect on the global generator
    W0 = random((F, K)).astype(float32) + epsilon
    H0 = random((K, N)).astype(float32) + epsilon
    with torch.cuda.device(dev):
        Vd = padded(np.ascontiguousarray(V, dtype=float32), (g.Fp, ld), dev)
        Wd = padded(W0.astype(float32), (g.Fp, g.Kp), dev)
        Hd = padded(H0.astype(float32), (g.Kp, ld), dev)
        run = HipSharedColumns(Vd, Hd, Wd, F, N, K, sparsityAlpha, epsilon)
        run.run(numIterations, collective=False)        # this call's columns only, whatever process group the caller may have set up
        return Wd[:F, :K].cpu().numpy(), Hd[:K, :N].cpu().numpy()


def _upload_coherence(sc, C, g):
    """(F, T) complex coherence -> the padded [2][Fp][Tp] Re / Im planes the angular and score GEMMs read (one contiguous upload, the
    de-interleave happens on the device)."""
    F, T = C.shape
    dC = sc.dev('CC', (2, g.Fp, g.Tp), corner=(F, T))
    up = sc.upload(C, 'C', complex64)
    dC[:, :F, :T].copy_(torch.view_as_real(up).permute(2, 0, 1))
    return dC


def _device_W(sc, W, g, dev):
    """Padded device image of a dictionary: the one behind the array if performKLNMF returned it (resident mode), else an upload."""
    rec = _staging.lookup(W, 'W', dev)
    if rec is not None and rec.meta == dict(F=g.F, K=g.K):
        return rec.tensors['W']
    dW = sc.dev('W', (g.Fp, g.Kp), corner=(g.F, g.K))
    dW[:g.F, :g.K].copy_(sc.upload(W, 'W', float32))
    return dW


def getAngularSpectrogram(spectralCoherenceV, frequenciesInHz, microphoneSeparationInMetres, numTDOAs, gccPHATNLEnabled=False,
                          gccPHATNLAlpha=2.0):
    """gccNMF/gccNMFFunctions.py:85-92.  Returns (numTDOAs, T) float64 like the reference; the
    contraction itself is an f32 MFMA GEMM [cos;sin]^T.[Re C;Im C].

    ``gccPHATNLEnabled`` / ``gccPHATNLAlpha`` (trailing keywords, the reference's setting names, realtime/config.py:42-43): the
    GCC-NONLIN spectrum sum_f 1 - tanh(alpha sqrt(max(0, 1 - Re(C e^{-j 2 pi f tau})))) of Blandin, Ozerov & Vincent (2012) instead,
    a VALU kernel (csrc/angular_nl.hip).  BSS-Locate's sqrt(2 - 2 re) form is this one with alpha * sqrt(2)."""
    nl, alpha = _hip.check_gcc_phat_nl(gccPHATNLEnabled, gccPHATNLAlpha)
    C = np.asarray(spectralCoherenceV)
    F, T = C.shape
    _, dev = _hip.lib(), _device()
    g = Geometry(F, T, 1, int(numTDOAs))
    trig = _trig_table(frequenciesInHz, microphoneSeparationInMetres, numTDOAs, g, dev)
    with _staging.Scope(dev) as sc:
        dC = _upload_coherence(sc, C, g)
        ang = sc.dev('ang', (g.Dp, g.Tp))
        _hip.angular_spectrogram(dC, trig, F, T, g.D, 1, ang, None, nl_alpha=alpha if nl else None)
        out = sc.download(ang[:g.D, :T], dtype=np.float64)
    return out


MAX_AUTO_SOURCES = _hip.MAX_AUTO_SOURCES      # the cap of numSources='auto'


def _report_auto_sources(count, status, maxSources, where):
    """What the named functions do with a count: status 1 is the reference's failure, status 2 is logged."""
    if status == 1:
        raise ValueError("didn't find enough peaks in %s" % where)
    if status == 2:
        logging.info('more than %d sources found, keeping the %d highest peaks' % (maxSources, maxSources))
    logging.info('numSources not provided, found %d sources' % count)


def estimateNumSourcesFromAngularSpectrum(angularSpectrum, maxSources=MAX_AUTO_SOURCES):
    """How many sources a mean angular spectrum shows (the count mode of gccnmf_pick_tdoa_peaks, csrc/source_count.hip; DESIGN section
    4f): the exact two-cluster k-means split of the heights of its strict local maxima, the upper cluster kept -- what the reference's
    ``numSources=None`` branch declares with KMeans(n_clusters=2) (gccNMFFunctions.py:105-110).  Returns (count, indexes, status):
    ``indexes`` the sorted list of the ``count`` kept peaks (np.int64), ``status`` 0, 1 (no peak, or heights without a finite sum:
    count 0) or 2 (more than ``maxSources`` found: the highest ``maxSources`` kept)."""
    _hip.check_auto_sources('auto', maxSources)
    spectrum = np.ascontiguousarray(angularSpectrum, dtype=np.float64)
    if spectrum.ndim != 1:
        raise ValueError('angularSpectrum must be one-dimensional (the time mean), got shape %s' % (spectrum.shape,))
    D, S = spectrum.shape[0], int(maxSources)
    _, dev = _hip.lib(), _device()
    with _staging.Scope(dev) as sc:
        dM = sc.upload(spectrum, 'meanA')
        res = sc.dev('counted', (S + 1,), torch.int32)                # [0..S): indexes, [S]: status
        _hip.count_tdoa_peaks(dM, D, D, S, 1, res, res.data_ptr() + 4 * S)
        out = sc.download(res)
    indexes = sorted(np.int64(i) for i in out[:S] if i >= 0)
    return len(indexes), indexes, int(out[S])


def estimateTargetTDOAIndexesFromAngularSpectrum(angularSpectrum, microphoneSeparationInMetres, numTDOAs, numSources):
    """gccNMF/gccNMFFunctions.py:94-116: strict local maxima, top ``numSources`` by value, sorted
    ascending.  The reference's failure branches are NameErrors (:104 ``os``, :106 ``KMeans``);
    here they raise ValueError.  ``numSources='auto'``: what the :105-110 branch was meant to return -- the peaks of the upper of two
    height clusters, MAX_AUTO_SOURCES at the most (estimateNumSourcesFromAngularSpectrum); None and 0 keep raising."""
    if _hip.check_auto_sources(numSources, MAX_AUTO_SOURCES):
        count, sourcePeakIndexes, status = estimateNumSourcesFromAngularSpectrum(angularSpectrum, MAX_AUTO_SOURCES)
        _report_auto_sources(count, status, MAX_AUTO_SOURCES, 'estimateTargetTDOAIndexesFromAngularSpectrum')
        logging.info('Found target TDOAs: %s' % str(sourcePeakIndexes))
        return sourcePeakIndexes
    if not numSources:
        raise ValueError('numSources is required (the reference KMeans branch cannot run: gccNMFFunctions.py:106)')
    spectrum = np.ascontiguousarray(angularSpectrum, dtype=np.float64)
    D = spectrum.shape[0]
    S = int(numSources)
    _, dev = _hip.lib(), _device()
    logging.info('numSources provided, taking first %d peaks' % numSources)
    with _staging.Scope(dev) as sc:
        dM = sc.upload(spectrum, 'meanA')
        res = sc.dev('peaks', (S + 1,), torch.int32)                  # [0..S): indexes, [S]: status
        _hip.pick_tdoa_peaks(dM, D, D, S, 1, res, res.data_ptr() + 4 * S)
        out = sc.download(res)
    if int(out[S]) != 0:
        raise ValueError("didn't find enough peaks in estimateTargetTDOAIndexesFromAngularSpectrum")
    sourcePeakIndexes = sorted(np.int64(i) for i in out[:S])
    logging.info('Found target TDOAs: %s' % str(sourcePeakIndexes))
    return sourcePeakIndexes


def check_target_tdoa_indexes(targetTDOAIndexes, numTime):
    """The ``targetTDOAIndexes`` argument of getTargetTDOAGCCNMFs, no device needed: the reference's 1-D list (one index per target) or
    a 2-D (numTargets, T) array of per-frame indexes (estimateTargetTDOATracksFromAngularSpectrogram).  Returns (int32 array, tracks?)."""
    idx = np.asarray(targetTDOAIndexes)
    if idx.ndim not in (1, 2) or idx.size == 0 or not 1 <= idx.shape[0] <= 255:
        raise ValueError('targetTDOAIndexes must be a list of 1 to 255 indexes or a (numTargets, T) array, got shape %s' % (idx.shape,))
    if idx.dtype.kind not in 'iu':
        if idx.dtype.kind != 'f' or not np.array_equal(idx, np.round(idx)):
            raise ValueError('targetTDOAIndexes must be whole numbers')
    if idx.ndim == 2 and idx.shape[1] != int(numTime):
        raise ValueError('per-frame targetTDOAIndexes must have one column per frame: expected (numTargets, %d), got %s' % (numTime, idx.shape))
    return np.ascontiguousarray(idx, dtype=np.int32), idx.ndim == 2


def check_angular_spectrogram_for_tracks(angularSpectrogram, numTDOAs, numSources, localizationWindowSize):
    """Arguments of estimateTargetTDOATracksFromAngularSpectrogram, no device needed.  Returns (float32 (D, T) array, S, L)."""
    _, L = _hip.check_tdoa_tracking(True, localizationWindowSize, numSources)
    A = np.asarray(angularSpectrogram)
    if A.ndim != 2 or A.dtype.kind not in 'fiu' or not 3 <= A.shape[0] <= 4096 or not 1 <= A.shape[1] <= _hip.TRACKS_MAX_FRAMES:
        raise ValueError('angularSpectrogram must be a real (numTDOAs, T) array with 3 <= numTDOAs <= 4096, got %s %s' % (A.dtype, A.shape))
    if numTDOAs is not None and int(numTDOAs) != A.shape[0]:
        raise ValueError('angularSpectrogram has %d rows, numTDOAs is %r' % (A.shape[0], numTDOAs))
    return np.ascontiguousarray(A, dtype=np.float32), int(numSources), L


def estimateTargetTDOATracksFromAngularSpectrogram(angularSpectrogram, microphoneSeparationInMetres, numTDOAs, numSources,
                                                   localizationWindowSize):
    """Time-varying twin of estimateTargetTDOAIndexesFromAngularSpectrum (not in the reference): for every frame t
    the ``numSources`` largest strict local maxima of mean(angularSpectrogram[:, lo:hi], axis=-1) over the centred window lo = max(0, t -
    L // 2), hi = min(T, t - L // 2 + L), L = ``localizationWindowSize`` frames, ascending.  A frame with fewer peaks takes the previous
    frame's set (the frames in front of the first complete one take that one's); no complete frame at all raises ValueError.  Target i is
    a frame's i-th peak from the left: talkers whose directions cross swap rows.  The spectrogram is taken as float32 (what
    getAngularSpectrogram computes); the window sums are float64.  Returns an int64 (numSources, T) array -- pass it to
    getTargetTDOAGCCNMFs as ``targetTDOAIndexes``."""
    A, S, L = check_angular_spectrogram_for_tracks(angularSpectrogram, numTDOAs, numSources, localizationWindowSize)
    D, T = A.shape
    _, dev = _hip.lib(), _device()
    g = Geometry(2, T, 1, D, S)
    with _staging.Scope(dev) as sc:
        ang = sc.dev('ang', (g.Dp, g.Tp), corner=(D, T))
        ang[:D, :T].copy_(sc.upload(A, 'A', float32))
        res = sc.dev('tracks', (S + 1, g.Tp), torch.int32)              # rows [0..S): tracks, row S: per-frame status
        _hip.pick_tdoa_tracks(ang, D, T, S, L, 1, res, res.data_ptr() + 4 * S * g.Tp)
        out = sc.download(res[:, :T])
    if (out[S] & 2).any():
        raise ValueError("didn't find enough peaks in any frame in estimateTargetTDOATracksFromAngularSpectrogram")
    return out[:S].astype(np.int64)


def getTargetTDOAGCCNMFs(coherenceV, microphoneSeparationInMetres, numTDOAs, frequenciesInHz, targetTDOAIndexes, W, stereoH):
    """gccNMF/gccNMFFunctions.py:118-135.  Returns (numTargets, K, T) float32.  ``targetTDOAIndexes``: the reference's list of one
    index per target, or a 2-D (numTargets, T) array of per-frame indexes (estimateTargetTDOATracksFromAngularSpectrogram): atom k of
    frame t is then scored against tau[i, t]."""
    C = np.asarray(coherenceV)
    F, T = C.shape
    targetTDOAIndexes, tracks = check_target_tdoa_indexes(targetTDOAIndexes, T)
    numTargets = targetTDOAIndexes.shape[0]
    numChannels, K, numTime = stereoH.shape
    lib, dev = _hip.lib(), _device()
    g = Geometry(F, T, K, int(numTDOAs), numTargets)
    trig = _trig_table(frequenciesInHz, microphoneSeparationInMetres, numTDOAs, g, dev)
    with _staging.Scope(dev) as sc:
        dC = _upload_coherence(sc, C, g)
        dW = _device_W(sc, W, g, dev)
        if tracks:
            dIdx = sc.dev('idx_tracks', (numTargets, g.Tp), torch.int32, corner=(numTargets, T))
            dIdx[:, :T].copy_(sc.upload(targetTDOAIndexes, 'idx', np.int32))
        else:
            dIdx = sc.upload(targetTDOAIndexes, 'idx')
        ws = sc.dev('ws_scores', (lib.gccnmf_scores_workspace_floats(F, T, numTargets, 1),))
        scores = sc.dev('scores', (g.Kp, numTargets, g.Tp))
        _hip.target_scores_masks(dC, trig, dIdx, dW, F, T, K, g.D, numTargets, 1, ws, scores, None, tracks=tracks)
        out = sc.download(scores[:K, :, :T].permute(1, 0, 2), shape=(numTargets, K, T))
        sc.remember(out, 'G', dict(scores=scores), dict(S=numTargets, K=K, T=T))
    return out


def getTargetCoefficientMasks(targetTDOAGCCNMFs, numTargets):
    """gccNMF/gccNMFFunctions.py:137-143: one-hot of nanargmax over targets (first wins ties);
    only the first ``numTargets`` masks are filled, as in the reference loop."""
    G = np.asarray(targetTDOAGCCNMFs)
    S, K, T = G.shape
    _, dev = _hip.lib(), _device()
    g = Geometry(2, T, K, 1, S)
    with _staging.Scope(dev) as sc:
        rec = _staging.lookup(G, 'G', dev)
        if rec is not None:
            scores = rec.tensors['scores']
        else:
            scores = sc.dev('scores', (g.Kp, S, g.Tp), corner=(K, S, T))
            scores[:K, :, :T].copy_(sc.upload(G, 'G', float32).permute(1, 0, 2))
        am = sc.dev('argmax', (g.Kp, g.Tp), torch.uint8)
        _hip.argmax_targets(scores, K, T, S, 1, am)
        # numpy.nanargmax raises on a slice that is NaN for every target (:138); argument validation, checked where the data is
        allnan = torch.isnan(scores[:K, :, :T]).all(dim=1).any()
        # the reference's loop (:140-142): masks[i][argmax == i] = 1 for i < numTargets -- an exact 0 / 1 format expansion of the arg-max image
        targets = torch.arange(S, device=dev, dtype=torch.uint8)
        targets[int(numTargets):] = 255
        onehot = am[:K, :T].unsqueeze(0) == targets.view(S, 1, 1)
        masks = sc.download(onehot, shape=(S, K, T), dtype=G.dtype if G.dtype in (np.float32, np.float64) else np.float32)
        bad = sc.download(allnan.view(1).to(torch.uint8))
        if int(numTargets) >= S:
            sc.remember(masks, 'M', dict(argmax=am), dict(S=S, K=K, T=T))
    if bad[0]:
        raise ValueError('All-NaN slice encountered')          # numpy.nanargmax behaviour (:138)
    return masks


def check_atom_tdoa_arguments(coherenceV, numTDOAs, frequenciesInHz, W):
    """Arguments of getAtomTDOAIndexes, no device needed.  Returns (C (F, T), W (F, K), numTDOAs)."""
    C, W = np.asarray(coherenceV), np.asarray(W)
    if C.ndim != 2 or C.dtype.kind not in 'cfiu' or C.shape[0] < 2 or C.shape[1] < 1:
        raise ValueError('coherenceV must be an (F, T) array with F >= 2 and T >= 1, got %s %s' % (C.dtype, C.shape))
    if W.ndim != 2 or W.dtype.kind not in 'fiu' or W.shape[0] != C.shape[0] or W.shape[1] < 1:
        raise ValueError('W must be a real (%d, K) array, got %s %s' % (C.shape[0], W.dtype, W.shape))
    if isinstance(numTDOAs, bool) or int(numTDOAs) != numTDOAs or not 1 <= int(numTDOAs) <= _hip.ATOM_TDOA_MAX_D:
        raise ValueError('numTDOAs must be a whole number from 1 to %d, got %r' % (_hip.ATOM_TDOA_MAX_D, numTDOAs))
    if np.size(frequenciesInHz) != C.shape[0]:
        raise ValueError('frequenciesInHz must have one entry per row of coherenceV (%d), got %d' % (C.shape[0], np.size(frequenciesInHz)))
    return C, W, int(numTDOAs)


def getAtomTDOAIndexes(coherenceV, microphoneSeparationInMetres, numTDOAs, frequenciesInHz, W):
    """Every atom's own TDOA in every frame (not in the reference's offline module; the streaming processor computes it per frame,
    gccNMF/realtime/gccNMFProcessor.py:254,:259): argmax over the WHOLE grid of sum_f W[f, k] Re(C[f, t] exp(-2j pi f tau_d)).  First
    index wins an exact tie, NaN scores are ignored, an all-NaN column gives 0.  Returns an int64 (K, T) array.  No (K, numTDOAs, T)
    array is formed anywhere: the scores live in matrix-core accumulators (csrc/atom_tdoa.hip)."""
    C, W, D = check_atom_tdoa_arguments(coherenceV, numTDOAs, frequenciesInHz, W)
    F, T = C.shape
    K = W.shape[1]
    _, dev = _hip.lib(), _device()
    g = Geometry(F, T, K, D)
    trig = _trig_table(frequenciesInHz, microphoneSeparationInMetres, D, g, dev)
    with _staging.Scope(dev) as sc:
        dC = _upload_coherence(sc, C, g)
        dW = _device_W(sc, W, g, dev)
        atom = sc.dev('atom_tdoa', (g.Kp, g.Tp), torch.int16)
        _hip.atom_tdoa_indexes(dC, trig, dW, F, T, K, D, 1, atom)
        out = sc.download(atom[:K, :T].to(torch.int32) & 0xffff)
    return out.astype(np.int64)


def check_enhancement_mask_arguments(atomTDOAIndexes, targetTDOAIndex):
    """Arguments of getEnhancementCoefficientMasks, no device needed.  Returns (uint16 (K, T) indexes, int32 target array, per frame?)."""
    A = np.asarray(atomTDOAIndexes)
    if A.ndim != 2 or A.size == 0 or A.dtype.kind not in 'iu' or A.min() < 0 or A.max() > 65535:
        raise ValueError('atomTDOAIndexes must be a (K, T) array of whole numbers in [0, 65535], got %s %s' % (A.dtype, A.shape))
    tg = np.asarray(targetTDOAIndex)
    if tg.ndim not in (0, 1) or tg.dtype.kind not in 'iuf' or (tg.ndim == 1 and tg.shape[0] != A.shape[1]):
        raise ValueError('targetTDOAIndex must be a number or one number per frame (%d), got shape %s' % (A.shape[1], tg.shape))
    if not np.isfinite(tg).all() or not np.array_equal(tg, np.round(tg)) or np.abs(tg).max() >= 2 ** 24:
        raise ValueError('targetTDOAIndex must be whole numbers')
    return np.ascontiguousarray(A, dtype=np.uint16), np.ascontiguousarray(np.atleast_1d(tg), dtype=np.int32), tg.ndim == 1


def getEnhancementCoefficientMasks(atomTDOAIndexes, targetTDOAIndex, targetMode=_hip.TARGET_MODE_WINDOW_FUNCTION, targetTDOAEpsilon=5.0,
                                   targetTDOABeta=2.0, targetTDOANoiseFloor=0.0):
    """The talker's and the noise's coefficient masks of offline speech enhancement, [talker, noise] = (m, 1 - m), from every atom's own
    TDOA index i (getAtomTDOAIndexes) and the talker's ``targetTDOAIndex`` (a number, or one per frame):
        TARGET_MODE_BOXCAR           m = |i - target| < epsilon                                          (realtime/gccNMFProcessor.py:263)
        TARGET_MODE_WINDOW_FUNCTION  m = exp(-(|i - target| / epsilon) ** beta) / (1 + noiseFloor) + noiseFloor, unclamped     (:265)
    ``targetMode``: the constants realtime.py exports (or 'boxcar' / 'window'); the defaults are the reference's (processor :193,
    realtime/config.py:56-58).  Returns float32 (2, K, T): pass it to getTargetSpectrogramEstimates as its masks."""
    window, eps, beta, nf = _hip.check_enhancement_target(targetMode, targetTDOAEpsilon, targetTDOABeta, targetTDOANoiseFloor)
    A, tg, per_frame = check_enhancement_mask_arguments(atomTDOAIndexes, targetTDOAIndex)
    K, T = A.shape
    _, dev = _hip.lib(), _device()
    g = Geometry(2, T, K, 1, 2)
    with _staging.Scope(dev) as sc:
        atom = sc.dev('atom_tdoa', (g.Kp, g.Tp), torch.int16, corner=(K, T))
        atom[:K, :T].copy_(sc.upload(A.view(np.int16), 'atom', np.int16))
        if per_frame:
            dT = sc.dev('target_tracks', (g.Tp,), torch.int32, corner=(T,))
            dT[:T].copy_(sc.upload(tg, 'target', np.int32))
        else:
            dT = sc.upload(tg, 'target', np.int32)
        image = sc.dev('argmax', (g.Kp, g.Tp), torch.uint8)
        dM = sc.dev('enh_masks', (2, g.Kp, g.Tp))
        _hip.enhancement_masks(atom, dT, T, K, 1, image, dM, window=window, eps=eps, beta=beta, noise_floor=nf, per_frame=per_frame)
        masks = sc.download(dM[:, :K, :T], shape=(2, K, T))
        if not window:                   # resident mode: the reconstruction takes the one-hot image the boxcar masks are an expansion of
            sc.remember(masks, 'M', dict(argmax=image), dict(S=2, K=K, T=T))
    return masks


def getTargetSpectrogramEstimates(targetCoefficientMasks, complexMixtureSpectrogram, W, stereoH, reconstruction='direct',
                                  spatialIterations=0):
    """gccNMF/gccNMFFunctions.py:145-151.  Returns (numTargets, 2, F, T) complex64.

    ``reconstruction='ratio'`` (not in the reference): the Wiener-like ratio mask X_c * W.(H_c o M_i) / den instead of W.(H_c o M_i) with
    the mixture phase.  Masks that came from getTargetCoefficientMasks take the one-hot form (den = the sum of the targets' numerators:
    the targets add up to the mixture); any other mask array takes the soft form (den = W.H_c).  At most 8 targets.

    ``reconstruction='spatial'``: either form of the ratio mask followed by the multichannel Wiener filter of csrc/spatial.hip (one 2 x 2
    spatial covariance per target and bin from the masked estimates, then v_i R_i (sum_j v_j R_j)^-1 applied to the stereo mixture);
    ``spatialIterations`` (0 to 255) EM iterations of the local Gaussian model refine v_i and R_i in between (csrc/spatial_em.hip)."""
    M = np.asarray(targetCoefficientMasks)
    X = np.asarray(complexMixtureSpectrogram)
    S, K, T = M.shape
    check_reconstruction(reconstruction, S)
    spatialIterations = _hip.check_spatial_iterations(spatialIterations, reconstruction)
    C, F, _ = X.shape
    if C != 2:
        raise ValueError('stereo spectrogram expected')
    _, dev = _hip.lib(), _device()
    g = Geometry(F, T, K, 1, S)
    with _staging.Scope(dev) as sc:
        recM = _staging.lookup(M, 'M', dev)
        if recM is not None and recM.meta == dict(S=S, K=K, T=T):
            dA, dM = recM.tensors['argmax'], None                       # the arg-max image the masks were expanded from
        else:
            dA, dM = None, sc.dev('masks', (S, g.Kp, g.Tp), corner=(K, T))
            dM[:, :K, :T].copy_(sc.upload(M, 'M', float32))
        recX = _staging.lookup(X, 'X', dev)
        if recX is not None and recX.meta == dict(F=F, T=T):
            dX, dV = recX.tensors['X'], recX.tensors['V']
        else:
            dX = sc.dev('X', (2, g.Fp, g.Tp, 2), corner=(F, T))
            torch.view_as_complex(dX)[:, :F, :T].copy_(sc.upload(X, 'X', complex64))
            dV = sc.dev('V', (g.Fp, g.Np), corner=(F, g.N))
            _hip.magnitude(dX, F, T, 1, dV)
        dW = _device_W(sc, W, g, dev)
        dH = sc.dev('H', (g.Kp, g.Np), corner=(K, g.N))
        dH[:K, :g.N].unflatten(1, (2, T)).copy_(sc.upload(np.asarray(stereoH), 'stereoH', float32).permute(1, 0, 2))   # (K, [L | R])
        ws = None
        if reconstruction != 'ratio':
            ws = sc.dev('ws_cov' if reconstruction == 'spatial' else 'ws_rec', (_hip.reconstruct_workspace_floats(reconstruction, T, K, S, 1, g.Fp, spatialIterations),))
        spec = sc.dev('spec', (2 * S, g.Fp, g.Tp, 2))
        _hip.reconstruct(dW, dH, dA, dM, dX, dV, F, T, K, S, 1, spec, mode=reconstruction, workspace=ws, iterations=spatialIterations)
        out = sc.download(torch.view_as_complex(spec)[:, :F, :T], shape=(S, 2, F, T))
        sc.remember(out, 'S', dict(spec=spec), dict(nsig=2 * S, F=F, T=T))
    return out


def getTargetSignalEstimates(targetSpectrogramEstimates, windowSize, hopSize, windowFunction):
    """gccNMF/gccNMFFunctions.py:153-163: istft (center=True) of every (target, channel) times
    2*hop/ws.  Returns ndarray (numTargets, numChannels, hop*(T-1)) float32."""
    S4 = np.asarray(targetSpectrogramEstimates)
    numTargets, numChannels, numFreq, numTime = S4.shape
    stftGainFactor = hopSize / float(windowSize) * 2
    rec = _staging.lookup(S4, 'S', _device())
    if rec is not None and rec.meta != dict(nsig=numTargets * numChannels, F=numFreq, T=numTime):
        rec = None
    y = _istft_device(S4.reshape(numTargets * numChannels, numFreq, numTime), hopSize, windowSize, windowFunction,
                      center=True, gain=stftGainFactor, device_spec=None if rec is None else rec.tensors['spec'])
    return y.reshape(numTargets, numChannels, -1)


def saveTargetSignalEstimates(targetSignalEstimates, sampleRate, mixtureFileNamePrefix):
    """gccNMF/gccNMFFunctions.py:165-169."""
    numTargets = targetSignalEstimates.shape[0]
    for targetIndex in range(numTargets):
        wavwrite(targetSignalEstimates[targetIndex], getSourceEstimateFileName(mixtureFileNamePrefix, targetIndex), sampleRate)


# ---- named by BASELINE.json's north_star; not in the reference -----------------
def getTargetTDOAEstimates(complexMixtureSpectrogram, sampleRate, microphoneSeparationInMetres, numTDOAs, numSources,
                           gccPHATNLEnabled=False, gccPHATNLAlpha=2.0):
    """Convenience wrapper over the reference's three-step TDOA estimation
    (runGCCNMF.py:44-47): coherence -> getAngularSpectrogram -> time mean ->
    estimateTargetTDOAIndexesFromAngularSpectrum.  Returns (targetTDOAIndexes, meanAngularSpectrum).
    ``gccPHATNLEnabled`` / ``gccPHATNLAlpha``: as for getAngularSpectrogram (the peaks of the GCC-NONLIN spectrum).
    ``numSources='auto'``: the file's own count (estimateNumSourcesFromAngularSpectrum), MAX_AUTO_SOURCES at the most."""
    nl, alpha = _hip.check_gcc_phat_nl(gccPHATNLEnabled, gccPHATNLAlpha)
    auto = _hip.check_auto_sources(numSources, MAX_AUTO_SOURCES)
    if auto:
        numSources = MAX_AUTO_SOURCES
    X = np.asarray(complexMixtureSpectrogram).astype(complex64)
    C, F, T = X.shape
    _, dev = _hip.lib(), _device()
    g = Geometry(F, T, 1, int(numTDOAs), int(numSources))
    frequenciesInHz = linspace(0, sampleRate / 2.0, F)
    trig = torch.from_numpy(steering_tables(frequenciesInHz, getTDOAsInSeconds(microphoneSeparationInMetres, numTDOAs),
                                            g.Fp, g.Dp)).to(dev)
    dX = padded(np.ascontiguousarray(X).view(float32).reshape(2, F, T, 2), (2, g.Fp, g.Tp, 2), dev)
    dC = torch.zeros((2, g.Fp, g.Tp), dtype=torch.float32, device=dev)
    ang = torch.zeros((g.Dp, g.Tp), dtype=torch.float32, device=dev)
    meanA = torch.zeros((g.Dp,), dtype=torch.float64, device=dev)
    idx = torch.zeros((g.S,), dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    _hip.coherence(dX, F, T, 1, dC)
    _hip.angular_spectrogram(dC, trig, F, T, g.D, 1, ang, meanA, nl_alpha=alpha if nl else None)
    if auto:
        _hip.count_tdoa_peaks(meanA, g.D, g.Dp, g.S, 1, idx, status)
        found = sorted(np.int64(i) for i in idx.cpu().numpy() if i >= 0)
        _report_auto_sources(len(found), int(status.cpu()[0]), g.S, 'getTargetTDOAEstimates')
        return found, meanA[:g.D].cpu().numpy()
    _hip.pick_tdoa_peaks(meanA, g.D, g.Dp, g.S, 1, idx, status)
    if int(status.cpu()[0]) != 0:
        raise ValueError("didn't find enough peaks in getTargetTDOAEstimates")
    return sorted(np.int64(i) for i in idx.cpu().numpy()), meanA[:g.D].cpu().numpy()
