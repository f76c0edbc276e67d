"""Device-resident GCC-NMF pipeline for a batch of equally shaped stereo mixtures.

Python here is plumbing only: PyTorch-ROCm owns the HBM allocations and the HIP
stream, every stage is one (or a few) calls into libgccnmf_hip.so through
``_hip`` (C ABI, include/gccnmf_hip.h).  Nothing in this module computes on the
host except the input-independent constant tables (window, FFT twiddles,
steering cos/sin, MT19937 initial W/H), which the reference also derives on the
host (gccNMF/gccNMFFunctions.py:53-59, :70-73, :87-89).

Stage order = gccNMF/runGCCNMF.py:36-52.
"""
import ctypes
import functools
import warnings

import numpy as np
import torch

from . import _hip
from ._hip import (_ptr, _stream, klnmf_divergence, check_gcc_phat_nl, check_tdoa_tracking, check_reconstruction,       # noqa: F401
                   GCCNMF_FLAG_FIXED_W, GCCNMF_FLAG_H_ONES, GCCNMF_RECONSTRUCT_RATIO, RECONSTRUCTIONS, RATIO_MAX_TARGETS)

SPEED_OF_SOUND_IN_METRES_PER_SECOND = 340.29          # gccNMF/gccNMFFunctions.py:38


def _on_device(method):
    """The C library launches on the CURRENT HIP device: make the object's device current for the duration of the call."""
    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        with torch.cuda.device(self.device):
            return method(self, *args, **kwargs)
    return wrapper


def num_frames(n_samples, n_fft, hop):
    """gccNMF/librosaSTFT.py:425."""
    return 1 + int((n_samples - n_fft) / hop)


def klnmf_initial_factors(F, N, K, epsilon=1e-16, seedValue=0):
    """gccNMF/gccNMFFunctions.py:70-73: legacy MT19937, W before H, float64 -> float32, + epsilon."""
    rs = np.random.RandomState(seedValue)
    W = rs.random_sample((F, K)).astype(np.float32) + epsilon
    H = rs.random_sample((K, N)).astype(np.float32) + epsilon
    return W.astype(np.float32), H.astype(np.float32)


def semi_supervised_initial_factors(dictionaryW, numFreeAtoms, N, epsilon=1e-16, seedValue=0):
    """Initial (W, H) of semi-supervised KL-NMF: the dictionary's columns followed by columns [K_fixed, K) of the W0 that
    klnmf_initial_factors(F, N, K, epsilon, seedValue) draws for K = K_fixed + numFreeAtoms; H is its H0.  float32 (F, K), (K, N)."""
    F, Kf = dictionaryW.shape
    W0, H0 = klnmf_initial_factors(F, N, Kf + int(numFreeAtoms), epsilon, seedValue)
    return np.ascontiguousarray(np.concatenate([np.asarray(dictionaryW, np.float32), W0[:, Kf:]], axis=1)), H0


class ChainHandOverError(RuntimeError):
    """A chained KL-NMF launch of a chunk did not hand over cleanly (gccnmf_klnmf_chain_status): the run is repeated on plain launches."""


def check_temporal_continuity(temporalContinuity, dictionaryW, numFreeAtoms, divergence, tolerance, klnmf_flags, nmf_groups, windowSize,
                              dictionarySize, batch):
    """The ``temporalContinuity`` keyword of the engines; no device needed.  Returns the weight as a float; ValueError for a weight that is
    no finite number >= 0 and, for a weight above 0, with anything the temporal-continuity call does not combine with or outside its
    envelope (at most 2049 bins, 1024 atoms, 65535 files)."""
    weight = _hip.check_continuity(temporalContinuity, 2)[0]
    if weight > 0:
        if dictionaryW is not None or numFreeAtoms:
            raise ValueError('temporalContinuity learns every atom: not available with dictionaryW or numFreeAtoms')
        if _hip.check_divergence(divergence) != 'kl':
            raise ValueError('temporalContinuity is a term of the KL iteration: not available with divergence=%r' % (divergence,))
        if tolerance is not None:
            raise ValueError('temporalContinuity has no stopping rule on the penalised objective: not available with tolerance')
        if klnmf_flags & 6:
            raise ValueError('temporalContinuity cannot be combined with the concurrent-groups or unfused-W-update bits of klnmf_flags')
        if nmf_groups not in (None, 1):
            raise ValueError('temporalContinuity runs as one file group (nmf_groups=1)')
        _hip._continuity_words(weight, 2, int(windowSize) // 2 + 1, 2, 128 if dictionarySize is None else int(dictionarySize), max(int(batch), 1), 0,
                               False)
    return weight


def converge_klnmf(launch, divergence, factors, maxIterations, tolerance, checkEvery, failed=None):
    """KL-NMF in chunks of ``checkEvery`` iterations until every file has converged or ``maxIterations`` is reached (plumbing: the
    iterations and the divergence are library calls).

    launch(n, first) runs n more iterations on the factors in place (repeated gccnmf_klnmf calls continue where the last one stopped);
    divergence() returns the (batch,) float64 host array of D(V || W.H) (one synchronisation per check); factors: the device tensors,
    batch first, that hold each file's result; failed(): the chain status after a chunk (non-zero raises ChainHandOverError).

    After a chunk, file b has converged when D_prev - D_cur < tolerance * D_prev or D_cur <= 0, D_prev of the first check being the
    divergence of the initial factors.  A RISE of D therefore stops a file too: intended for sparsityAlpha > 0, where the updates
    minimise D + alpha * sum(H) and D alone may go up.  A non-finite D stops nothing (it surfaces through the status checks).  A
    converged file's factors are copied aside at that check and put back at the end, while the batch goes on: its result and its
    iteration count depend on that file alone.  Chunked and single-call runs agree to round-off only (H is materialised, H *= atom
    norms, between chunks).  Returns (iterations (batch,) int64, trace (checks + 1, batch) float64; a converged file's column
    keeps the value it stopped at)."""
    D_prev = np.array(divergence(), dtype=np.float64)
    batch = D_prev.shape[0]
    trace = [D_prev.copy()]
    iterations = np.zeros(batch, np.int64)
    active = np.ones(batch, bool)
    snapshots, frozen, done = None, [], 0
    while done < maxIterations and active.any():
        n = min(checkEvery, maxIterations - done)
        launch(n, done == 0)
        done += n
        if failed is not None and failed():
            raise ChainHandOverError('a chained KL-NMF launch did not hand over cleanly')
        D = np.array(divergence(), dtype=np.float64)
        with np.errstate(invalid='ignore', over='ignore'):
            converged = active & ((D_prev - D < tolerance * D_prev) | (D <= 0))
        trace.append(np.where(active, D, trace[-1]))
        iterations[converged] = done
        active &= ~converged
        D_prev = np.where(active, D, D_prev)
        if converged.any() and active.any() and done < maxIterations:          # the batch goes on: keep what these files have now
            idx = torch.as_tensor(np.nonzero(converged)[0], device=factors[0].device)
            if snapshots is None:
                snapshots = [torch.empty_like(t) for t in factors]
            for snap, t in zip(snapshots, factors):
                snap.index_copy_(0, idx, t.index_select(0, idx))
            frozen.extend(np.nonzero(converged)[0].tolist())
    iterations[active] = done
    if frozen:
        idx = torch.as_tensor(frozen, device=factors[0].device)
        for snap, t in zip(snapshots, factors):
            t.index_copy_(0, idx, snap.index_select(0, idx))
    return iterations, np.stack(trace)


def check_iterations(trace, checkEvery, maxIterations):
    """The iteration count behind every row of a converge_klnmf trace: 0, checkEvery, 2 checkEvery, ... capped at maxIterations."""
    return [c * checkEvery if c * checkEvery < maxIterations else maxIterations for c in range(len(trace))]


def check_dictionary(W, F):
    """A pre-trained dictionary as the fixed-dictionary call takes it: finite, non-negative float32 (F, K) with 1 <= K <= 1024."""
    W = np.asarray(W)
    if W.ndim != 2 or W.shape[0] != F or not 1 <= W.shape[1] <= 1024:
        raise ValueError('dictionaryW must have shape (%d, K) with 1 <= K <= 1024, got %s' % (F, W.shape))
    W = W.astype(np.float32)
    if not np.isfinite(W).all() or (W < 0).any():
        raise ValueError('dictionaryW must be finite and non-negative')
    return W


def inferKLNMFCoefficients(V, W, numIterations, sparsityAlpha=0, epsilon=1e-16, seedValue=0, initialH='random', device='cuda:0',
                           tolerance=None, checkEvery=10):
    """H of KL-NMF against the fixed dictionary W -- performKLNMF's H update (gccNMF/gccNMFFunctions.py:76) with W never updated, on
    the device (gccnmf_klnmf with GCCNMF_FLAG_FIXED_W).  V: (F, N) or (batch, F, N); W: (F, K).  initialH: 'random' = the H0 that
    performKLNMF draws (klnmf_initial_factors(...)[1]), 'ones' = all ones.  Returns float32 H of shape (K, N) or (batch, K, N).

    ``tolerance`` (None = exactly ``numIterations`` iterations): stop each file once its KL divergence has stopped falling, checked
    every ``checkEvery`` iterations with ``numIterations`` as the maximum (converge_klnmf states the rule).  Returns (H, info) then,
    info = {'iterations': per file (an int for a single V), 'divergences': [(iteration, D), ...] from (0, D of the initial H)}."""
    V = np.asarray(V, dtype=np.float32)
    single = V.ndim == 2
    if single:
        V = V[None]
    if V.ndim != 3:
        raise ValueError('V must be (F, N) or (batch, F, N)')
    B, F, N = V.shape
    W = check_dictionary(W, F)
    K = W.shape[1]
    if initialH not in ('random', 'ones'):
        raise ValueError("initialH must be 'random' or 'ones'")
    tolerance, checkEvery, numIterations = _hip.check_convergence(tolerance, checkEvery, numIterations)
    lib = _hip.lib()
    dev = torch.device(device)
    g = Geometry(F, -(-N // 2), K)
    Np = -(-N // 64) * 64
    with torch.cuda.device(dev):
        Vd = torch.zeros((B, g.Fp, Np), dtype=torch.float32, device=dev)
        Vd[:, :F, :N] = torch.from_numpy(np.ascontiguousarray(V)).to(dev)
        Wd = padded(W, (g.Fp, g.Kp), dev)
        Hd = torch.zeros((B, g.Kp, Np), dtype=torch.float32, device=dev)
        if initialH != 'ones':
            Hd[:, :K, :N] = torch.from_numpy(klnmf_initial_factors(F, N, K, epsilon, seedValue)[1]).to(dev)
        ws = torch.zeros(lib.gccnmf_klnmf_workspace_floats(F, N, K, B), dtype=torch.float32, device=dev)

        def launch(n, first):            # (the all-ones start is a flag of the first call only: later chunks continue from H)
            _hip.klnmf(Vd, Wd, Hd, ws, F, N, K, B, n, float(sparsityAlpha), float(epsilon), fixed_w=True, h_ones=first and initialH == 'ones')
        if tolerance is None:
            launch(numIterations, True)
            H = Hd[:, :K, :N].cpu().numpy()
            return H[0] if single else H
        if initialH == 'ones':
            Hd[:, :K, :N] = 1            # the divergence of the initial factors reads H
        iterations, trace = converge_klnmf(launch, lambda: klnmf_divergence(Vd, Wd, Hd, ws, F, N, K, B, fixed=True).cpu().numpy(),
                                           [Hd], numIterations, tolerance, checkEvery)
        H = Hd[:, :K, :N].cpu().numpy()
    checks = check_iterations(trace, checkEvery, numIterations)
    if single:
        return H[0], dict(iterations=int(iterations[0]), divergences=[(it, float(d[0])) for it, d in zip(checks, trace)])
    return H, dict(iterations=iterations, divergences=[(it, d.copy()) for it, d in zip(checks, trace)])


def fft_twiddles(n_fft):
    k = np.arange(n_fft // 2, dtype=np.float64)
    tw = np.exp(-2j * np.pi * k / n_fft).astype(np.complex64)
    return np.ascontiguousarray(tw).view(np.float32)


def steering_tables(frequenciesInHz, tdoasInSeconds, Fp, Dp):
    """cos / sin of 2*pi*f*tau, evaluated in float64 like the reference's
    exp(outer(f, -2j*pi*tau)) (gccNMF/gccNMFFunctions.py:89,127), zero padded to [2][Fp][Dp]."""
    E = np.exp(np.outer(np.asarray(frequenciesInHz, np.float64), -(2j * np.pi) * np.asarray(tdoasInSeconds, np.float64)))
    F, D = E.shape
    trig = np.zeros((2, Fp, Dp), np.float32)
    trig[0, :F, :D] = E.real
    trig[1, :F, :D] = -E.imag
    return trig


class Geometry(object):
    """Padded storage geometry; the pitches come from the library so host and kernels cannot disagree."""

    def __init__(self, F, T, K, D=1, S=1):
        vals = [ctypes.c_int() for _ in range(4)]
        _hip.check(_hip.lib().gccnmf_pitches(F, T, K, *[ctypes.byref(v) for v in vals]), 'gccnmf_pitches')
        self.F, self.T, self.K, self.D, self.S = F, T, K, D, S
        self.N = 2 * T
        self.Fp, self.Kp, self.Np, self.Tp = [v.value for v in vals]
        self.Dp = -(-D // 64) * 64


def padded(host, shape, device, dtype=torch.float32):
    """Upload ``host`` (ndarray) into the top-left corner of a zero tensor of ``shape``."""
    t = torch.zeros(shape, dtype=dtype, device=device)
    src = torch.from_numpy(np.ascontiguousarray(host))
    idx = tuple(slice(0, n) for n in host.shape)
    t[idx] = src.to(device)
    return t


class GCCNMFEngine(object):
    """All buffers of one batch shape, allocated once; ``separate()`` runs the full path on device.

    ``GCCNMFEngine(lengths=[n_0, n_1, ...], ...)`` -- mixtures of DIFFERENT lengths -- returns a ``RaggedGCCNMFEngine``.

    ``dictionaryW``: a pre-trained (n_fft/2+1, K) dictionary (e.g. pretraining.loadPretrainedW): KL-NMF then infers only the coefficients
    against it (gccnmf_klnmf with GCCNMF_FLAG_FIXED_W, every iteration in one launch) and K is the dictionary's.  ``initialH``: 'random'
    (the H0 performKLNMF draws) or 'ones'.

    ``numFreeAtoms`` = n > 0 beside ``dictionaryW`` (semi-supervised KL-NMF): every file learns n free atoms of its
    own beside the dictionary, with the coefficients of all K = K_fixed + n atoms (gccnmf_klnmf with GCCNMF_FLAG_FREE_ATOMS(n)) -- what
    the dictionary was not trained on (an unseen noise, another room) goes to the free atoms instead of being forced onto speech atoms.
    The dictionary's columns stay bit for bit; the free atoms start as columns [K_fixed, K) of the W0 that
    klnmf_initial_factors(F, N, K, epsilon, seedValue) draws, H as its H0.  ``get_WH()`` returns each file's learned W.  K_fixed a
    multiple of 16, n <= 128, K <= 1024; not with initialH='ones' or lengths=.

    ``reconstruction``: 'direct' = the reference's target spectrograms, W.(H_c o M_i) with the mixture phase (gccNMFFunctions.py:145-151);
    'ratio' = the Wiener-like ratio mask X_c * W.(H_c o M_i) / sum_j W.(H_c o M_j), whose targets add up to the mixture (one fused launch,
    csrc/ratio.hip; at most 8 targets); 'spatial' = the ratio mask followed by a multichannel Wiener filter (csrc/spatial.hip; DESIGN
    section 4c): one 2 x 2 spatial covariance per target and bin from the masked estimates, then the stereo mixture vector filtered with
    v_i R_i (sum_j v_j R_j)^-1 per (bin, frame) -- the targets still add up to the mixture, and the inter-channel phase is used.
    ``spatialIterations`` (0 to 255, default 0; with 'spatial' only): that many EM iterations of the local Gaussian
    model refine v_i and R_i between the two steps, in one launch (csrc/spatial_em.hip); 0 is the filter alone, bit for bit.
    Everything up to the coefficient masks is the same in all modes.

    ``gccPHATNLEnabled`` / ``gccPHATNLAlpha`` (the reference's settings, gccNMF/realtime/config.py:42-43): localise on the GCC-NONLIN
    angular spectrum sum_f 1 - tanh(alpha sqrt(max(0, 1 - Re(C e^{-j 2 pi f tau})))) of Blandin, Ozerov & Vincent (2012) instead of
    GCC-PHAT (csrc/angular_nl.hip).  The BSS-Locate toolbox writes sqrt(2 - 2 re): that is this function with alpha * sqrt(2).  Only the
    TDOA indexes change; the GCC-NMF atom scores stay PHAT.

    ``tdoaTracking`` / ``localizationWindowSize`` (talkers who move): instead of one TDOA per target for the whole
    file, ``localize()`` also picks the ``numTargets`` peaks of every frame's windowed mean of the angular spectrogram (a centred window
    of ``localizationWindowSize`` frames, truncated at the ends of the file) and ``masks()`` scores every atom and frame against that
    frame's directions: ``get_tdoa_tracks()`` (batch, S, T), ``get_track_status()`` (batch, T; 1 = the frame had fewer peaks and took
    the previous frame's set).  Target i of a frame is its i-th peak from the left: talkers whose directions cross swap outputs.
    ``get_tdoa_indexes()`` stays the whole-file estimate.  A window of 2T - 1 frames or more gives the static path bit for bit.

    ``numTargets='auto'`` / ``maxTargets``: every file is split into as many targets as its own mean angular
    spectrum shows -- ``localize()`` counts them (the exact two-cluster split of the peak heights, the count mode of
    gccnmf_pick_tdoa_peaks) and ``masks()`` scores the atoms against each file's own directions.  All buffers and outputs have
    ``maxTargets`` (default 4, at most 8) slots per file; the slots at and beyond a file's count are all zero.  ``get_num_sources()``
    (batch,), ``get_tdoa_indexes()`` (batch, maxTargets) with -1 beyond the count, ``get_count_status()`` (batch,): 0, 1 = no peak
    (``check_status()`` raises), 2 = more than maxTargets found, the highest kept (not raised).  Not with tdoaTracking.

    ``tolerance`` / ``checkEvery``: with a tolerance, ``numIterations`` is the MAXIMUM -- ``klnmf()`` runs the
    library in chunks of ``checkEvery`` iterations and stops each file once its KL divergence D(V || W.H) has stopped falling
    (converge_klnmf states the rule; a rise stops a file too, which is intended for sparsityAlpha > 0).  ``get_iterations()`` (batch,),
    ``get_divergence_trace()`` (checks + 1, batch).  A file's factors and count depend on that file alone; they agree with a
    single call of the same count to round-off, not to the bit.  ``tolerance=None`` is the single call, bit for bit.
    ``get_divergence()`` (batch,) float64 works after ``klnmf()`` either way: one launch (gccnmf_klnmf_stage, stage 7).

    ``divergence`` = 'kl' (default) | 'is' | 'euclidean' (DESIGN section 2d): the objective the factorisation minimises -- Itakura-Saito
    or Euclidean NMF in place of KL (gccnmf_klnmf with GCCNMF_FLAG_DIVERGENCE_*: plain launches, one file group).  V stays the MAGNITUDE
    spectrogram and everything behind the factors is unchanged; ``tolerance`` / ``get_divergence()`` / ``get_divergence_trace()`` use the
    chosen divergence (getBetaDivergence states each).  Not with ``dictionaryW`` or ``numFreeAtoms``, nor with the concurrent-groups or
    unfused-W-update bits of ``klnmf_flags`` (ValueError); at most 1024 atoms and 2049 bins.
    ``temporalContinuity`` = weight >= 0 (default 0: the engine as it was, bit for bit): KL-NMF whose H update carries
    the temporal-continuity term inside the two column segments [L | R] of V (performTemporalKLNMF states it).  Everything behind the
    factors is unchanged and ``get_divergence()`` stays the KL divergence; one file group; not with ``dictionaryW``, ``numFreeAtoms``,
    another ``divergence``, ``tolerance`` or the concurrent-groups / unfused-W-update bits (ValueError before a device is looked for);
    at most 1024 atoms and 2049 bins."""

    def __new__(cls, n_samples=None, *args, **kwargs):
        if cls is GCCNMFEngine and kwargs.get('lengths') is not None:
            kwargs = dict(kwargs)
            if kwargs.pop('numFreeAtoms', 0):
                raise ValueError('numFreeAtoms is not available with lengths= (the ragged engine has no semi-supervised form)')
            return RaggedGCCNMFEngine(kwargs.pop('lengths'), *args, **kwargs)
        return super(GCCNMFEngine, cls).__new__(cls)

    def __init__(self, n_samples, sampleRate=16000, windowSize=1024, hopSize=256, numTDOAs=128,
                 microphoneSeparationInMetres=1.0, numTargets=3, dictionarySize=None, numIterations=100,
                 sparsityAlpha=0, epsilon=1e-16, seedValue=0, batch=1, windowFunction=np.hanning,
                 device='cuda:0', klnmf_flags=0, nmf_groups=None, dictionaryW=None, initialH='random', reconstruction='direct',
                 gccPHATNLEnabled=False, gccPHATNLAlpha=2.0, tdoaTracking=False, localizationWindowSize=None, tolerance=None, checkEvery=10,
                 numFreeAtoms=0, maxTargets=None, spatialIterations=0, divergence='kl', temporalContinuity=0.0):
        self.autoTargets, numTargets = _hip.check_auto_targets(numTargets, maxTargets, tdoaTracking)
        self.temporalContinuity = check_temporal_continuity(temporalContinuity, dictionaryW, numFreeAtoms, divergence, tolerance, klnmf_flags,
                                                            nmf_groups, windowSize, dictionarySize, batch)
        if self.temporalContinuity > 0:
            nmf_groups = 1
        self.divergence = _hip.check_divergence(divergence, int(windowSize) // 2 + 1, None if dictionarySize is None else int(dictionarySize))
        if self.divergence != 'kl':
            if dictionaryW is not None or numFreeAtoms:
                raise ValueError('divergence=%r learns every atom: not available with dictionaryW or numFreeAtoms' % (self.divergence,))
            if klnmf_flags & 6:
                raise ValueError('divergence=%r cannot be combined with the concurrent-groups or unfused-W-update bits of klnmf_flags'
                                 % (self.divergence,))
            if nmf_groups not in (None, 1):
                raise ValueError('divergence=%r runs as one file group (nmf_groups=1)' % (self.divergence,))
            nmf_groups = 1
        if initialH not in ('random', 'ones'):
            raise ValueError("initialH must be 'random' or 'ones'")
        self.initialH = initialH
        if numFreeAtoms and dictionaryW is None:
            raise ValueError('numFreeAtoms needs dictionaryW (without a dictionary every atom is free: dictionarySize)')
        if numFreeAtoms and initialH == 'ones':
            raise ValueError("numFreeAtoms cannot be combined with initialH='ones'")
        self.tolerance, self.checkEvery, numIterations = _hip.check_convergence(tolerance, checkEvery, numIterations)
        self.iterations_used = self.divergence_trace = None
        self.tdoaTracking, self.localizationWindowSize = check_tdoa_tracking(tdoaTracking, localizationWindowSize, numTargets)
        self.reconstruction = check_reconstruction(reconstruction, numTargets)
        self.spatialIterations = _hip.check_spatial_iterations(spatialIterations, self.reconstruction)
        if self.reconstruction == 'spatial':
            _hip.reconstruct_spatial_batch(batch)          # at most 65535 files per call: ValueError here, not at the first reconstruct()
        self.gccPHATNLEnabled, self.gccPHATNLAlpha = check_gcc_phat_nl(gccPHATNLEnabled, gccPHATNLAlpha)
        self.dictionaryW, self.numFreeAtoms = None, 0
        if dictionaryW is not None:
            self.dictionaryW = check_dictionary(dictionaryW, int(windowSize) // 2 + 1)
            self.numFreeAtoms = _hip.check_free_atoms(numFreeAtoms, self.dictionaryW.shape[1], int(windowSize) // 2 + 1)
            K = self.dictionaryW.shape[1] + self.numFreeAtoms
            if dictionarySize is not None and int(dictionarySize) != K:
                raise ValueError('dictionarySize %d conflicts with the %d atoms of dictionaryW%s' % (
                    dictionarySize, K, ' and the free atoms' if self.numFreeAtoms else ''))
            dictionarySize, nmf_groups = K, 1
        elif dictionarySize is None:
            dictionarySize = 128
        if not torch.cuda.is_available():
            raise _hip.HipLibraryError('no ROCm device visible: the GCC-NMF HIP path has no CPU fallback')
        self.lib = _hip.lib()
        self.device = torch.device(device)
        self.n_samples, self.sampleRate = int(n_samples), sampleRate
        self.n_fft, self.hop = int(windowSize), int(hopSize)
        self.iters, self.alpha, self.eps, self.seed = int(numIterations), float(sparsityAlpha), float(epsilon), seedValue
        self.batch = int(batch)
        self.d = microphoneSeparationInMetres
        self.klnmf_flags = klnmf_flags
        # KL-NMF runs per file group, each group on its own stream (the mixtures are independent): the end of one group's
        # launch -- when its last workgroups no longer fill both slots of every CU -- overlaps the start of another
        # group's.  A group must still fill the chip with throughput tiles by itself: >= 16 files.  Bitwise the same result.
        # Measured (64 files, K = 1024): 1 group 287.0 ms per step, 2 groups 278-280 ms; 4 groups 308 ms with the default 4
        # hardware queues (two groups end up sharing one and serialise) and 277 ms with GPU_MAX_HW_QUEUES=8 -- so 2.
        if nmf_groups is None:
            # two groups only when each half alone still makes the library's launch-size decisions exactly as the whole
            # batch would (>= 256 throughput tiles per GEMM launch, >= 256 atom tiles for the fused W update): the same
            # kernels run either way and the outputs are bit-identical
            half = self.batch // 2
            tiles_wh = -(-(2 * num_frames(self.n_samples, self.n_fft, self.hop)) // 64)
            atoms = -(-int(dictionarySize) // 64)
            nmf_groups = 2 if (self.batch % 2 == 0 and half >= 16 and half * tiles_wh >= 256 and half * atoms >= 256) else 1
            # Round 6: where the library runs the whole KL-NMF call as ONE chained launch (gccnmf_klnmf_plan bit 3: tiles handed over
            # between the GEMMs through ready counters, no launch boundaries left to overlap), one group is as fast as two plain ones at
            # 64 files and faster everywhere else (40 files: 134 k -> 156 k frames/s) -- and a second chained launch beside it only costs.
            Fq, Nq = int(windowSize) // 2 + 1, 2 * num_frames(self.n_samples, self.n_fft, self.hop)
            if nmf_groups > 1 and Nq > 0 and self.lib.gccnmf_klnmf_plan(Fq, Nq, int(dictionarySize), self.batch, klnmf_flags) & 8:
                nmf_groups = 1
        if nmf_groups < 1 or self.batch % nmf_groups:
            raise ValueError('nmf_groups must divide the batch')
        self.nmf_groups = int(nmf_groups)
        F = self.n_fft // 2 + 1
        T = num_frames(self.n_samples, self.n_fft, self.hop)
        if T < 2:
            raise ValueError('Buffer is too short (n=%d) for frame_length=%d' % (n_samples, self.n_fft))
        self.g = g = Geometry(F, T, int(dictionarySize), int(numTDOAs), int(numTargets))
        self.L = self.hop * (T - 1)
        dev, B = self.device, self.batch
        f32 = torch.float32

        with torch.cuda.device(dev):
            # constant tables
            self.window = torch.from_numpy(np.asarray(windowFunction(self.n_fft), np.float64).astype(np.float32)).to(dev)
            self.twiddle = torch.from_numpy(fft_twiddles(self.n_fft)).to(dev)
            maxTDOA = self.d / SPEED_OF_SOUND_IN_METRES_PER_SECOND
            self.tdoasInSeconds = np.linspace(-maxTDOA, maxTDOA, g.D)
            self.frequenciesInHz = np.linspace(0, sampleRate / 2.0, F)
            self.trig = torch.from_numpy(steering_tables(self.frequenciesInHz, self.tdoasInSeconds, g.Fp, g.Dp)).to(dev)
            W0, H0 = klnmf_initial_factors(F, g.N, g.K, self.eps, seedValue)
            self.W0 = padded(W0, (g.Fp, g.Kp), dev)
            self.H0 = padded(H0, (g.Kp, g.Np), dev)

            z = lambda *shape: torch.zeros(shape, dtype=f32, device=dev)
            self.x = z(B, 2, self.n_samples)
            self.X = z(B, 2, g.Fp, g.Tp, 2)
            self.V = z(B, g.Fp, g.Np)
            self.CC = z(B, 2, g.Fp, g.Tp)
            self.W = z(B, g.Fp, g.Kp)
            self.H = z(B, g.Kp, g.Np)
            if self.numFreeAtoms:
                # semi-supervised: every file starts from the dictionary followed by the drawn free atoms (refilled by _klnmf_start)
                self.W0 = padded(semi_supervised_initial_factors(self.dictionaryW, self.numFreeAtoms, g.N, self.eps, seedValue)[0], (g.Fp, g.Kp), dev)
            elif self.dictionaryW is not None:
                # the dictionary never changes: the per-file W that the masks and the reconstruction read is filled once, here
                self.W0 = padded(self.dictionaryW, (g.Fp, g.Kp), dev)
                self.W.copy_(self.W0.unsqueeze(0).expand_as(self.W))
            # nmf_groups equal group workspaces (for one group == the whole-batch workspace)
            self.ws_nmf = z(_hip.klnmf_continuity_workspace_floats(F, g.N, g.K, B) if self.temporalContinuity > 0 else
                            self.nmf_groups * _hip.klnmf_divergence_workspace_floats(F, g.N, g.K, B // self.nmf_groups, self.divergence))
            self.nmf_streams = [torch.cuda.Stream(device=dev) for _ in range(self.nmf_groups)] if self.nmf_groups > 1 else []
            # Copy streams of separate_batches, created ONCE and right behind the group streams.  The runtime maps streams onto a
            # few hardware queues in creation order (4 by default), and a queue is in-order: a 244 MB download that shares its queue
            # with a KL-NMF group holds that group's next kernels back for its 5 ms.  Fresh streams per call walked through torch's
            # pool and landed on the groups' queues every other call (measured: 264 ms per batch instead of 258).
            self.copy_streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
            self.ang = z(B, g.Dp, g.Tp)
            self.mean_ang = torch.zeros((B, g.Dp), dtype=torch.float64, device=dev)
            self.tdoa_idx = torch.zeros((B, g.S), dtype=torch.int32, device=dev)
            self.status = torch.zeros((B,), dtype=torch.int32, device=dev)
            if self.tdoaTracking:
                if T > _hip.TRACKS_MAX_FRAMES:
                    raise ValueError('tdoaTracking takes files of fewer than 2^21 frames, got %d' % T)
                self.tracks = torch.zeros((B, g.S, g.Tp), dtype=torch.int32, device=dev)
                self.track_status = torch.zeros((B, g.Tp), dtype=torch.int32, device=dev)
            self.ws_scores = z(self.lib.gccnmf_scores_workspace_floats(F, T, g.S, B))
            self.scores = z(B, g.Kp, g.S * g.Tp)
            self.argmax = torch.zeros((B, g.Kp, g.Tp), dtype=torch.uint8, device=dev)
            self.ws_rec = z(self._reconstruct_workspace_floats()) if self.reconstruction == 'direct' else None
            # the spatial mode's covariances [B][S][Fp][4], with spatialIterations followed by the powers [B][S][Fp][Tp]; an engine switched
            # to 'spatial' or given more iterations later allocates them at its next reconstruct()
            self.ws_cov = z(self._reconstruct_workspace_floats()) if self.reconstruction == 'spatial' else None
            self.spec = z(B, 2 * g.S, g.Fp, g.Tp, 2)
            # windowed time frames [B][2S][T][n_fft]: only the two-kernel iSTFT needs them (allocated on first use); the default is the
            # fused inverse-transform + overlap-add pass, available while n_fft + 3 * hop <= 2048 and hop <= n_fft (frames further apart
            # than their length leave samples no frame touches, which the fused pass would not write)
            self.frames = None
            # (a fused workgroup transforms 35 frames in sequence: with fewer than ~256 of them the two-kernel form is the faster one --
            # one file: 181 us fused against 42 us)
            self.fused_istft = self.n_fft + 3 * self.hop <= 2048 and self.hop <= self.n_fft and B * g.S * -(-T // 32) >= 256
            self.y = z(B, g.S, 2, self.L)
            self.pcm_in = None        # set by upload_pcm16(): the STFT then reads int16 frames directly
            self.pcm_out = None

    # ---- stages (each asynchronous on the current torch stream) ---------------------------------
    @_on_device
    def stft(self):
        pcm = self.pcm_in is not None     # int16 interleaved frames straight from the wav data chunk
        _hip.stft_stereo(self.pcm_in if pcm else self.x, self.n_samples, self.n_fft, self.hop, self.g.T, self.batch, self.window, self.twiddle,
                         self.X, self.V, self.CC, pcm16=pcm)

    @_on_device
    def pack_pcm16(self):
        """y -> int16 interleaved [batch][S][L][2] with wavwrite's clip protection per target (wavfile.py:39-48)."""
        g = self.g
        if self.pcm_out is None:
            self.pcm_out = torch.zeros((self.batch, g.S, self.L, 2), dtype=torch.int16, device=self.device)
            self.pcm_peak = torch.zeros((self.batch * g.S,), dtype=torch.int32, device=self.device)
        _hip.pack_pcm16(self.y, self.batch * g.S, self.L, self.pcm_peak, self.pcm_out)

    @_on_device
    def klnmf(self):
        """KL-NMF of the batch from the initial factors: ``numIterations`` iterations in one call, or -- with a tolerance -- in chunks
        of ``checkEvery`` until every file has converged (at most ``numIterations``)."""
        if self.tolerance is None:
            self._klnmf_start()
            self._klnmf_iterate(self.iters, True)
            return
        for attempt in range(2):
            self._klnmf_start()
            if self._fixed() and self.initialH == 'ones':
                self.H[:, :self.g.K, :self.g.N] = 1                 # the divergence of the initial factors reads H
            try:
                self.iterations_used, self.divergence_trace = converge_klnmf(
                    self._klnmf_iterate, lambda: self._divergence().cpu().numpy(), [self.H] if self._fixed() else [self.W, self.H],
                    self.iters, self.tolerance, self.checkEvery, failed=self.chain_failed)
                return
            except ChainHandOverError:
                if attempt:
                    raise
                self._fall_back_to_plain_launches()

    def _fall_back_to_plain_launches(self):
        warnings.warn('gcc_nmf_amd: a chained KL-NMF launch did not hand over cleanly; this process falls back to the plain launches '
                      '(gccnmf_set_tuning(21, 0)) and repeats the batch', RuntimeWarning)
        _hip.check(self.lib.gccnmf_set_tuning(21, 0), 'gccnmf_set_tuning')

    def _fixed(self):
        """A dictionary and no free atoms: the fixed-dictionary call (one shared W, never written)."""
        return self.dictionaryW is not None and not self.numFreeAtoms

    def _klnmf_start(self):
        """The initial factors into W and H (a fixed dictionary with the all-ones start needs none: H is then output only)."""
        if self._fixed():
            if self.initialH != 'ones':
                self.H.copy_(self.H0.unsqueeze(0).expand_as(self.H))
            return
        self.W.copy_(self.W0.unsqueeze(0).expand_as(self.W))
        self.H.copy_(self.H0.unsqueeze(0).expand_as(self.H))

    def _groups(self):
        """(first file, files, workspace, stream or None) of every KL-NMF file group: equal shares of the batch and of ws_nmf (a group's
        status words sit at the end of its own share); a single group is the whole batch on the current stream."""
        per, ws_per = self.batch // self.nmf_groups, self.ws_nmf.numel() // self.nmf_groups
        for i in range(self.nmf_groups):
            yield i * per, per, self.ws_nmf[i * ws_per:], self.nmf_streams[i] if self.nmf_streams else None

    def _divergence(self):
        """(batch,) float64 on the device: stage 7 per file group, each in its own workspace."""
        g = self.g
        fixed = self._fixed()
        out = [klnmf_divergence(self.V[b0], self.W0 if fixed else self.W[b0], self.H[b0], ws, g.F, g.N, g.K, per, fixed, divergence=self.divergence)
               for b0, per, ws, _ in self._groups()]
        return out[0] if len(out) == 1 else torch.cat(out)

    @_on_device
    def get_divergence(self):
        """(batch,) float64: D(V || W.H) of the factors as they are now (after klnmf()), in the engine's ``divergence``; one launch and a
        download."""
        return self._divergence().cpu().numpy()

    def get_iterations(self):
        """(batch,) int64: the iterations each file ran (the check at which it converged, else numIterations).  Needs a tolerance."""
        if self.tolerance is None or self.iterations_used is None:
            raise ValueError('get_iterations needs tolerance= and a klnmf() run')
        return self.iterations_used.copy()

    def get_divergence_trace(self):
        """(checks + 1, batch) float64: each file's divergence at iteration 0 and at every check; a converged file's column keeps the
        value it stopped at.  Needs a tolerance."""
        if self.tolerance is None or self.divergence_trace is None:
            raise ValueError('get_divergence_trace needs tolerance= and a klnmf() run')
        return self.divergence_trace.copy()

    def _klnmf_iterate(self, iters, first):
        """``iters`` more iterations on W and H in place, as the library chooses to launch them (first: the first call of a run)."""
        g = self.g
        fixed = self._fixed()        # (one group then; with the all-ones start H is output only: no H0 broadcast)
        if self.nmf_groups > 1:
            main = torch.cuda.current_stream(self.device)
            ready = torch.cuda.Event()
            ready.record(main)
        for b0, per, ws, st in self._groups():
            if st is not None:
                st.wait_event(ready)
            # groups: the groups' launches share the chip, so launch forms are chosen for all groups together (a file's bits do not
            # depend on the split) and each keeps the throughput tile -- its partial last round overlaps the other group's kernels
            # (all-half-height tiles, which win for a 32-file launch ALONE, lose here: 152.4 k vs 155.4 k frames/s)
            _hip.klnmf(self.V[b0], self.W0 if fixed else self.W[b0], self.H[b0], ws, g.F, g.N, g.K, per, iters, self.alpha, self.eps,
                       fixed_w=fixed, h_ones=fixed and first and self.initialH == 'ones', groups=self.nmf_groups,
                       flags=0 if fixed else self.klnmf_flags, free_atoms=self.numFreeAtoms, stream=None if st is None else st.cuda_stream,
                       divergence=self.divergence, continuity=self.temporalContinuity, segments=2)
            if st is not None:
                done = torch.cuda.Event()
                done.record(st)
                main.wait_event(done)

    @_on_device
    def localize(self):
        g = self.g
        _hip.angular_spectrogram(self.CC, self.trig, g.F, g.T, g.D, self.batch, self.ang, self.mean_ang,
                                 nl_alpha=self.gccPHATNLAlpha if self.gccPHATNLEnabled else None)
        if self.autoTargets:
            _hip.count_tdoa_peaks(self.mean_ang, g.D, g.Dp, g.S, self.batch, self.tdoa_idx, self.status)
            return
        _hip.pick_tdoa_peaks(self.mean_ang, g.D, g.Dp, g.S, self.batch, self.tdoa_idx, self.status)
        if self.tdoaTracking:
            _hip.pick_tdoa_tracks(self.ang, g.D, g.T, g.S, self.localizationWindowSize, self.batch, self.tracks, self.track_status)

    @_on_device
    def masks(self):
        g = self.g
        if self.autoTargets:
            _hip.target_scores_masks_counted(self.CC, self.trig, self.tdoa_idx, self.W, g.F, g.T, g.K, g.D, g.S, self.batch, self.ws_scores,
                                             self.scores, self.argmax, counted=True)
            return
        _hip.target_scores_masks(self.CC, self.trig, self.tracks if self.tdoaTracking else self.tdoa_idx, self.W, g.F, g.T, g.K, g.D, g.S,
                                 self.batch, self.ws_scores, self.scores, self.argmax, tracks=self.tdoaTracking)

    def _reconstruct_workspace_floats(self):
        g = self.g
        return _hip.reconstruct_workspace_floats(self.reconstruction, g.T, g.K, g.S, self.batch, g.Fp, self.spatialIterations)

    def _reconstruct_workspace(self):
        """The workspace of the current mode; the spatial one is (re)allocated here when the mode or spatialIterations grew past it."""
        if self.reconstruction != 'spatial':
            _hip.check_spatial_iterations(self.spatialIterations, self.reconstruction)
            return self.ws_rec
        need = self._reconstruct_workspace_floats()
        if self.ws_cov is None or self.ws_cov.numel() < need:
            self.ws_cov = torch.zeros(need, dtype=torch.float32, device=self.device)
        return self.ws_cov

    @_on_device
    def reconstruct(self):
        g = self.g
        _hip.reconstruct(self.W, self.H, self.argmax, None, self.X, self.V, g.F, g.T, g.K, g.S, self.batch, self.spec, mode=self.reconstruction,
                         workspace=self._reconstruct_workspace(), iterations=self.spatialIterations)

    @_on_device
    def istft(self, keep_frames=False):
        """spec -> y.  keep_frames: the two-kernel form that also leaves the windowed time frames in ``self.frames``."""
        g = self.g
        gain = np.float32(self.hop / float(self.n_fft) * 2)           # gccNMFFunctions.py:155
        frames = None
        if keep_frames or not self.fused_istft:
            if self.frames is None:
                self.frames = torch.zeros((self.batch, 2 * g.S, g.T, self.n_fft), dtype=torch.float32, device=self.device)
            frames = self.frames
        _hip.istft_ola(self.spec, 2 * g.S, self.n_fft, self.hop, g.T, self.batch, self.window, self.twiddle, gain, True, frames, self.y)

    @_on_device
    def run(self, stft=True):
        """samples already in ``self.x`` -> separated waveforms in ``self.y`` (all on device, asynchronous)."""
        if stft:
            self.stft()
        self.klnmf()
        self.localize()
        self.masks()
        self.reconstruct()
        self.istft()
        self._scored_y = self.y           # what score() reads: the buffer this run wrote (separate_batches alternates two)

    # ---- host <-> device -------------------------------------------------------------------------
    def _checked_samples(self, stereoSamples, one_file=True):
        """Host samples as float32 (batch, 2, n), ValueError otherwise; one_file: a single (2, n) mixture is a batch of one."""
        x = np.asarray(stereoSamples, dtype=np.float32)
        if one_file and x.ndim == 2:
            x = x[None]
        if x.shape != tuple(self.x.shape):
            raise ValueError('expected samples of shape %s, got %s' % (tuple(self.x.shape), x.shape))
        if not np.isfinite(x).all():
            raise ValueError('Audio buffer is not finite everywhere')      # librosaSTFT.py:488-489
        return x

    @_on_device
    def upload(self, stereoSamples):
        x = self._checked_samples(stereoSamples)
        self.pcm_in = None
        self.x.copy_(torch.from_numpy(np.ascontiguousarray(x)))

    @_on_device
    def upload_pcm16(self, pcm):
        """(batch, n, 2) int16 interleaved stereo frames, exactly as scipy.io.wavfile.read returns them (no host conversion)."""
        pcm = np.asarray(pcm)
        if pcm.ndim == 2:
            pcm = pcm[None]
        if pcm.dtype != np.int16 or pcm.shape != (self.batch, self.n_samples, 2):
            raise ValueError('expected int16 frames of shape %s, got %s %s' % ((self.batch, self.n_samples, 2), pcm.dtype, pcm.shape))
        if self.pcm_in is None:
            self.pcm_in = torch.zeros((self.batch, self.n_samples, 2), dtype=torch.int16, device=self.device)
        self.pcm_in.copy_(torch.from_numpy(np.ascontiguousarray(pcm)))

    @_on_device
    def separate_pcm16(self, pcm):
        """int16 frames in -> int16 frames out: (batch, n, 2) -> (batch, S, hop*(T-1), 2), i.e. loadMixtureSignal ...
        saveTargetSignalEstimates (runGCCNMF.py:35-54) minus the file system, with both wav conversions on the device."""
        self.upload_pcm16(pcm)
        self.run()
        self.pack_pcm16()
        out = self.pcm_out.cpu().numpy()
        self.check_status()
        self.check_pcm_finite()
        return out

    @_on_device
    def separate(self, stereoSamples):
        """(batch, 2, n) float32 host samples -> (batch, S, 2, hop*(T-1)) float32 host waveforms."""
        x = self._checked_samples(stereoSamples)
        # one page-locked staging pair (allocated on first use: 82 MB + 244 MB of host memory for a 64-file batch, nothing extra on the
        # device): both copies move at PCIe speed instead of through pageable bounce buffers (313 -> 285 ms host to host for one
        # batch).  The double-buffered pipeline -- a second x / y pair in HBM, two more pinned pairs -- belongs to separate_batches.
        if getattr(self, '_pin', None) is None:
            self._pin = (torch.zeros(self.x.shape, dtype=torch.float32).pin_memory(), torch.zeros(self.y.shape, dtype=torch.float32).pin_memory())
        hx, hy = self._pin
        hx.copy_(torch.from_numpy(np.ascontiguousarray(x)))
        self.pcm_in = None
        self.x.copy_(hx, non_blocking=True)
        self.run()
        if self.chain_failed():
            # The chained KL-NMF launch did not hand over cleanly (a consumer timed out / a work list ran on more than one XCC): its factors are
            # NaN by construction.  Do not fail the batch: switch this process to the plain launches and run the stages behind the STFT again.
            self._fall_back_to_plain_launches()
            self.run(stft=False)
        hy.copy_(self.y, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        self.check_status()
        return hy.numpy().copy()

    def separate_batches(self, batches):
        """Generator over an iterable of (batch, 2, n) float32 host arrays -> one (batch, S, 2, hop*(T-1)) float32 array per
        input, in order.  Same results as ``separate`` per batch, but the PCIe transfers (pinned staging buffers, their own
        streams) of batch i+1 (up) and i-1 (down) run under the compute of batch i: sustained host-to-host throughput
        approaches the device rate instead of paying both copies per batch."""
        dev = self.device
        g = self.g
        with torch.cuda.device(dev):
            compute = torch.cuda.current_stream(dev)
            s_in, s_out = self.copy_streams
            if getattr(self, '_pipe', None) is None:       # second device buffers + pinned staging: allocated once (page-locking is slow)
                self._pipe = dict(x=torch.zeros_like(self.x), y=torch.zeros_like(self.y),
                                  hx=[torch.zeros(self.x.shape, dtype=torch.float32).pin_memory() for _ in range(2)],
                                  hy=[torch.zeros(self.y.shape, dtype=torch.float32).pin_memory() for _ in range(2)],
                                  hs=[torch.zeros(self.status.shape, dtype=self.status.dtype).pin_memory() for _ in range(2)],
                                  ds=[torch.zeros_like(self.status) for _ in range(2)])
            xs, ys = [self.x, self._pipe['x']], [self.y, self._pipe['y']]
            hx, hy, status = self._pipe['hx'], self._pipe['hy'], self._pipe['hs']
            ev_in = [torch.cuda.Event() for _ in range(2)]
            ev_done = [torch.cuda.Event() for _ in range(2)]
            ev_out = [torch.cuda.Event() for _ in range(2)]
            ev_stft = torch.cuda.Event()
            pending = []                       # slots whose results have not been yielded yet, oldest first
            download = None                    # the deferred download of the batch enqueued last

            def collect(slot):
                ev_out[slot].synchronize()
                st = status[slot].numpy()
                if st.any():
                    raise ValueError(self._too_few_peaks(st))
                return hy[slot].numpy().copy()

            try:
                for i, batch in enumerate(batches):
                    slot = i & 1
                    if len(pending) == 2:                                # this slot's previous occupant must be handed out first
                        yield collect(pending.pop(0))
                    x = self._checked_samples(batch, one_file=False)
                    hx[slot].copy_(torch.from_numpy(np.ascontiguousarray(x)))    # host memcpy into the pinned buffer
                    with torch.cuda.stream(s_in):
                        s_in.wait_event(ev_done[slot])                   # batch i-2 no longer reads this x buffer
                        xs[slot].copy_(hx[slot], non_blocking=True)
                        ev_in[slot].record(s_in)
                    compute.wait_event(ev_in[slot])
                    compute.wait_event(ev_out[slot])                     # batch i-2's waveforms have left this y buffer
                    self.x, self.y, self.pcm_in = xs[slot], ys[slot], None
                    self.stft()
                    if download is not None:                             # batch i-1 goes down now that this batch's STFT is past
                        ev_stft.record(compute)
                        download(ev_stft)
                    self.run(stft=False)
                    self._pipe['ds'][slot].copy_(self.file_status())     # per-slot snapshot ON the compute stream: batch i+1's
                    ev_done[slot].record(compute)                        # localize() rewrites self.status before s_out has copied it

                    # The download is a shader copy on this runtime (rocprofv3: __amd_rocclr_copyBuffer, 4.6 ms for 244 MB at PCIe
                    # speed); next to the HBM-bound STFT of the following batch it held that kernel up from 0.6 to 4.9 ms.  So it is
                    # enqueued behind that STFT (or at once for the last batch) and runs in the shadow of the MFMA-bound KL-NMF.
                    def download(after=None, slot=slot):
                        with torch.cuda.stream(s_out):
                            s_out.wait_event(ev_done[slot])
                            if after is not None:
                                s_out.wait_event(after)
                            hy[slot].copy_(ys[slot], non_blocking=True)
                            status[slot].copy_(self._pipe['ds'][slot], non_blocking=True)
                            ev_out[slot].record(s_out)
                    pending.append(slot)
                if download is not None:
                    download()
                while pending:
                    yield collect(pending.pop(0))
            finally:
                torch.cuda.synchronize(dev)
                self.x, self.y = xs[0], ys[0]

    @_on_device
    def score(self, images, filterLength=512, guardSamples=0):
        """BSS Eval image criteria (evaluation.bss_eval_images) of the waveforms of the last ``separate()`` (or ``run()``; after
        ``separate_batches``, of the last batch it ran), scored where they lie on the device -- no download.  ``images``: the true source images (batch, S, 2, n_samples), host array or tensor,
        on the mixture's time axis: waveform sample y[n] belongs to images[..., n + windowSize // 2].  ``guardSamples`` are cut at both
        ends of the waveforms first.  Returns (sdr, isr, sir, sar, perm), each (batch, S) indexed by true source: output perm[b][j] is
        true source j, the assignment with the largest mean SIR.  On the enhancement engine S = 2: talker, noise.
        ValueError: numTargets='auto' (an empty slot has no image), no separation yet, a wrong shape, guardSamples not a whole number >= 0 or cutting
        everything, the rules of bss_eval_images, non-finite images or waveforms."""
        from . import evaluation
        if self.autoTargets:
            raise ValueError("score() is not available with numTargets='auto': empty target slots have no image")
        y = getattr(self, '_scored_y', None)
        if y is None:
            raise ValueError('score() needs a separation first: nothing has been separated by this engine yet')
        g = guardSamples
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or g < 0 or 2 * g >= self.L:
            raise ValueError('guardSamples must be a whole number >= 0 that leaves samples to score (%d per waveform), got %r' % (self.L, g))
        want = (self.batch, self.g.S, 2, self.n_samples)
        if tuple(images.shape) != want:
            raise ValueError('expected images of shape %s, got %s' % (want, tuple(images.shape)))
        off, g = self.n_fft // 2 + int(g), int(g)
        n = self.L - 2 * g
        evaluation.check_image_shape((self.batch, self.g.S, 2, n), filterLength)
        if torch.is_tensor(images):
            S = images[..., off:off + n].to(device=self.device, dtype=torch.float32).contiguous()
        else:
            S = torch.from_numpy(np.ascontiguousarray(np.asarray(images)[..., off:off + n], dtype=np.float32)).to(self.device)
        E = y[..., g:g + n].contiguous()
        if not (bool(torch.isfinite(S).all()) and bool(torch.isfinite(E).all())):
            raise ValueError('images or separated waveforms are not finite everywhere')
        from . import _eval
        _eval.require_device()
        return evaluation.score_device(S, E, filterLength)

    @_on_device
    def check_pcm_finite(self):
        """After pack_pcm16(): a NaN / Inf sample in a waveform shows up in that group's peak image (csrc/fft.hip)."""
        bad = (self.pcm_peak.cpu().numpy().view(np.uint32) >= 0x7F800000).reshape(self.batch, self.g.S)
        if bad.any():
            raise ValueError('non-finite samples in the separated waveforms of file(s) %s' % np.nonzero(bad.any(axis=1))[0].tolist())

    def file_status(self):
        """int32 [batch] on the device, non-zero = the file cannot be separated: too few peaks in its mean angular spectrum -- with
        tdoaTracking, in every frame's windowed mean (bit 1 of any frame's track status; the whole-file estimate is then only reported);
        with numTargets='auto', no peak at all (count status 1; a capped count, status 2, is no failure)."""
        if self.autoTargets:
            return (self.status == 1).to(torch.int32)
        return (self.track_status[:, 0] & 2) if self.tdoaTracking else self.status

    def _too_few_peaks(self, st):
        files = np.nonzero(st)[0].tolist()
        if self.autoTargets:
            return 'no angular-spectrum peak to count in file(s) %s' % files
        return 'fewer than %d angular-spectrum peaks in file(s) %s' % (self.g.S, files)

    @_on_device
    def check_status(self):
        self.check_chain_status()
        st = self.file_status().cpu().numpy()
        if st.any():
            raise ValueError(self._too_few_peaks(st))

    @_on_device
    def _chain_status(self):
        """Status word of the last chained KL-NMF launch(es) of this engine (0 = clean or not chained); synchronises the stream."""
        g = self.g
        torch.cuda.current_stream(self.device).synchronize()
        worst = 0
        for _, per, ws, _ in self._groups():
            worst |= _hip.klnmf_chain_status(ws, g.F, g.N, g.K, per)
        return worst

    chain_failed = _chain_status

    def check_chain_status(self):
        """A chained KL-NMF launch whose hand-over failed has turned W and H into NaN; say so instead of letting NaN travel on."""
        st = self._chain_status()
        if st:
            raise _hip.HipLibraryError('the chained KL-NMF launch did not hand over cleanly (status %d: %s): W and H of this batch are NaN.  '
                                       'GCCNMF_TUNE="21=0" runs the plain launches.'
                                       % (st, 'a consumer timed out' if st & 1 else 'a work list ran on more than one XCC'))

    # ---- views of device results in the reference's shapes ------------------------------------------
    def get_X(self):
        g = self.g
        return torch.view_as_complex(self.X)[:, :, :g.F, :g.T].cpu().numpy()

    def get_V(self):
        g = self.g
        return self.V[:, :g.F, :g.N].cpu().numpy()

    def get_C(self):
        g = self.g
        c = self.CC[:, :, :g.F, :g.T].cpu().numpy()
        return (c[:, 0] + 1j * c[:, 1]).astype(np.complex64)

    def get_WH(self):
        g = self.g
        return self.W[:, :g.F, :g.K].cpu().numpy(), self.H[:, :g.K, :g.N].cpu().numpy()

    def get_angular(self):
        g = self.g
        return self.ang[:, :g.D, :g.T].cpu().numpy(), self.mean_ang[:, :g.D].cpu().numpy()

    def get_tdoa_indexes(self):
        """(batch, S) int32, ascending per file; with numTargets='auto' S = maxTargets and the slots beyond a file's count hold -1."""
        return self.tdoa_idx.cpu().numpy()

    def get_num_sources(self):
        """(batch,) int64: the targets of every file -- with numTargets='auto' the count ``localize()`` found, else numTargets."""
        if not self.autoTargets:
            return np.full((self.batch,), self.g.S, dtype=np.int64)
        return (self.tdoa_idx >= 0).sum(dim=1).cpu().numpy().astype(np.int64)

    def get_count_status(self):
        """(batch,) int32 (numTargets='auto' only): 0 = counted, 1 = no peak to count, 2 = more than maxTargets, the highest kept."""
        if not self.autoTargets:
            raise ValueError("get_count_status needs numTargets='auto'")
        return self.status.cpu().numpy()

    def get_tdoa_tracks(self):
        """(batch, S, T) int32: the TDOA index of target i in frame t (tdoaTracking only)."""
        if not self.tdoaTracking:
            raise ValueError('get_tdoa_tracks needs tdoaTracking=True')
        return self.tracks[:, :, :self.g.T].cpu().numpy()

    def get_track_status(self):
        """(batch, T) int32: 0 = the frame had numTargets peaks, 1 = it took another frame's set, 3 = no frame of the file had enough."""
        if not self.tdoaTracking:
            raise ValueError('get_track_status needs tdoaTracking=True')
        return self.track_status[:, :self.g.T].cpu().numpy()

    def get_scores(self):
        g = self.g
        s = self.scores.view(self.batch, g.Kp, g.S, g.Tp)[:, :g.K, :, :g.T]
        return s.permute(0, 2, 1, 3).contiguous().cpu().numpy()

    def get_argmax(self):
        g = self.g
        return self.argmax[:, :g.K, :g.T].cpu().numpy()

    def get_spec(self):
        g = self.g
        s = torch.view_as_complex(self.spec)[:, :, :g.F, :g.T].cpu().numpy()
        return s.reshape(self.batch, g.S, 2, g.F, g.T)


def check_enhancement_target_index(targetTDOAIndex, batch, numTDOAs):
    """The ``targetTDOAIndex`` keyword of GCCNMFEnhancementEngine, no device needed: None (localise), one index for every file or one
    per file, whole numbers in [0, numTDOAs).  Returns None or an int32 (batch,) array; ValueError otherwise."""
    if targetTDOAIndex is None:
        return None
    tg = np.asarray(targetTDOAIndex)
    if tg.ndim not in (0, 1) or tg.dtype.kind not in 'iuf' or (tg.ndim == 1 and tg.shape[0] != int(batch)):
        raise ValueError('targetTDOAIndex must be None, one index or one index per file (%d), got shape %s' % (batch, tg.shape))
    if not np.isfinite(tg).all() or not np.array_equal(tg, np.round(tg)) or tg.min() < 0 or tg.max() >= int(numTDOAs):
        raise ValueError('targetTDOAIndex must be whole numbers in [0, %d), got %r' % (numTDOAs, targetTDOAIndex))
    return np.ascontiguousarray(np.broadcast_to(tg, (int(batch),)), dtype=np.int32)


class GCCNMFEnhancementEngine(GCCNMFEngine):
    """Offline speech enhancement of a batch: ONE talker against noise (the reference's "offline speech enhancement" workflow; DESIGN
    section 4e).  Every atom of every frame goes to the talker or to the noise by the atom's OWN TDOA -- the arg-max of its GCC-NMF
    score over the whole TDOA grid (csrc/atom_tdoa.hip; gccNMF/realtime/gccNMFProcessor.py:254,:259) -- compared with the talker's:

    ``targetMode='boxcar'``: talker where |i - target| < ``targetTDOAEpsilon`` (:263); ``'window'``: the soft mask
    exp(-(|i - target| / epsilon) ** ``targetTDOABeta``) / (1 + ``targetTDOANoiseFloor``) + noiseFloor (:265), noise = 1 - talker.
    (The constants TARGET_MODE_BOXCAR / TARGET_MODE_WINDOW_FUNCTION of realtime.py are taken too.)

    ``localize()`` picks ONE peak of each file's mean angular spectrum as the talker's direction (with ``tdoaTracking``: one per frame);
    ``targetTDOAIndex`` -- one index, or one per file -- skips the pick.  ``separate()`` returns (batch, 2, 2, L) waveforms ordered
    [talker, noise], and so do ``separate_batches`` and ``separate_pcm16``; ``get_atom_tdoa_indexes()`` (batch, K, T).  Everything in
    front of the masks is GCCNMFEngine's: ``dictionaryW``, ``numFreeAtoms``, ``tolerance``, ``divergence``, ``reconstruction``,
    ``spatialIterations``, ``gccPHATNLEnabled``.
    There is no ``numTargets`` keyword (two outputs), and no ragged form: ``lengths=`` raises ValueError."""

    def __init__(self, n_samples, *args, **kwargs):
        if 'numTargets' in kwargs:
            raise TypeError('GCCNMFEnhancementEngine takes no numTargets keyword: its outputs are the talker and the noise')
        if kwargs.pop('lengths', None) is not None:
            raise ValueError('GCCNMFEnhancementEngine has no ragged form: lengths= is not available')
        names = ('sampleRate', 'windowSize', 'hopSize', 'numTDOAs', 'microphoneSeparationInMetres')
        if len(args) > len(names):
            raise TypeError('GCCNMFEnhancementEngine takes at most %d positional arguments besides n_samples' % len(names))
        kwargs.update(zip(names, args))
        self.targetMode, self.targetTDOAEpsilon, self.targetTDOABeta, self.targetTDOANoiseFloor = _hip.check_enhancement_target(
            kwargs.pop('targetMode', 'boxcar'), kwargs.pop('targetTDOAEpsilon', 5.0), kwargs.pop('targetTDOABeta', 2.0),
            kwargs.pop('targetTDOANoiseFloor', 0.0))
        numTDOAs = int(kwargs.get('numTDOAs', 128))
        if not 3 <= numTDOAs <= _hip.ATOM_TDOA_MAX_D:
            raise ValueError('enhancement takes 3 to %d TDOAs, got %d' % (_hip.ATOM_TDOA_MAX_D, numTDOAs))
        fixed = check_enhancement_target_index(kwargs.pop('targetTDOAIndex', None), kwargs.get('batch', 1), numTDOAs)
        super(GCCNMFEnhancementEngine, self).__init__(n_samples, numTargets=2, **kwargs)
        g, B, dev = self.g, self.batch, self.device
        with torch.cuda.device(dev):
            self.scores = self.ws_scores = None              # the per-target score stage does not run here
            self.fixedTargetTDOAIndex = fixed is not None
            self.tdoa_idx = torch.zeros((B, 1), dtype=torch.int32, device=dev)
            if fixed is not None:
                self.tdoa_idx.copy_(torch.from_numpy(fixed).view(B, 1))
            if self.tdoaTracking:
                self.tracks = torch.zeros((B, 1, g.Tp), dtype=torch.int32, device=dev)
            self.atom_tdoa = torch.zeros((B, g.Kp, g.Tp), dtype=torch.int16, device=dev)         # uint16 bits
            self.soft_masks = torch.zeros((B, 2, g.Kp, g.Tp), dtype=torch.float32, device=dev) if self.targetMode else None

    def _per_frame(self):
        return self.tdoaTracking and not self.fixedTargetTDOAIndex

    @_on_device
    def localize(self):
        g = self.g
        _hip.angular_spectrogram(self.CC, self.trig, g.F, g.T, g.D, self.batch, self.ang, self.mean_ang,
                                 nl_alpha=self.gccPHATNLAlpha if self.gccPHATNLEnabled else None)
        if self.fixedTargetTDOAIndex:
            return
        _hip.pick_tdoa_peaks(self.mean_ang, g.D, g.Dp, 1, self.batch, self.tdoa_idx, self.status)
        if self.tdoaTracking:
            _hip.pick_tdoa_tracks(self.ang, g.D, g.T, 1, self.localizationWindowSize, self.batch, self.tracks, self.track_status)

    def file_status(self):
        if self.fixedTargetTDOAIndex:
            return torch.zeros_like(self.status)
        return super(GCCNMFEnhancementEngine, self).file_status()

    @_on_device
    def masks(self):
        g = self.g
        _hip.atom_tdoa_indexes(self.CC, self.trig, self.W, g.F, g.T, g.K, g.D, self.batch, self.atom_tdoa)
        _hip.enhancement_masks(self.atom_tdoa, self.tracks if self._per_frame() else self.tdoa_idx, g.T, g.K, self.batch,
                               None if self.targetMode else self.argmax, self.soft_masks, window=self.targetMode,
                               eps=self.targetTDOAEpsilon, beta=self.targetTDOABeta, noise_floor=self.targetTDOANoiseFloor,
                               per_frame=self._per_frame())

    @_on_device
    def reconstruct(self):
        g = self.g
        _hip.reconstruct(self.W, self.H, None if self.targetMode else self.argmax, self.soft_masks, self.X, self.V, g.F, g.T, g.K, 2,
                         self.batch, self.spec, mode=self.reconstruction, workspace=self._reconstruct_workspace(),
                         iterations=self.spatialIterations)

    def get_atom_tdoa_indexes(self):
        """(batch, K, T) int32: the TDOA index of every atom in every frame (after masks())."""
        g = self.g
        return (self.atom_tdoa[:, :g.K, :g.T].to(torch.int32) & 0xffff).cpu().numpy()

    def get_enhancement_masks(self):
        """(batch, 2, K, T) float32 [talker, noise] (after masks()): the soft masks, or the boxcar image expanded to 0 / 1."""
        g = self.g
        if self.targetMode:
            return self.soft_masks[:, :, :g.K, :g.T].cpu().numpy()
        noise = self.argmax[:, :g.K, :g.T].to(torch.float32)
        return torch.stack([1 - noise, noise], dim=1).cpu().numpy()


class RaggedGCCNMFEngine(object):
    """A batch of mixtures of DIFFERENT lengths (the reference separates a file of any length per call, gccNMF/runGCCNMF.py:30-36; sharding
    "independent mixture files" over GPUs means files as they come).  ``lengths``: samples per file, in the caller's order.

    KL-NMF -- 98 % of the path -- runs over ALL files in ONE chained launch whose work lists hold each file's own column tiles
    (gccnmf_klnmf_ragged: padding to the 64-column tile only, the files dealt out to the XCDs by length).  The one-shot stages (STFT,
    localisation, masks, reconstruction, iSTFT) run per distinct length, on the ordinary engine of that length.  A file's results are bit
    for bit those it gets in an equal-length batch.  Where the library has no chained form for the shape (GCCNMF_ERR_UNSUPPORTED: short
    dictionaries, a handful of files) the files of each length run their KL-NMF as a batch of their own -- and so they do with
    ``divergence`` = 'is' / 'euclidean' and with ``temporalContinuity`` > 0 (GCCNMFEngine states the keywords), which have no ragged launch."""

    def __init__(self, lengths, sampleRate=16000, windowSize=1024, hopSize=256, numTDOAs=128, microphoneSeparationInMetres=1.0,
                 numTargets=3, dictionarySize=None, numIterations=100, sparsityAlpha=0, epsilon=1e-16, seedValue=0,
                 windowFunction=np.hanning, device='cuda:0', klnmf_flags=0, dictionaryW=None, initialH='random', reconstruction='direct',
                 gccPHATNLEnabled=False, gccPHATNLAlpha=2.0, tdoaTracking=False, localizationWindowSize=None, tolerance=None, checkEvery=10,
                 maxTargets=None, spatialIterations=0, divergence='kl', temporalContinuity=0.0):
        self.tolerance, self.checkEvery, numIterations = _hip.check_convergence(tolerance, checkEvery, numIterations)
        self.temporalContinuity = check_temporal_continuity(temporalContinuity, dictionaryW, 0, divergence, tolerance, klnmf_flags, None,
                                                            windowSize, dictionarySize, len(lengths))
        self.divergence = _hip.check_divergence(divergence, int(windowSize) // 2 + 1, None if dictionarySize is None else int(dictionarySize))
        if self.divergence != 'kl':
            if dictionaryW is not None:
                raise ValueError('divergence=%r learns every atom: not available with dictionaryW or numFreeAtoms' % (self.divergence,))
            if klnmf_flags & 6:
                raise ValueError('divergence=%r cannot be combined with the concurrent-groups or unfused-W-update bits of klnmf_flags'
                                 % (self.divergence,))
        self.autoTargets, slots = _hip.check_auto_targets(numTargets, maxTargets, tdoaTracking)
        self.reconstruction = check_reconstruction(reconstruction, slots)
        self.spatialIterations = _hip.check_spatial_iterations(spatialIterations, self.reconstruction)
        self.gccPHATNLEnabled, self.gccPHATNLAlpha = check_gcc_phat_nl(gccPHATNLEnabled, gccPHATNLAlpha)
        self.tdoaTracking, self.localizationWindowSize = check_tdoa_tracking(tdoaTracking, localizationWindowSize, slots)
        if not torch.cuda.is_available():
            raise _hip.HipLibraryError('no ROCm device visible: the GCC-NMF HIP path has no CPU fallback')
        self.lib = _hip.lib()
        self.device = torch.device(device)
        self.lengths = [int(n) for n in lengths]
        if not self.lengths:
            raise ValueError('no files')
        self.batch = len(self.lengths)
        self.iters, self.alpha, self.eps = int(numIterations), float(sparsityAlpha), float(epsilon)
        self.klnmf_flags = klnmf_flags
        kw = dict(sampleRate=sampleRate, windowSize=windowSize, hopSize=hopSize, numTDOAs=numTDOAs,
                  microphoneSeparationInMetres=microphoneSeparationInMetres, numTargets=numTargets, dictionarySize=dictionarySize,
                  numIterations=numIterations, sparsityAlpha=sparsityAlpha, epsilon=epsilon, seedValue=seedValue,
                  windowFunction=windowFunction, device=device, klnmf_flags=klnmf_flags, dictionaryW=dictionaryW, initialH=initialH,
                  reconstruction=reconstruction, gccPHATNLEnabled=gccPHATNLEnabled, gccPHATNLAlpha=gccPHATNLAlpha,
                  tdoaTracking=tdoaTracking, localizationWindowSize=localizationWindowSize,     # (each file's windows end at its own T)
                  tolerance=tolerance, checkEvery=checkEvery, maxTargets=maxTargets, spatialIterations=spatialIterations,
                  divergence=self.divergence, temporalContinuity=self.temporalContinuity)
        # one ordinary engine per distinct length: its files (caller's indexes, ascending) are its batch
        self.files_of = {}
        for i, n in enumerate(self.lengths):
            self.files_of.setdefault(n, []).append(i)
        self.sub = dict((n, GCCNMFEngine(n, batch=len(idx), nmf_groups=1, **kw)) for n, idx in sorted(self.files_of.items()))
        longest = self.sub[max(self.sub)]
        self.g = g = longest.g                                   # geometry of the longest file: the pitch of every file's V / H block
        self.N = [self.sub[n].g.N for n in self.lengths]       # columns per file
        self.frames = [self.sub[n].g.T for n in self.lengths]
        with torch.cuda.device(self.device):
            z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)
            self.ragged = None
            # a fixed dictionary: each length's engine runs its own one-launch call; a tolerance: each length's files converge as a batch of their
            # own; IS / Euclid: the ragged launch is KL only, each length runs as a batch of its own
            if len(self.sub) > 1 and dictionaryW is None and self.tolerance is None and self.divergence == 'kl' and not self.temporalContinuity:
                ws = self.lib.gccnmf_klnmf_ragged_workspace_floats(g.F, g.N, g.K, self.batch)
                if ws > 0:
                    self.ragged = dict(V=z(self.batch, g.Fp, g.Np), W=z(self.batch, g.Fp, g.Kp), H=z(self.batch, g.Kp, g.Np), ws=z(ws),
                                       N=(ctypes.c_int * self.batch)(*self.N))
        self.ragged_klnmf_used = None                            # set by run(): True = one ragged launch, False = one call per length

    def klnmf(self):
        """KL-NMF of every file: one ragged chained launch, or -- where the library has none for this shape -- one call per length."""
        with torch.cuda.device(self.device):
            r = self.ragged
            if r is not None:
                g = self.g
                for n, e in self.sub.items():
                    idx = torch.as_tensor(self.files_of[n], device=self.device)
                    r['V'][idx, :, :e.g.Np] = e.V                # (columns beyond a file's own stay zero: never written)
                    r['W'][idx] = e.W0
                    r['H'][idx, :, :e.g.Np] = e.H0
                rc = self.lib.gccnmf_klnmf_ragged(_ptr(r['V']), _ptr(r['W']), _ptr(r['H']), _ptr(r['ws']), g.F, r['N'], g.N, g.K, self.batch,
                                                  self.iters, self.alpha, self.eps, self.klnmf_flags, _stream())
                if rc == 0:
                    self._ragged_ran = True
                    for n, e in self.sub.items():
                        idx = torch.as_tensor(self.files_of[n], device=self.device)
                        e.W.copy_(r['W'][idx])
                        e.H.copy_(r['H'][idx, :, :e.g.Np])
                    self.ragged_klnmf_used = True
                    return
                if rc != 3:                                      # GCCNMF_ERR_UNSUPPORTED: no chained form for this shape
                    _hip.check(rc, 'gccnmf_klnmf_ragged')
            self.ragged_klnmf_used = False
            for e in self.sub.values():
                e.klnmf()

    def run(self, stft=True):
        if stft:
            for e in self.sub.values():
                e.stft()
        self.klnmf()
        for e in self.sub.values():
            e.localize()
            e.masks()
            e.reconstruct()
            e.istft()

    def upload(self, mixtures):
        """mixtures[i]: (2, lengths[i]) float32 samples of file i."""
        if len(mixtures) != self.batch:
            raise ValueError('expected %d mixtures' % self.batch)
        for n, e in self.sub.items():
            e.upload(np.stack([np.asarray(mixtures[i], dtype=np.float32) for i in self.files_of[n]]))

    def separate(self, mixtures):
        """list of (2, lengths[i]) float32 host arrays -> list of (S, 2, hop * (T_i - 1)) float32 host waveforms, in the caller's order."""
        self.upload(mixtures)
        self.run()
        out = [None] * self.batch
        if self.ragged_klnmf_used:
            torch.cuda.current_stream(self.device).synchronize()
            st = _hip.klnmf_chain_status(self.ragged['ws'], self.g.F, self.g.N, self.g.K, self.batch)
            if st:
                raise _hip.HipLibraryError('the ragged chained KL-NMF launch did not hand over cleanly (status %d): W and H are NaN' % st)
        for n, e in self.sub.items():
            y = e.y.cpu().numpy()
            e.check_status()
            for k, i in enumerate(self.files_of[n]):
                out[i] = y[k]
        return out

    def _per_file(self, values):
        return [values[n][self.files_of[n].index(i)] for i, n in enumerate(self.lengths)]

    def get_divergence(self):
        """(batch,) float64 in the caller's order: D(V || W.H) of every file's factors (after klnmf())."""
        return np.array(self._per_file(dict((n, e.get_divergence()) for n, e in self.sub.items())), dtype=np.float64)

    def get_iterations(self):
        """(batch,) int64 in the caller's order: the iterations each file ran.  Needs a tolerance."""
        return np.array(self._per_file(dict((n, e.get_iterations()) for n, e in self.sub.items())), dtype=np.int64)

    def get_divergence_trace(self):
        """One (checks_i + 1,) float64 array per file, in the caller's order (the files of each length run, and are checked, as a batch
        of their own).  Needs a tolerance."""
        return self._per_file(dict((n, e.get_divergence_trace().T) for n, e in self.sub.items()))

    def get_num_sources(self):
        """(batch,) int64 in the caller's order: the targets of every file (numTargets='auto': the count found in it)."""
        return np.array(self._per_file(dict((n, e.get_num_sources()) for n, e in self.sub.items())), dtype=np.int64)

    def get_tdoa_tracks(self):
        """One (S, T_i) int32 array per file, in the caller's order (tdoaTracking only)."""
        return self._per_file(dict((n, e.get_tdoa_tracks()) for n, e in self.sub.items()))

    def get_track_status(self):
        """One (T_i,) int32 array per file, in the caller's order (tdoaTracking only)."""
        return self._per_file(dict((n, e.get_track_status()) for n, e in self.sub.items()))

    def file(self, i):
        """(engine of file i's length, its index in that engine's batch): ``e, k = eng.file(i); e.get_WH()[0][k]``."""
        n = self.lengths[i]
        return self.sub[n], self.files_of[n].index(i)
