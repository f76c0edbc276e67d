"""Streaming (real-time) GCC-NMF on MI355X -- the reference's ``gccNMF/realtime/gccNMFProcessor.py`` frame processor
(a Theano graph there) and ``gccNMF/realtime/utils.py`` overlap-add, as one C-ABI call per audio block
(``gccnmf_rt_process_block``, csrc/rt.hip).

``GCCNMFProcessor`` keeps the reference's constructor arguments, attributes and methods
(``processFrames(windowedSamples)``, ``setTargetTDOARange``, ``reset``); ``StreamingGCCNMF`` is the fused
block-in / block-out path (input ring, frames, mask, synthesis, overlap-add and TDOA tracking all on device).
``StreamingGCCNMFBank`` runs S such streams of one configuration in the same device call per block, each bit for bit a
``StreamingGCCNMF`` of its own.
``targetMode = TARGET_MODE_MULTIPLE`` separates ``numSources`` talkers per stream instead of enhancing one (the ``targets`` layout of ``_hip.rt_process_block``): one-hot
arg-max-over-targets coefficient masks, one output per target, the N largest peaks of the gccPHAT window mean tracked online.
No CPU fallback: without the library / a device the constructor raises ``HipLibraryError``.
"""
import numpy as np
import torch

from . import _hip
from ._hip import MAX_SOURCES, MAX_BANK_STREAMS           # noqa: F401  (the limits of the block call's layouts, public here)
from .engine import padded, fft_twiddles, _on_device

SPEED_OF_SOUND_IN_METRES_PER_SECOND = 340.29
TARGET_MODE_BOXCAR = 0                   # gccNMFProcessor.py:35-37
TARGET_MODE_MULTIPLE = 1
TARGET_MODE_WINDOW_FUNCTION = 2


def asymmetricWindows(windowSize, synthesisSize):
    """Low-latency analysis / synthesis window pair (README.md:74-78; construction after Mauler & Martin 2007): a long analysis window
    for spectral resolution, a synthesis window on the last ``synthesisSize`` samples only.  analysis * synthesis is the periodic Hann
    of length synthesisSize, which overlap-adds to 1 at hopSize = synthesisSize / 2: algorithmic latency synthesisSize samples."""
    K, M = int(windowSize), int(synthesisSize) // 2
    if synthesisSize % 2 or not 0 < 2 * M <= K:
        raise ValueError('synthesisSize must be even and at most windowSize')
    n = np.arange(K, dtype=np.float64)
    long_rise = np.sqrt(0.5 * (1.0 - np.cos(2.0 * np.pi * n / (2 * (K - M))))) if K > M else np.ones(K)
    short = 0.5 * (1.0 - np.cos(2.0 * np.pi * (n - (K - 2 * M)) / (2 * M)))
    analysis = np.where(n < K - M, long_rise, np.sqrt(np.maximum(short, 0.0)))
    with np.errstate(divide='ignore', invalid='ignore'):
        synthesis = np.where(n < K - 2 * M, 0.0, np.where(n < K - M, short / long_rise, np.sqrt(np.maximum(short, 0.0))))
    return analysis.astype(np.float32), synthesis.astype(np.float32)


def _device():
    if not torch.cuda.is_available():
        raise _hip.HipLibraryError('no ROCm device visible: gcc_nmf_amd has no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


class GCCNMFProcessor(object):
    """gccNMF/realtime/gccNMFProcessor.py:167-275.  ``dictionariesW[dictionaryType][dictionarySize]`` is the (F, K) float32
    dictionary (:241).  ``numTDOAs`` is an attribute the reference receives through its parameter queue before ``reset()``;
    here it is also a constructor keyword, and so is ``numSources`` (the talkers separated with ``targetMode = TARGET_MODE_MULTIPLE``,
    1..8; like the reference, :131, a new value takes effect with ``reset()``).

    Multiple mode (parity unpinned: the reference defines the mode, :35-37, and never built it): atom k of frame t goes to the target
    TDOA index whose GCC-NMF score is largest (``gccNMFFunctions.py:137-143`` on the streaming scores), every target has its own mask,
    synthesis and output, and the online localisation keeps the ``numSources`` largest peaks of the gccPHAT window mean as the next
    block's targets, in ascending order -- target identity is left-to-right order, so two talkers that cross swap outputs.  The host
    mirrors ``gccPHATHistory`` and ``inputSpectrogramHistory`` are filled as in the other modes and ``tdoaHistory`` receives the N
    indexes as an (N, 1) column; ``outputSpectrogramHistory`` and ``coefficientMaskHistories`` are not filled in this mode.

    ``gccPHATNLEnabled`` (default False) / ``gccPHATNLAlpha`` (default 2.0): the reference's GCC-NONLIN settings (config.py:42-43,
    a processor parameter that needs ``reset()``, gccNMFProcessor.py:131-132; parity unpinned: the reference has no code for them).
    Attributes and constructor keywords; a new value takes effect with ``reset()``.  When enabled, gccPHAT is
    nanmean_f 1 - tanh(alpha sqrt(max(0, 1 - Re(C e^{-j w tau})))) (Blandin, Ozerov & Vincent 2012; BSS-Locate's sqrt(2 - 2 re) form
    is this one with alpha * sqrt(2)) in all three target modes; the history, window mean and arg-max / peak rule are unchanged and the
    GCC-NMF scores stay PHAT.

    ``spatialFilterEnabled`` (default False) / ``spatialFilterFrames`` (default 128, 0.5 s at the low-latency hop): the online spatial
    (multichannel Wiener) filter behind the mask, the streaming form of the offline ``reconstruction='spatial'`` (no counterpart in the
    reference).  The masked
    spectra give each component (multiple mode: the N targets; the single-target modes: the talker and the residual X - Y) a power and
    a 2 x 2 spatial covariance, the latter a trace-normalised exponential average with a time constant of ``spatialFilterFrames`` frames
    that is carried from block to block; the stereo mixture vector is then filtered per component (include/gccnmf_hip.h states the
    recursion).  Attributes and constructor keywords; a new value takes effect with the next call (no ``reset()`` needed); ``reset()``
    clears the covariances."""

    def __init__(self, sampleRate, windowSize, numTimePerChunk, dictionariesW, dictionaryType, dictionarySize, numHUpdates,
                 microphoneSeparationInMetres, localizationEnabled, localizationWindowSize, gccPHATHistory=None, tdoaHistory=None,
                 inputSpectrogramHistory=None, outputSpectrogramHistory=None, coefficientMaskHistories=None, numTDOAs=64,
                 numTDOAHistory=128, analysisWindow=None, synthesisWindow=None, numSources=2, gccPHATNLEnabled=False,
                 gccPHATNLAlpha=2.0, spatialFilterEnabled=False, spatialFilterFrames=_hip.DEFAULT_SPATIAL_FILTER_FRAMES):
        # any even size like the reference (numpy.fft.rfft / irfft, gccNMFProcessor.py:202,:231): powers of two from 64 up take the
        # radix-2 LDS transform, every other even size the direct-sum kernels of csrc/rt.hip
        if int(windowSize) != windowSize or int(windowSize) < 4 or int(windowSize) > 4096 or int(windowSize) % 2:
            raise ValueError('windowSize=%r is not supported by the HIP frame processor: an even size from 4 to 4096' % (windowSize,))
        _check_num_sources(numSources)
        self.gccPHATNLEnabled, self.gccPHATNLAlpha = gccPHATNLEnabled, gccPHATNLAlpha
        self._gcc_phat_nl()               # ValueError before the constructor looks for a device
        self.spatialFilterEnabled, self.spatialFilterFrames = spatialFilterEnabled, spatialFilterFrames
        self._spatial_word()
        self.lib = _hip.lib()
        self.device = _device()
        self.sampleRate, self.windowSize, self.numTimePerChunk = sampleRate, int(windowSize), int(numTimePerChunk)
        self.dictionariesW, self.dictionaryType, self.dictionarySize = dictionariesW, dictionaryType, dictionarySize
        # The reference accepts numHUpdates and never uses it (:168).  Here 0 (the reference's config default, config.py:73) IS the
        # reference's mask; n > 0 runs n KL-NMF coefficient updates per frame with W fixed (gccNMFFunctions.py:76) -- the "NMF
        # coefficients are inferred frame-by-frame" of README.md:74, for which the checkout holds no code (parity unpinned).
        self.numHUpdates = int(numHUpdates or 0)
        self.microphoneSeparationInMetres = microphoneSeparationInMetres
        self.localizationEnabled, self.localizationWindowSize = localizationEnabled, int(localizationWindowSize)
        self.numTDOAs, self.numTDOAHistory = int(numTDOAs), int(numTDOAHistory)
        # host mirrors for the GUI (gccNMFProcessor.py:180-184): any object with SharedMemoryCircularBuffer's set() (utils.py:34-70);
        # filled after every call from ONE small download of the device state (:211-229)
        self.gccPHATHistory, self.tdoaHistory = gccPHATHistory, tdoaHistory
        self.inputSpectrogramHistory, self.outputSpectrogramHistory = inputSpectrogramHistory, outputSpectrogramHistory
        self.coefficientMaskHistories = coefficientMaskHistories
        self.generation = 0
        self.separationEnabled = True
        self.targetMode = TARGET_MODE_WINDOW_FUNCTION
        self.windowFunction = np.sqrt(np.hamming(self.windowSize).astype(np.float32))[:, np.newaxis]      # :186
        self.synthesisWindowFunction = self.windowFunction
        if analysisWindow is not None:                    # low-latency extension: separate (asymmetric) windows, see asymmetricWindows()
            a = np.asarray(analysisWindow, np.float32)
            sy = np.asarray(synthesisWindow if synthesisWindow is not None else analysisWindow, np.float32)
            if a.shape != (self.windowSize,) or sy.shape != (self.windowSize,):
                raise ValueError('analysisWindow / synthesisWindow must have windowSize samples')
            self.windowFunction, self.synthesisWindowFunction = a[:, np.newaxis], sy[:, np.newaxis]
        self._target_host = np.array([10.0, 2.0, 1.0, 0.0], np.float32)                                   # :195-198
        self.numSources = numSources
        self.reset()

    def _gcc_phat_nl(self):
        """Word 6 of the target row for the current attributes: gccPHATNLAlpha when GCC-NONLIN is enabled, 0.0 (PHAT) when not."""
        enabled, alpha = _hip.check_gcc_phat_nl(self.gccPHATNLEnabled, self.gccPHATNLAlpha)
        return np.float32(alpha if enabled else 0.0)

    def _spatial_word(self):
        """Word 7 of the target row for the current attributes: spatialFilterFrames when the filter is enabled, 0.0 (off) when not."""
        enabled, frames = _hip.check_spatial_filter(self.spatialFilterEnabled, self.spatialFilterFrames)
        return np.float32(frames if enabled else 0.0)

    def _apply_spatial(self):
        """Before a call (never inside a graph capture): the row word follows the attributes, and the covariances start over when the
        components change meaning (into or out of multiple mode).  Returns whether the call runs the filter."""
        word, multi = self._spatial_word(), self.multiple()
        if word != self._spatial_row:
            self.dTarget[7] = float(word)
            self._spatial_row = word
        if word > 0 and self._spatial_multi != multi:
            self.dSpatial.zero_()
            self._spatial_multi = multi
        return bool(word > 0)

    # ---- reference API ------------------------------------------------------------------------------------------
    @_on_device
    def reset(self):
        """:233-270 (buildTheanoFunctions): tables and buffers for the current dictionary / TDOA grid."""
        dev = self.device
        self.generation += 1              # every device buffer below is re-allocated: captured graphs that hold the old pointers are stale
        self.W = np.asarray(self.dictionariesW[self.dictionaryType][self.dictionarySize], np.float32)
        self.numFrequencies, self.numAtom = self.W.shape
        if self.numFrequencies != self.windowSize // 2 + 1:
            raise ValueError('dictionary has %d rows, window size %d needs %d' % (self.numFrequencies, self.windowSize, self.windowSize // 2 + 1))
        F, K, D, Tc = self.numFrequencies, self.numAtom, self.numTDOAs, self.numTimePerChunk
        NS = _check_num_sources(self.numSources)
        nl_word = self._gcc_phat_nl()
        self.Kp, self.Dp = -(-K // 64) * 64, -(-D // 32) * 32
        self.frequenciesInHz = np.linspace(0, self.sampleRate / 2, F).astype(np.float32)                 # :245
        self.maxTDOA = self.microphoneSeparationInMetres / SPEED_OF_SOUND_IN_METRES_PER_SECOND
        self.hypothesisTDOAs = np.linspace(-self.maxTDOA, self.maxTDOA, D).astype(np.float32)            # :247
        self.expJOmegaTau = np.exp(np.outer(self.frequenciesInHz, -(2j * np.pi) * self.hypothesisTDOAs)).astype(np.complex64)
        z = lambda *shape, **kw: torch.zeros(shape, dtype=kw.get('dtype', torch.float32), device=dev)
        self.dW = padded(self.W, (F, self.Kp), dev)
        self.dCos = padded(np.ascontiguousarray(self.expJOmegaTau.real), (F, self.Dp), dev)
        self.dSin = padded(np.ascontiguousarray(-self.expJOmegaTau.imag), (F, self.Dp), dev)
        self.dWindow = torch.from_numpy(np.ascontiguousarray(self.windowFunction[:, 0])).to(dev)
        self.dSynthWindow = torch.from_numpy(np.ascontiguousarray(self.synthesisWindowFunction[:, 0])).to(dev)
        self.dColsum = padded(self.W.sum(axis=0, dtype=np.float32), (self.Kp,), dev)          # sum_f W: denominator of the H update
        self.dHcoef, self.dRv = z(self.Kp, Tc, 2), z(F, Tc, 2)
        N = self.windowSize
        if N >= 64 and N & (N - 1) == 0:
            self.dTwiddle = torch.from_numpy(fft_twiddles(N)).to(dev)
        else:           # the full-circle table of the direct-sum kernels: (cos, sin)(2 pi k / N), float64 on the host like the twiddles
            ang = 2.0 * np.pi * np.arange(N, dtype=np.float64) / N
            self.dTwiddle = torch.from_numpy(np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)).reshape(-1)).to(dev)
        # what the host mirrors are computed from lives in ONE block, so that they cost one download per call: X | Y | HMask | gccPHAT | target
        # (the target row is 16 words: {index, epsilon, beta, noiseFloor, -, -, nlAlpha, -, tau_0 .. tau_7}; words 8.. are multiple mode's)
        sizes = [2 * F * Tc * 2, 2 * F * Tc * 2, self.Kp * Tc, D * Tc, 16]
        offs = np.concatenate([[0], np.cumsum([-(-n // 4) * 4 for n in sizes])])
        self.dMirror = z(int(offs[-1]))
        part = lambda i, *shape: self.dMirror[int(offs[i]):int(offs[i]) + sizes[i]].view(*shape)
        self.dX, self.dY, self.dC = part(0, 2, F, Tc, 2), part(1, 2, F, Tc, 2), z(F, Tc, 2)
        self.dHMask, self.dArgmax = part(2, self.Kp, Tc), z(self.Kp, Tc, dtype=torch.int32)
        self.dTfMask, self.dGccPhat = z(2, F, Tc), part(3, D, Tc)     # tfMask: [F][Tc] used without coefficient inference, [2][F][Tc] with
        # the gccPHAT history and, behind it, the spatial filter's covariances [NC][F][4] (NC = 2 or numSources): one buffer, the block
        # call's `hist`
        at = _hip.rt_spatial_state_offset(D, self.numTDOAHistory)
        self.dHistState = z(at + _hip.rt_spatial_state_floats(F, max(NS, 2)))
        self.dHist, self.dSpatial = self.dHistState[:D * self.numTDOAHistory].view(D, self.numTDOAHistory), self.dHistState[at:]
        self.dHistPos = z(1, dtype=torch.int32)
        self.dTarget = part(4, 16)
        self.dTarget[:4].copy_(torch.from_numpy(self._target_host))
        self._nl_word = nl_word                           # GCC-NONLIN as this reset() saw it: alpha, or 0 = PHAT
        self.dTarget[6] = float(nl_word)
        self._spatial_row, self._spatial_multi, self._spatial_on = np.float32(0.0), None, False      # word 7 as the device has it
        self._mirror_offs, self._mirror_sizes, self._mirror_host = offs, sizes, None
        # _target_dirty: a device call ran with the online localisation on since the value was last known on the host
        self._calls, self._target_dirty, self._target_value, self._target_pin = 0, False, float(self._target_host[0]), None
        self.dFramesIn, self.dFramesOut = z(2, Tc, self.windowSize), z(2, Tc, self.windowSize)
        # multiple mode: N masks, masked spectra and frames (the other buffers are shared with the single-target modes)
        self._sources = NS
        self.dYm, self.dHMaskm, self.dTfMaskm = z(NS, 2, F, Tc, 2), z(NS, self.Kp, Tc), z(NS, 2, F, Tc)
        self.dFramesOutM = z(NS, 2, Tc, self.windowSize)
        self._indexes_host = default_target_indexes(NS, D)
        self.dTarget[8:8 + NS].copy_(torch.from_numpy(self._indexes_host))
        self._indexes_dirty, self._indexes_pin = False, None

    @_on_device
    def setTargetTDOARange(self, targetTDOAIndex, targetTDOAEpsilon, targetTDOABeta, targetTDOANoiseFloor):
        """:272-275"""
        self._target_host = np.array([targetTDOAIndex, targetTDOAEpsilon, targetTDOABeta, targetTDOANoiseFloor], np.float32)
        self.dTarget[:4].copy_(torch.from_numpy(self._target_host))
        self._target_value, self._target_dirty = float(self._target_host[0]), False

    @_on_device
    def setTargetTDOAIndexes(self, indexes):
        """Multiple mode's targets (the reference's ``targetTDOAIndexes`` message, gccNMFProcessor.py:108-111): ``numSources`` integer
        TDOA indexes in [0, numTDOAs).  The online localisation rewrites them after every block while it is enabled."""
        v = _check_target_indexes(indexes, self._sources, self.numTDOAs)
        self.dTarget[8:8 + self._sources].copy_(torch.from_numpy(v))
        self._indexes_host, self._indexes_dirty = v, False

    @property
    def targetTDOAIndexes(self):
        """(numSources,) multiple mode's target indexes, cached like ``targetTDOAIndex`` (fetched only when the tracking ran since the
        last read)."""
        if self._indexes_dirty:
            if self._indexes_pin is None:
                self._indexes_pin = torch.zeros(16, dtype=torch.float32).pin_memory()
            with torch.cuda.device(self.device):
                self._indexes_pin.copy_(self.dTarget, non_blocking=True)
                torch.cuda.current_stream(self.device).synchronize()
            self._indexes_host, self._indexes_dirty = self._indexes_pin.numpy()[8:8 + self._sources].copy(), False
        return self._indexes_host.copy()

    def multiple(self):
        """True when the next call runs multiple mode; then ``numSources`` must be the value the last ``reset()`` saw."""
        if int(self.targetMode) != TARGET_MODE_MULTIPLE:
            return False
        if int(self.numSources) != self._sources:
            raise ValueError('numSources changed from %d to %r: call reset() first' % (self._sources, self.numSources))
        return True

    @property
    def targetTDOAIndex(self):
        """The tracked target TDOA index.  Only the online localisation (csrc/rt.hip) changes it on the device, and the masks always use the
        device value -- so after tracking has run and ``localizationEnabled`` is switched off (the reference toggles it at run time,
        gccNMFProcessor.py:112-116), the LAST TRACKED index stays the answer, not what setTargetTDOARange once set.  A device call that ran
        with the localisation on marks the host copy stale; the value is then fetched at most once (from the history mirror when that
        was downloaded anyway, else one 16-byte page-locked copy) -- repeated reads never touch the device."""
        if self._target_dirty:
            if self._target_pin is None:
                self._target_pin = torch.zeros(4, dtype=torch.float32).pin_memory()
            with torch.cuda.device(self.device):
                self._target_pin.copy_(self.dTarget[:4], non_blocking=True)
                torch.cuda.current_stream(self.device).synchronize()
            self._target_value, self._target_dirty = float(self._target_pin[0]), False
        return self._target_value

    def _tables(self):
        """The read-only pointer arguments of the block call, in its order: W .. colsumW."""
        return self.dW, self.dCos, self.dSin, self.dWindow, self.dSynthWindow, self.dTwiddle, self.dColsum

    def _settings(self, hop, block):
        """The integer arguments of the block call in front of its mode word, in its order: windowSize .. localization_window."""
        return (self.windowSize, hop, block, self.numAtom, self.Kp, self.numTDOAs, self.Dp, self.numTDOAHistory, self.targetMode,
                self.separationEnabled, self.localizationEnabled, self.localizationWindowSize)

    @_on_device
    def _call(self, block_in, block_out, in_ring, out_ring, hop, block, out_delay_blocks=2, frames=False, localize='with'):
        """out_ring / block_out: [N][2][...] in multiple mode."""
        self._calls += 1
        multi = self.multiple()
        spatial = self._spatial_on and bool(self.separationEnabled)
        if self.localizationEnabled:
            if multi:
                self._indexes_dirty = True
            else:
                self._target_dirty = True
        Y, HMask, tfMask = (self.dYm, self.dHMaskm, self.dTfMaskm) if multi else (self.dY, self.dHMask, self.dTfMask)
        # the multi-target row always has word 6; the single-target call is told when its row does
        _hip.rt_process_block(block_in, block_out, in_ring, out_ring, self.dX, Y, self.dC, HMask, self.dArgmax, tfMask, self.dHist,
                              self.dHistPos, self.dTarget, self.dGccPhat, *self._tables(), self.dHcoef, self.dRv,
                              *self._settings(hop, block), self.numHUpdates, out_delay_blocks, frames=frames, localize=localize,
                              targets=self._sources if multi else None, nl_row=not multi and (self._nl_word > 0 or spatial),
                              spatial=spatial)

    @_on_device
    def processFrames(self, windowedSamples):
        """:201-231.  (2, windowSize, Tc) windowed-sample frames -> (2, windowSize, Tc) processed frames (float32); in multiple mode
        (numSources, 2, windowSize, Tc), one set of frames per target."""
        ws = np.asarray(windowedSamples, np.float32)
        Tc = self.numTimePerChunk
        if ws.shape != (2, self.windowSize, Tc):
            raise ValueError('expected windowedSamples of shape %s, got %s' % ((2, self.windowSize, Tc), ws.shape))
        self.dFramesIn.copy_(torch.from_numpy(np.ascontiguousarray(ws.transpose(0, 2, 1))))
        self._spatial_on = self._apply_spatial()
        # hop = windowSize, block = Tc * windowSize describes Tc back-to-back frames to the kernels' start0/step arithmetic
        if self.multiple():
            self._call(None, None, self.dFramesIn, self.dFramesOutM, self.windowSize, Tc * self.windowSize, frames=True)
            out = self.dFramesOutM.cpu().numpy().transpose(0, 1, 3, 2)
        else:
            self._call(None, None, self.dFramesIn, self.dFramesOut, self.windowSize, Tc * self.windowSize, frames=True)
            out = self.dFramesOut.cpu().numpy().transpose(0, 2, 1)
        self.fill_histories()
        return out

    def wants_histories(self):
        return any(h is not None for h in (self.gccPHATHistory, self.tdoaHistory, self.inputSpectrogramHistory,
                                           self.outputSpectrogramHistory)) or bool(self.coefficientMaskHistories)

    @_on_device
    def fill_histories(self):
        """The reference's history updates (:211-229) from the state the last device call left: one download of dMirror, then its own
        NumPy expressions on X, Y, HMask and gccPHAT.  The TDOA tracking itself already ran on the device (history ring + arg-max,
        csrc/rt.hip); ``tdoaHistory`` receives the index it picked.  No-op when no history object was given."""
        if not self.wants_histories():
            return
        if self._mirror_host is None:
            self._mirror_host = torch.zeros(self.dMirror.shape, dtype=torch.float32).pin_memory()
        self._mirror_host.copy_(self.dMirror, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        m, o, n = self._mirror_host.numpy(), self._mirror_offs, self._mirror_sizes
        self._target_value, self._target_dirty = float(m[o[4]]), False                  # the tracked index came along
        N = self._sources
        self._indexes_host, self._indexes_dirty = m[o[4] + 8:o[4] + 8 + N].copy(), False     # ... and multiple mode's
        multi = self.multiple()
        F, Tc, K, D = self.numFrequencies, self.numTimePerChunk, self.numAtom, self.numTDOAs
        cplx = lambda i: m[o[i]:o[i] + n[i]].reshape(2, F, Tc, 2).copy().view(np.complex64)[..., 0]
        X = cplx(0)
        # multiple mode has N masks and outputs: no coefficient-mask or output-spectrogram mirror there
        if not multi and self.separationEnabled and self.coefficientMaskHistories:
            self.coefficientMaskHistories[self.dictionarySize].set(1 - m[o[2]:o[2] + n[2]].reshape(self.Kp, Tc)[:K])          # :211-212
        if self.inputSpectrogramHistory is not None:
            self.inputSpectrogramHistory.set(-np.mean(np.abs(X), axis=0) ** (1 / 3.0))                                      # :216-217
        if self.gccPHATHistory is not None:
            self.gccPHATHistory.set(m[o[3]:o[3] + n[3]].reshape(D, Tc).copy())                                                 # :218-219
        if self.tdoaHistory is not None:                                                                                       # :220-227
            self.tdoaHistory.set(self._indexes_host.reshape(N, 1).copy() if multi else np.array([[np.float32(m[o[4]])]]))
        if not multi and self.outputSpectrogramHistory is not None:
            Y = cplx(1) if self.separationEnabled else X                                                                      # :213-214
            with np.errstate(invalid='ignore'):
                self.outputSpectrogramHistory.set(-np.nanmean(np.abs(Y), axis=0) ** (1 / 3.0))                                # :228-229

    # ---- device results of the last call, in the reference's shapes --------------------------------------------------
    @_on_device
    def intermediates(self):
        F, K, Tc = self.numFrequencies, self.numAtom, self.numTimePerChunk
        if self.multiple():         # HMask (N, K, Tc) one-hot; tfMask (N, F, Tc) without coefficient inference, (N, 2, F, Tc) with
            HMask, tfMask = self.dHMaskm[:, :K], self.dTfMaskm if self.numHUpdates else self.dTfMaskm[:, 0]
            own = dict(Y=torch.view_as_complex(self.dYm).cpu().numpy(), targetTDOAIndexes=self.targetTDOAIndexes)
        else:                       # HMask (K, Tc); tfMask (F, Tc) without coefficient inference, (2, F, Tc) with
            HMask, tfMask = self.dHMask[:K], self.dTfMask if self.numHUpdates else self.dTfMask.view(-1)[:F * Tc].view(F, -1)
            own = dict(Y=torch.view_as_complex(self.dY).cpu().numpy(), targetTDOAIndex=self.targetTDOAIndex)
        NC = self._sources if self.multiple() else 2          # the spatial filter's state (p0, p1, Re q, Im q) per component and bin
        own['spatialCovariance'] = self.dSpatial[:4 * NC * F].view(NC, F, 4).cpu().numpy()
        return dict(own, X=torch.view_as_complex(self.dX).cpu().numpy(), C=torch.view_as_complex(self.dC).cpu().numpy(),
                    HMask=HMask.cpu().numpy(), argmaxTDOA=self.dArgmax[:K].cpu().numpy(), tfMask=tfMask.cpu().numpy(),
                    Hcoef=self.dHcoef[:K].permute(2, 0, 1).contiguous().cpu().numpy(), gccPHAT=self.dGccPhat.cpu().numpy())


def _check_num_sources(n):
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= MAX_SOURCES:
        raise ValueError('numSources=%r: multiple mode separates 1 to %d sources' % (n, MAX_SOURCES))
    return int(n)


def default_target_indexes(numSources, numTDOAs):
    """Initial targets of multiple mode: spread evenly over the TDOA grid, ascending."""
    return np.array([(i + 1) * numTDOAs // (numSources + 1) for i in range(numSources)], np.float32)


def _check_target_indexes(indexes, numSources, numTDOAs):
    """``numSources`` integer TDOA indexes in [0, numTDOAs) as float32 (the target row's words 8..); ValueError otherwise."""
    try:
        v = np.asarray(indexes, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError('target TDOA indexes must be numbers, got %r' % (indexes,))
    if v.shape != (numSources,):
        raise ValueError('expected %d target TDOA indexes, got %r' % (numSources, indexes))
    if not (np.all(np.isfinite(v)) and np.all(v == np.round(v)) and np.all(v >= 0) and np.all(v < numTDOAs)):
        raise ValueError('target TDOA indexes must be integers in [0, %d), got %r' % (numTDOAs, indexes))
    return v.astype(np.float32)


def _check_stream_shape(processor, hopSize, blockSize, outputDelayBlocks):
    """The block / hop / hand-out checks of a streaming path over ``processor``; returns outputDelayBlocks as an int."""
    # outputDelayBlocks: 2 = the reference's hand-out (utils.py:116); 1 is complete when the synthesis window spans two hops
    if outputDelayBlocks not in (1, 2, 3, 4, 5, 6, 7):
        raise ValueError('outputDelayBlocks must be 1..7')
    outputDelayBlocks = int(outputDelayBlocks)
    # The block handed out is complete only when no later frame adds into it: the synthesis window's non-zero support (first
    # non-zero sample to the end of the frame) must fit in outputDelayBlocks * blockSize + hopSize samples.  2 is the reference's
    # hand-out whatever the window (utils.py:116 -- with its own 512 / 64 low-latency setting it hands out partial sums, and
    # the goldens pin that); any other delay must be complete.
    if outputDelayBlocks != 2:
        nz = np.nonzero(np.asarray(processor.synthesisWindowFunction).reshape(-1))[0]
        support = processor.windowSize - int(nz[0]) if len(nz) else 0
        if support > outputDelayBlocks * int(blockSize) + int(hopSize):
            raise ValueError('outputDelayBlocks=%d hands a block out before it is complete: the synthesis window spans %d samples, '
                             'at most %d fit (use asymmetricWindows, or the reference\'s delay of 2)'
                             % (outputDelayBlocks, support, outputDelayBlocks * int(blockSize) + int(hopSize)))
    if blockSize % hopSize or blockSize // hopSize != processor.numTimePerChunk:
        raise ValueError('blockSize/hopSize must equal the processor\'s numTimePerChunk')
    if 8 * blockSize < processor.windowSize + (processor.numTimePerChunk - 1) * hopSize:
        raise ValueError('blockSize=%d is not supported: the 8-block buffers (utils.py:87-92) must cover one block\'s windows' % blockSize)
    return outputDelayBlocks


class _BlockDriver(object):
    """The host side that ``StreamingGCCNMF`` and ``StreamingGCCNMFBank`` share: page-locked blocks in and out, the block call split in
    two so that the finished block is fetched before the tracking update runs, its fixed front captured once into a HIP graph, and the
    whole-signal loop.  A subclass has ``p``, ``device``, ``blockSize``, ``in_ring`` and ``block_in`` and supplies ``_outputs()`` ->
    (out_ring, block_out) of the current layout (allocating them when it changed), ``_call(block_in, block_out, localize)``,
    ``_state()`` (the tensors a call changes), ``_key()`` (what the captured launches depend on besides buffer contents),
    ``_check_block(block)``, ``_before_block()`` and ``_after_block()``."""

    def __init__(self, use_graph):
        self.use_graph = bool(use_graph)
        self.capture_error = None          # the exception of a failed HIP-graph capture (process_block then launches directly)
        self._pin_in, self._pin_out, self._ev_out = None, None, None      # made by the first process_block
        self._graph, self._graph_key = None, None

    def _check_block(self, block):
        pass

    def _after_block(self):
        pass

    def _before_block(self):
        """Settings that reach the device as buffer contents are written here: in front of every block, never inside a capture."""
        pass

    def process_block(self, block):
        """Host block(s) in -> host block(s) out.  The finished block is fetched (pinned buffer, its own event) BEFORE the tracking update
        of the next block's target has run: that kernel only writes state the next call reads, so it stays off the latency path.
        The fixed launch sequence (upload, kernels, download) is captured once into a HIP graph and replayed per block."""
        block = np.ascontiguousarray(block, dtype=np.float32)
        self._check_block(block)
        with torch.cuda.device(self.device):
            block_out = self._outputs()[1]
            if self._pin_in is None:
                self._pin_in = torch.zeros(self.block_in.shape, dtype=torch.float32).pin_memory()
                self._ev_out = torch.cuda.Event()
            if self._pin_out is None or self._pin_out.shape != block_out.shape:
                self._pin_out = torch.zeros(block_out.shape, dtype=torch.float32).pin_memory()
            self._pin_in.copy_(torch.from_numpy(block))
            self._before_block()
            key = self._key()              # re-capture when one of these changes
            if not self.use_graph:
                self._graph, self._graph_key = None, None
            elif self._graph_key != key:
                self._graph, self._graph_key = self._capture(), key
            if self._graph is not None:
                self._graph.replay()
            else:
                self._launch_front()
            self._ev_out.record()
            self._call(self.block_in, block_out, localize='only')
            self._ev_out.synchronize()
            out = self._pin_out.numpy().copy()
            self._after_block()
        return out

    def _launch_front(self):
        block_out = self._outputs()[1]
        self.block_in.copy_(self._pin_in, non_blocking=True)
        self._call(self.block_in, block_out, localize='skip')
        self._pin_out.copy_(block_out, non_blocking=True)

    def _capture(self):
        """upload -> kernels (all but the tracking update) -> download as one HIP graph: a single serial chain on one stream.  A failed
        capture is not silent: it is kept in ``capture_error`` and warned about once (the direct launches are correct but ~2x the p99
        latency); use_graph=False opts out."""
        try:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            held = self._state()
            saved = [t.clone() for t in held]
            with torch.cuda.graph(g):
                self._launch_front()
            for t, s0 in zip(held, saved):          # capture does not execute on ROCm; restore in case a runtime runs the body once
                t.copy_(s0)
            torch.cuda.synchronize()
            self.capture_error = None
            return g
        except Exception as e:
            import warnings
            if self.capture_error is None:
                warnings.warn('%s: HIP graph capture failed (%s: %s); falling back to direct launches'
                              % (type(self).__name__, type(e).__name__, e), RuntimeWarning)
            self.capture_error = e
            return None

    def _process_signal(self, x):
        """Device signal(s) (..., 2, n) -> host (lead of block_out..., n_blocks * blockSize): every block is one device call."""
        B = self.blockSize
        n_blocks = x.shape[-1] // B
        xb = x[..., :n_blocks * B].reshape(x.shape[:-1] + (n_blocks, B)).movedim(-2, 0).contiguous()      # [block][...][2][B]
        lead = tuple(self._outputs()[1].shape[:-1])
        out = torch.zeros((n_blocks,) + lead + (B,), dtype=torch.float32, device=self.device)
        for b in range(n_blocks):
            self.process_block_device(xb[b], out[b])
        return out.movedim(0, -2).reshape(lead + (n_blocks * B,)).cpu().numpy()


class StreamingGCCNMF(_BlockDriver):
    """``OverlapAddProcessor.processFrames(GCCNMFProcessor.processFrames)`` (utils.py:99-116) as one device call per block:
    ``process_block((2, blockSize)) -> (2, blockSize)``, output delayed by two blocks like the reference.  In multiple mode
    (``processor.targetMode = TARGET_MODE_MULTIPLE``) every target has its own output ring: ``(2, blockSize) -> (numSources, 2,
    blockSize)``; the single-target ring is kept apart, so a stream can switch modes."""

    def __init__(self, processor, hopSize, blockSize, outputDelayBlocks=2, use_graph=True):
        _BlockDriver.__init__(self, use_graph)
        self.outputDelayBlocks = _check_stream_shape(processor, hopSize, blockSize, outputDelayBlocks)
        self.p, self.hopSize, self.blockSize = processor, int(hopSize), int(blockSize)
        dev = self.device = processor.device
        self.in_ring = torch.zeros((2, 8 * blockSize), dtype=torch.float32, device=dev)
        self.out_ring = torch.zeros((2, 8 * blockSize), dtype=torch.float32, device=dev)
        self.block_in = torch.zeros((2, blockSize), dtype=torch.float32, device=dev)
        self.block_out = torch.zeros((2, blockSize), dtype=torch.float32, device=dev)
        self._multi_state = None           # (generation, N, out rings [N][2][8B], block_out [N][2][B]) of multiple mode

    def _outputs(self):
        """(out_ring, block_out) of the processor's current mode."""
        p = self.p
        if not p.multiple():
            return self.out_ring, self.block_out
        key = (p.generation, p._sources)
        if self._multi_state is None or self._multi_state[:2] != key:
            N, B = p._sources, self.blockSize
            z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=p.device)
            self._multi_state = key + (z(N, 2, 8 * B), z(N, 2, B))
        return self._multi_state[2], self._multi_state[3]

    def _call(self, block_in, block_out, localize='with'):
        self.p._call(block_in, block_out, self.in_ring, self._outputs()[0], self.hopSize, self.blockSize, self.outputDelayBlocks,
                     localize=localize)

    def _state(self):
        return self.in_ring, self._outputs()[0], self.p.dHistState, self.p.dHistPos, self.p.dTarget

    def _before_block(self):
        self.p._spatial_on = self.p._apply_spatial()

    def _key(self):
        p = self.p
        return (int(p.targetMode), bool(p.separationEnabled), p._spatial_on, bool(p.localizationEnabled), int(p.localizationWindowSize),
                int(p.numHUpdates), p.dW.data_ptr(), p.dTarget.data_ptr(), p.generation,      # reset() re-allocates every buffer
                p._sources if p.multiple() else 0, self._outputs()[0].data_ptr(), self._pin_out.data_ptr())

    def _after_block(self):
        self.p.fill_histories()            # host mirrors (only when history objects were given): after the tracking update

    def process_block_device(self, block_in, block_out):
        """Device tensors in/out, asynchronous on the current stream (what a capture/playback loop would call); block_out is
        [numSources][2][blockSize] in multiple mode."""
        self._before_block()
        self._call(block_in, block_out)

    def process_stream(self, stereoSamples):
        """(2, n) -> (2, n_blocks*blockSize) (multiple mode: (numSources, 2, n_blocks*blockSize)); the whole signal is uploaded once,
        every block is one device call."""
        return self._process_signal(torch.from_numpy(np.ascontiguousarray(stereoSamples, dtype=np.float32)).to(self.device))


class StreamingGCCNMFBank(_BlockDriver):
    """S independent real-time streams of one configuration, advanced together: one device call per block runs all of them
    (the ``streams`` layout of ``_hip.rt_process_block``).  Stream s produces bit for bit what a ``StreamingGCCNMF`` over its own
    ``GCCNMFProcessor`` of the same configuration produces when fed the same blocks.

    ``processor`` is the shared configuration: its dictionary, TDOA grid, windows, twiddles, ``targetMode``, ``numHUpdates`` and
    ``localizationWindowSize``, and its ``separationEnabled`` / ``localizationEnabled`` as master switches.  The bank allocates its
    own per-stream state (rings, spectra, masks, history ring, target row) and never touches the processor's.  Each stream has a
    target row {index, epsilon, beta, noiseFloor, separation, localisation, nlAlpha, spatialFilterFrames}: a stream separates (localises) when the processor's
    switch and its own are both on, and localises on GCC-NONLIN when its nlAlpha word is > 0 (``setGCCPHATNL``), and runs the online spatial filter behind its mask when its last word holds a time constant (``setSpatialFilter``).  After ``processor.reset()`` the next call re-allocates all per-stream state.

    The GUI's host mirrors (``GCCNMFProcessor.fill_histories``) are not produced for a bank.

    Multiple mode (the processor's ``targetMode = TARGET_MODE_MULTIPLE``, N = its ``numSources`` for every stream): target rows are 16
    words, words 8..8+N-1 the stream's target indexes (``setTargetTDOAIndexes(s, indexes)``; initially the processor's), and
    ``process_block`` returns (S, N, 2, blockSize).  Switching the processor into or out of multiple mode starts every stream over."""

    def __init__(self, processor, numStreams, hopSize, blockSize, outputDelayBlocks=2, use_graph=True):
        if int(numStreams) != numStreams or not 1 <= int(numStreams) <= MAX_BANK_STREAMS:
            raise ValueError('numStreams=%r: a bank holds 1 to %d streams' % (numStreams, MAX_BANK_STREAMS))
        _BlockDriver.__init__(self, use_graph)
        self.outputDelayBlocks = _check_stream_shape(processor, hopSize, blockSize, outputDelayBlocks)
        self.p, self.numStreams, self.hopSize, self.blockSize = processor, int(numStreams), int(hopSize), int(blockSize)
        self.device = processor.device
        self._generation = None
        self._alloc()

    # ---- per-stream state ----------------------------------------------------------------------------------------------
    def _initial_row(self):
        row = np.concatenate([self.p._target_host, np.array([1, 1, self.p._nl_word, self.p._spatial_word()], np.float32)]).astype(np.float32)
        if self._multi:                    # + the processor's target indexes (words 8..)
            tau = np.zeros(8, np.float32)
            tau[:self._sources] = self.p.targetTDOAIndexes
            row = np.concatenate([row, tau])
        return row

    def _layout(self):
        return (self.p.generation, self.p._sources) if self.p.multiple() else (self.p.generation, 0)

    @_on_device
    def _alloc(self):
        p, S, B = self.p, self.numStreams, self.blockSize
        F, Tc, D, Kp = p.numFrequencies, p.numTimePerChunk, p.numTDOAs, p.Kp
        self._layout_key = self._layout()
        self._multi, self._sources = self._layout_key[1] > 0, max(self._layout_key[1], 1)
        N = self._sources if self._multi else 1           # outputs per stream; the mask images carry N targets
        lead = (S, N) if self._multi else (S,)
        z = lambda *shape, **kw: torch.zeros(shape, dtype=kw.get('dtype', torch.float32), device=self.device)
        self.in_ring, self.out_ring = z(S, 2, 8 * B), z(*lead, 2, 8 * B)
        self.block_in, self.block_out = z(S, 2, B), z(*lead, 2, B)
        self.dX, self.dY, self.dC = z(S, 2, F, Tc, 2), z(*lead, 2, F, Tc, 2), z(S, F, Tc, 2)
        self.dHMask, self.dArgmax = z(*lead, Kp, Tc), z(S, Kp, Tc, dtype=torch.int32)
        self.dTfMask, self.dGccPhat = z(*lead, 2, F, Tc), z(S, D, Tc)
        self.dHist, self.dHistPos = z(S, D, p.numTDOAHistory), z(S, dtype=torch.int32)
        self.dHcoef, self.dRv = None, None     # coefficient-inference scratch: allocated with the first call that needs it
        self.dHistState, self.dSpatial = self.dHist, None      # the spatial filter's covariances behind the histories: likewise
        self._row0 = self._initial_row()
        self._spatial_rows = np.full(S, self._row0[7], np.float32)      # host copy of word 7 of every row
        self.dTarget = torch.from_numpy(np.tile(self._row0, (S, 1))).to(self.device)
        self._targets = self._row0[0].repeat(S).astype(np.float32)      # host copy of the tracked indexes
        self._tindexes = np.tile(self._row0[8:8 + self._sources], (S, 1)) if self._multi else None    # multiple mode's, (S, N)
        self._targets_dirty, self._targets_pin = False, None
        self._generation = p.generation
        self._graph, self._graph_key = None, None

    def _ensure_state(self):
        if self._layout_key != self._layout():              # processor reset() (every table re-allocated) or a mode change
            self._alloc()
        if self.p.numHUpdates and self.dHcoef is None:
            S, F, Tc, Kp = self.numStreams, self.p.numFrequencies, self.p.numTimePerChunk, self.p.Kp
            self.dHcoef = torch.zeros((S, Kp, Tc, 2), dtype=torch.float32, device=self.device)
            self.dRv = torch.zeros((S, F, Tc, 2), dtype=torch.float32, device=self.device)
        if self._spatial_call() and self.dSpatial is None:
            # the block call finds the covariances [S][NC][F][4] behind the S history images: one buffer, the histories carried over
            S, F, D, Lh = self.numStreams, self.p.numFrequencies, self.p.numTDOAs, self.p.numTDOAHistory
            NC = self._sources if self._multi else 2
            at = _hip.rt_spatial_state_offset(D, Lh, S)
            both = torch.zeros(at + _hip.rt_spatial_state_floats(F, NC, S), dtype=torch.float32, device=self.device)
            both[:S * D * Lh].copy_(self.dHist.reshape(-1))
            self.dHistState, self.dHist, self.dSpatial = both, both[:S * D * Lh].view(S, D, Lh), both[at:].view(S, NC, F, 4)

    def _spatial_call(self):
        """The call-level switch of the spatial filter: some stream's row word 7 holds a time constant."""
        return bool((self._spatial_rows > 0).any())

    def _stream_index(self, s):
        if int(s) != s or not 0 <= int(s) < self.numStreams:
            raise IndexError('stream %r of a bank of %d' % (s, self.numStreams))
        return int(s)

    # ---- per-stream control (none of these re-captures the graph: they only write the target rows) ------------------------
    @_on_device
    def setTargetTDOARange(self, s, targetTDOAIndex, targetTDOAEpsilon, targetTDOABeta, targetTDOANoiseFloor):
        """Words 0-3 of stream s's target row (``GCCNMFProcessor.setTargetTDOARange`` for one stream)."""
        s = self._stream_index(s)
        self._ensure_state()
        v = np.array([targetTDOAIndex, targetTDOAEpsilon, targetTDOABeta, targetTDOANoiseFloor], np.float32)
        self.dTarget[s, :4].copy_(torch.from_numpy(v))
        self._targets[s] = v[0]

    @_on_device
    def setSeparationEnabled(self, s, on):
        """Word 4 of stream s's row: off = the stream is passed through (synthesised from its unmasked spectrum)."""
        s = self._stream_index(s)
        self._ensure_state()
        self.dTarget[s, 4] = float(bool(on))

    @_on_device
    def setLocalizationEnabled(self, s, on):
        """Word 5 of stream s's row: off = the history still fills, the tracked index stays where it is."""
        s = self._stream_index(s)
        self._ensure_state()
        self.dTarget[s, 5] = float(bool(on))

    @_on_device
    def setGCCPHATNL(self, s, enabled, alpha=2.0):
        """Word 6 of stream s's row: GCC-NONLIN localisation for this stream alone (``gccPHATNLEnabled`` / ``gccPHATNLAlpha``; initially
        the processor's, as of its last ``reset()``).  Takes effect with the next block; the stream's gccPHAT history is kept, so reset
        the stream as well where PHAT and NONLIN columns must not share a window mean."""
        s = self._stream_index(s)
        on, a = _hip.check_gcc_phat_nl(enabled, alpha)
        self._ensure_state()
        self.dTarget[s, 6] = a if on else 0.0

    @_on_device
    def setSpatialFilter(self, s, enabled, frames=None):
        """Word 7 of stream s's row: the online spatial filter for this stream alone (``spatialFilterEnabled`` / ``spatialFilterFrames``;
        initially the processor's).  frames: the time constant of its covariances, None = the processor's ``spatialFilterFrames``.  Takes
        effect with the next block and keeps the stream's covariances (``reset_stream`` clears them).  Switching the first stream on (or
        the last one off) changes the call itself, so a captured graph is taken again; every other toggle only writes the row."""
        s = self._stream_index(s)
        on, tau = _hip.check_spatial_filter(enabled, self.p.spatialFilterFrames if frames is None else frames)
        self._ensure_state()
        self._spatial_rows[s] = tau if on else 0.0
        self._ensure_state()
        self.dTarget[s, 7] = float(self._spatial_rows[s])

    @_on_device
    def setTargetTDOAIndexes(self, s, indexes):
        """Multiple mode: words 8.. of stream s's row (``GCCNMFProcessor.setTargetTDOAIndexes`` for one stream)."""
        s = self._stream_index(s)
        self._ensure_state()
        if not self._multi:
            raise ValueError('setTargetTDOAIndexes needs the processor in TARGET_MODE_MULTIPLE')
        v = _check_target_indexes(indexes, self._sources, self.p.numTDOAs)
        self.dTarget[s, 8:8 + self._sources].copy_(torch.from_numpy(v))
        self._tindexes[s] = v

    @_on_device
    def reset_stream(self, s):
        """Stream s starts over (a session left, a new one takes its slot): its rings (all N output rings in multiple mode), history,
        history position and target row (the processor's target or target indexes, both switches on) are reset; no other stream is
        touched."""
        s = self._stream_index(s)
        self._ensure_state()
        for t in (self.in_ring, self.out_ring, self.dHist, self.dHistPos) + (() if self.dSpatial is None else (self.dSpatial,)):
            t[s].zero_()
        row = self._initial_row()
        self._spatial_rows[s] = row[7]
        self._ensure_state()
        self.dTarget[s].copy_(torch.from_numpy(row))
        self._targets[s] = row[0]
        if self._multi:
            self._tindexes[s] = row[8:8 + self._sources]

    @property
    def targetTDOAIndexes(self):
        """(S,) tracked target TDOA indexes ((S, numSources) in multiple mode), cached like ``GCCNMFProcessor.targetTDOAIndex``:
        fetched (one small download of the target rows) only when a call ran with the localisation on since they were last known
        on the host."""
        if self._targets_dirty:
            with torch.cuda.device(self.device):
                if self._targets_pin is None or self._targets_pin.shape != self.dTarget.shape:
                    self._targets_pin = torch.zeros(self.dTarget.shape, dtype=torch.float32).pin_memory()
                self._targets_pin.copy_(self.dTarget, non_blocking=True)
                torch.cuda.current_stream(self.device).synchronize()
            self._targets = self._targets_pin.numpy()[:, 0].copy()
            if self._multi:
                self._tindexes = self._targets_pin.numpy()[:, 8:8 + self._sources].copy()
            self._targets_dirty = False
        return (self._tindexes if self._multi else self._targets).copy()

    # ---- device calls -----------------------------------------------------------------------------------------------------
    def _outputs(self):
        self._ensure_state()
        return self.out_ring, self.block_out

    @_on_device
    def _call(self, block_in, block_out, localize='with'):
        p = self.p
        if p.localizationEnabled and localize != 'skip':
            self._targets_dirty = True
        _hip.rt_process_block(block_in, block_out, self.in_ring, self.out_ring, self.dX, self.dY, self.dC, self.dHMask, self.dArgmax,
                              self.dTfMask, self.dHist, self.dHistPos, self.dTarget, self.dGccPhat, *p._tables(), self.dHcoef, self.dRv,
                              *p._settings(self.hopSize, self.blockSize), p.numHUpdates, self.outputDelayBlocks, localize=localize,
                              streams=self.numStreams, targets=self._sources if self._multi else None,
                              spatial=self._spatial_call() and bool(p.separationEnabled))

    def _state(self):
        return self.in_ring, self.out_ring, self.dHistState, self.dHistPos, self.dTarget

    def _key(self):
        p = self.p
        return (int(p.targetMode), bool(p.separationEnabled), bool(p.localizationEnabled), int(p.localizationWindowSize),
                int(p.numHUpdates), p.dW.data_ptr(), self.dTarget.data_ptr(), p.generation, self._layout_key, self._pin_out.data_ptr(),
                self._spatial_call(), self.dHist.data_ptr())

    def _check_block(self, blocks):
        if blocks.shape != (self.numStreams, 2, self.blockSize):
            raise ValueError('expected blocks of shape %s, got %s' % ((self.numStreams, 2, self.blockSize), blocks.shape))

    def _check_blocks(self, t, shape):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('expected a contiguous float32 tensor of shape %s' % (shape,))

    def process_block_device(self, block_in, block_out):
        """(S, 2, blockSize) device tensors in, (S, 2, blockSize) ((S, N, 2, blockSize) in multiple mode) out, asynchronous on the
        current stream."""
        self._check_blocks(block_in, (self.numStreams, 2, self.blockSize))
        self._check_blocks(block_out, tuple(self._outputs()[1].shape))
        self._call(block_in, block_out)

    def process_streams(self, x):
        """(S, 2, n) -> (S, 2, n_blocks * blockSize) ((S, N, 2, ...) in multiple mode); the whole signal is uploaded once, every block
        is one device call."""
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
        if x.dim() != 3 or x.shape[0] != self.numStreams or x.shape[1] != 2:
            raise ValueError('expected signals of shape (%d, 2, n)' % self.numStreams)
        return self._process_signal(x)
