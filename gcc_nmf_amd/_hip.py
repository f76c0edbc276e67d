"""ctypes binding of libgccnmf_hip.so (include/gccnmf_hip.h).

The library is the product: there is NO CPU fallback.  If the shared object is
missing (or its symbols do not match the header) importing this module's
``lib()`` raises ``HipLibraryError`` -- loudly, on every call path.

Below ``lib()`` is the stage layer: one plain function per product stage, the ONLY place in the package that builds the mode words
of the C ABI (modes are keywords here; pointers are tensors, None or raw addresses; the stream defaults to torch's current one).
"""
import ctypes
import math
import numbers
import os
import warnings

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('GCCNMF_HIP_LIB') or os.path.join(_HERE, 'libgccnmf_hip.so')     # override: A/B builds only

c_int, c_long, c_float, c_void_p = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
P_INT = ctypes.POINTER(ctypes.c_int)


class SharedShard(ctypes.Structure):
    """gccnmf_shared_shard (include/gccnmf_hip.h)"""
    _fields_ = [('V', c_void_p), ('H', c_void_p), ('workspace', c_void_p), ('N', c_int), ('batch', c_int), ('ld', c_int)]


class DirectGemm(ctypes.Structure):
    """gccnmf_direct_gemm (include/gccnmf_hip.h): descriptor of one latency-path GEMM (csrc/direct.hip)"""
    _fields_ = [('A', c_void_p), ('B', c_void_p), ('sA', c_long), ('sB', c_long), ('lda', c_int), ('ldb', c_int),
                ('M', c_int), ('N', c_int), ('Kd', c_int), ('batch', c_int),
                ('bscale', c_void_p), ('s_bscale', c_long), ('tailA', c_void_p), ('s_tailA', c_long), ('tail_row', c_int),
                ('rowsumB', c_void_p), ('s_rowsumB', c_long), ('C', c_void_p), ('sC', c_long), ('ldc', c_int),
                ('Ct', c_void_p), ('sCt', c_long), ('ldct', c_int), ('E0', c_void_p), ('sE0', c_long), ('lde0', c_int),
                ('E1', c_void_p), ('sE1', c_long), ('E2', c_void_p), ('sE2', c_long), ('ktailA', c_void_p), ('ktailB', c_void_p),
                ('s_ktailA', c_long), ('s_ktailB', c_long), ('alpha', c_float), ('eps', c_float),
                ('tiles_m', c_int), ('tiles_n', c_int), ('xc', c_int), ('sm', c_int), ('sn', c_int), ('trace', c_void_p)]


# gccnmf_allreduce_fn: int (*)(void* ctx, float* buf, long count, void* stream)
RCCL_UNIQUE_ID_BYTES = 128
ALLREDUCE_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_long, c_void_p)

STATUS = {0: 'GCCNMF_OK', 1: 'GCCNMF_ERR_ARG (bad argument)', 2: 'GCCNMF_ERR_LAUNCH (HIP launch failed)',
          3: 'GCCNMF_ERR_UNSUPPORTED', 4: 'GCCNMF_ERR_COLLECTIVE (all-reduce hook / RCCL failed)'}

# name -> (restype, argtypes); mirrors include/gccnmf_hip.h declaration by declaration
SIGNATURES = {
    'gccnmf_version': (c_int, []),
    'gccnmf_set_tuning': (c_int, [c_int, c_int]),
    'gccnmf_pitches': (c_int, [c_int, c_int, c_int, P_INT, P_INT, P_INT, P_INT]),
    'gccnmf_stft_stereo': (c_int, [c_void_p, c_long, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    'gccnmf_dft_workspace_floats': (c_long, [c_int, c_int, c_int]),
    'gccnmf_stft_dft': (c_int, [c_void_p, c_long, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'gccnmf_istft_dft': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p]),
    'gccnmf_stft_stereo_pcm16': (c_int, [c_void_p, c_long, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p]),
    'gccnmf_pack_pcm16': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'gccnmf_klnmf_workspace_floats': (c_long, [c_int, c_int, c_int, c_int]),
    'gccnmf_klnmf': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                             c_float, c_int, c_void_p]),
    'gccnmf_klnmf_ragged_workspace_floats': (c_long, [c_int, c_int, c_int, c_int]),
    'gccnmf_klnmf_ragged': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, P_INT, c_int, c_int, c_int, c_int, c_float,
                                    c_float, c_int, c_void_p]),
    'gccnmf_klnmf_chain_status': (c_int, [c_void_p, c_int, c_int, c_int, c_int, P_INT]),
    'gccnmf_klnmf_plan': (c_int, [c_int, c_int, c_int, c_int, c_int]),
    'gccnmf_klnmf_stage': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float,
                                   c_int, c_int, c_void_p]),
    'gccnmf_klnmf_shared_workspace_floats': (c_long, [c_int, c_int, c_int, c_int]),
    'gccnmf_klnmf_shared_partial_floats': (c_long, [c_int, c_int]),
    'gccnmf_klnmf_shared_begin': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'gccnmf_klnmf_shared_step_a': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                           c_int, c_float, c_float, c_void_p]),
    'gccnmf_klnmf_shared_step_b': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'gccnmf_klnmf_shared_finish': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'gccnmf_klnmf_shared_shard_workspace_floats': (c_long, [c_int, c_int, c_int, c_int, c_int]),
    'gccnmf_klnmf_shared_run': (c_int, [ctypes.POINTER(SharedShard), c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float,
                                        c_float, c_void_p, c_void_p, c_void_p]),
    'gccnmf_rccl_available': (c_int, []),
    'gccnmf_rccl_unique_id': (c_int, [ctypes.c_char_p]),
    'gccnmf_rccl_comm_init': (c_int, [ctypes.c_char_p, c_int, c_int, ctypes.POINTER(c_void_p)]),
    'gccnmf_rccl_comm_destroy': (c_int, [c_void_p]),
    'gccnmf_rccl_allreduce': (c_int, [c_void_p, c_void_p, c_long, c_void_p]),
    'gccnmf_rccl_allreduce_hook': (c_void_p, []),
    'gccnmf_angular_spectrogram': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                           c_void_p]),
    'gccnmf_pick_tdoa_peaks': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'gccnmf_scores_workspace_floats': (c_long, [c_int, c_int, c_int, c_int]),
    'gccnmf_target_scores_masks': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                           c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'gccnmf_argmax_targets': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'gccnmf_coherence': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'gccnmf_magnitude': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'gccnmf_reconstruct_workspace_floats': (c_long, [c_int, c_int, c_int, c_int]),
    'gccnmf_reconstruct': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'gccnmf_istft_ola': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_int,
                                 c_void_p, c_void_p, c_void_p]),
    'gccnmf_ola_frames_halo': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    'gccnmf_rt_process_block': (c_int, [c_void_p] * 19 + [c_int] * 13 + [c_void_p]),
    'gccnmf_rt_process_block_ll': (c_int, [c_void_p] * 23 + [c_int] * 15 + [c_void_p]),
    'gccnmf_gemm_direct': (c_int, [ctypes.POINTER(DirectGemm), c_int, c_int, c_void_p]),
    'gccnmf_debug_gemm_plan': (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, P_INT, P_INT, c_int]),
    'gccnmf_debug_gemm': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                  c_int, c_int, c_long, c_long, c_long, c_void_p, c_void_p, c_void_p]),
}


# entry points of the lab build only (make -C gcc_nmf_amd/csrc EXPERIMENTS=1 -> libgccnmf_hip_exp.so; `#ifdef GCCNMF_EXPERIMENTS` in the header)
EXPERIMENT_SIGNATURES = {
    'gccnmf_debug_set_trace': (c_int, [c_void_p, c_int]),
    'gccnmf_debug_mfma_peak': (c_int, [c_void_p, c_int, c_int, c_void_p]),
}


class HipLibraryError(RuntimeError):
    pass


def check_gcc_phat_nl(gccPHATNLEnabled, gccPHATNLAlpha):
    """The reference's two GCC-NONLIN settings (gccNMF/realtime/config.py:42-43) as the engines, the named functions and the real-time
    processor take them; no device needed.  Returns (enabled, alpha): alpha a finite number > 0 that is a normal float32, ValueError
    otherwise (checked whether or not the setting is enabled, so a bad value cannot wait for the switch)."""
    a = gccPHATNLAlpha
    if isinstance(a, bool) or not isinstance(a, numbers.Real) or not math.isfinite(a) or not a > 0:
        raise ValueError('gccPHATNLAlpha must be a finite number > 0, got %r' % (a,))
    a32 = ctypes.c_float(float(a)).value
    if not 1.17549435e-38 <= a32 < float('inf'):
        raise ValueError('gccPHATNLAlpha=%r is not a normal float32' % (a,))
    return bool(gccPHATNLEnabled), float(a32)


def check_convergence(tolerance, checkEvery, numIterations):
    """The ``tolerance`` / ``checkEvery`` keywords of the engines, inferKLNMFCoefficients and performKLNMFUntilConverged, and the
    iteration count they cap; no device needed.  ``tolerance``: None (a fixed number of iterations) or a finite float with
    0 < tolerance < 1, the relative decrease of the KL divergence per check below which a file stops.  ``checkEvery``: iterations between
    two checks, an integer >= 1 (checked whether or not a tolerance is given, so a bad value cannot wait for the switch).
    ``numIterations``: with a tolerance the maximum, an integer >= 0; without one it is the fixed count and is taken as
    ``int(numIterations)``, as it always was.  Returns (tolerance or None, checkEvery, numIterations)."""
    if tolerance is not None:
        if isinstance(tolerance, bool) or not isinstance(tolerance, numbers.Real) or not math.isfinite(tolerance) or not 0 < tolerance < 1:
            raise ValueError('tolerance must be None or a finite number with 0 < tolerance < 1, got %r' % (tolerance,))
        tolerance = float(tolerance)
    if isinstance(checkEvery, bool) or not isinstance(checkEvery, numbers.Integral) or checkEvery < 1:
        raise ValueError('checkEvery must be a whole number of iterations >= 1, got %r' % (checkEvery,))
    if tolerance is None:
        return None, int(checkEvery), int(numIterations)
    if isinstance(numIterations, bool) or not isinstance(numIterations, numbers.Integral) or numIterations < 0:
        raise ValueError('the number of iterations must be a whole number >= 0, got %r' % (numIterations,))
    return tolerance, int(checkEvery), int(numIterations)


def check_tdoa_tracking(tdoaTracking, localizationWindowSize, numSources):
    """The ``tdoaTracking`` / ``localizationWindowSize`` keywords of the engines and the window argument of
    estimateTargetTDOATracksFromAngularSpectrogram; no device needed.  The window is a number of frames: an integer >= 1 (checked
    whether or not tracking is on, so a bad value cannot wait for the switch), required when tracking is on; tracking also needs
    the number of sources (the peak rule keeps that many peaks per frame, 1 to 255).  Returns (tracking, window or None)."""
    L = localizationWindowSize
    if L is not None:
        if isinstance(L, bool) or not isinstance(L, numbers.Integral) or L < 1:
            raise ValueError('localizationWindowSize must be a whole number of frames >= 1, got %r' % (L,))
        L = int(L)
    if tdoaTracking:
        if L is None:
            raise ValueError('tdoaTracking needs localizationWindowSize (frames)')
        S = numSources
        if S is None or isinstance(S, bool) or not isinstance(S, numbers.Integral) or not 1 <= S <= 255:
            raise ValueError('tdoaTracking needs the number of sources (1 to 255), got %r' % (S,))
    return bool(tdoaTracking), L


def load_library(path, signatures, optional=(), lenient=False):
    """``ctypes.CDLL(path)`` with typed prototypes: ``signatures`` and ``optional`` map name -> (restype, argtypes).  HipLibraryError if the
    file is missing, does not load or lacks a name of ``signatures`` (``lenient``: such a name is skipped and stays uncallable); names of
    ``optional`` are typed where the library has them.  The one loader of the five binding modules."""
    if not os.path.exists(path):
        raise HipLibraryError(
            '%s is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` or '
            '`make -C gcc_nmf_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.' % path)
    try:
        handle = ctypes.CDLL(path)
    except OSError as e:
        raise HipLibraryError('cannot load %s: %s' % (path, e))
    for table, required in ((signatures, not lenient), (dict(optional), False)):
        for name, (restype, argtypes) in table.items():
            fn = getattr(handle, name, None)
            if fn is None:
                if required:
                    raise HipLibraryError('%s does not export %s (stale build? re-run make -C gcc_nmf_amd/csrc)' % (path, name))
                continue
            fn.restype = restype
            fn.argtypes = argtypes
    return handle


def require_device(lib_fn, what):
    """HipLibraryError unless ``lib_fn()`` loads its library and a ROCm device is visible; ``what`` names the kernels in the message."""
    lib_fn()
    if not torch.cuda.is_available():
        raise HipLibraryError('no ROCm device visible: %s no CPU fallback' % what)


_lib = None


def lib():
    """The loaded shared library with typed prototypes; raises HipLibraryError if it cannot be used."""
    global _lib
    if _lib is not None:
        return _lib
    # GCCNMF_HIP_LIB names an A/B build of another revision: entry points it lacks are simply not callable
    handle = load_library(LIB_PATH, SIGNATURES, optional=EXPERIMENT_SIGNATURES, lenient=bool(os.environ.get('GCCNMF_HIP_LIB')))
    # A/B runs without code changes: GCCNMF_TUNE="9=2,8=1" applies gccnmf_set_tuning(key, value) pairs at load time
    for kv in filter(None, os.environ.get('GCCNMF_TUNE', '').split(',')):
        key, value = [int(v) for v in kv.split('=')]
        if handle.gccnmf_set_tuning(key, value) != 0:
            # a rejected pair would silently measure the defaults (a product build rejects the experiment-only keys): always loud.
            # GCCNMF_TUNE_LENIENT=1 (one tuning string across libraries of different revisions) downgrades it to a warning.
            msg = 'GCCNMF_TUNE: gccnmf_set_tuning(%d, %d) was rejected by %s' % (key, value, LIB_PATH)
            if os.environ.get('GCCNMF_TUNE_LENIENT', '') in ('', '0'):
                raise HipLibraryError(msg)
            warnings.warn(msg + ' -- running with that key at its default')
    _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        raise HipLibraryError('%s failed: %s' % (what, STATUS.get(status, 'status %d' % status)))


# ---- the stage layer ---------------------------------------------------------------------------------------------------------
def _ptr(t):
    """A pointer argument of the ABI: a tensor's address, a raw integer address as it is, None = null."""
    return 0 if t is None else t if isinstance(t, int) else t.data_ptr()


def _stream(device=None):
    """Raw hipStream_t of torch's current stream on `device` (default: the current device)."""
    return torch.cuda.current_stream(device).cuda_stream


def _stage(name, *args, stream=None, what=None):
    """One stage call: the arguments in the header's order (pointers, by the prototype, through ``_ptr``), the stream last, the
    status checked under the entry point's name (or ``what``)."""
    args = [_ptr(a) if t is c_void_p else a for a, t in zip(args, SIGNATURES[name][1])]
    check(getattr(lib(), name)(*args, _stream() if stream is None else stream), what or name)


def stft_stereo(x, n, n_fft, hop, T, batch, window, twiddle, X, V, CC, pcm16=False, stream=None):
    """x: [batch][2][n] float32 samples, or with pcm16 [batch][n][2] int16 interleaved frames (contiguous files either way)."""
    name, stride = ('gccnmf_stft_stereo_pcm16', n) if pcm16 else ('gccnmf_stft_stereo', 2 * n)
    _stage(name, x, stride, n, n_fft, hop, T, batch, window, twiddle, X, V, CC, stream=stream)


def istft_ola(spec, nsig, n_fft, hop, T, batch, window, twiddle, gain, center, frames, y, stream=None):
    """frames: None = the fused inverse transform + overlap-add where the library has one, else the scratch of the two-kernel form."""
    _stage('gccnmf_istft_ola', spec, nsig, n_fft, hop, T, batch, window, twiddle, gain, 1 if center else 0, frames, y, stream=stream)


def ola_frames_halo(previous, halo, frames, nsig, n_fft, hop, T, first, L, gain, y, stream=None):
    _stage('gccnmf_ola_frames_halo', previous, halo, frames, nsig, n_fft, hop, T, first, L, gain, y, stream=stream)


def pack_pcm16(y, nsig, L, peak, out, stream=None):
    _stage('gccnmf_pack_pcm16', y, nsig, L, peak, out, stream=stream)


def coherence(X, F, T, batch, CC, stream=None):
    _stage('gccnmf_coherence', X, F, T, batch, CC, stream=stream)


def magnitude(X, F, T, batch, V, stream=None):
    _stage('gccnmf_magnitude', X, F, T, batch, V, stream=stream)


GCCNMF_FLAG_FIXED_W = 1 << 16           # include/gccnmf_hip.h: W is one shared [Fp][Kp] dictionary and is never updated
GCCNMF_FLAG_H_ONES = 1 << 17            # include/gccnmf_hip.h: H starts as all ones (output only)
GCCNMF_STAGE_DIVERGENCE = 7             # include/gccnmf_hip.h: gccnmf_klnmf_stage, "KL divergence of the current factors"


FREE_ATOMS_MAX = 128                    # include/gccnmf_hip.h: the most free atoms of a semi-supervised call
SEMI_MAX_ATOMS, SEMI_MAX_BINS = 1024, 2049


def GCCNMF_FLAG_FREE_ATOMS(n):
    """include/gccnmf_hip.h: the last n atoms of every file's W are learned beside the dictionary in front of them (bits 18-25)."""
    return int(n) << 18


def check_free_atoms(numFreeAtoms, K_fixed, F=None):
    """The argument rules of the semi-supervised call (GCCNMF_FLAG_FREE_ATOMS in include/gccnmf_hip.h) for ``numFreeAtoms`` free atoms
    behind a dictionary of ``K_fixed`` atoms (and, if given, F bins); no device needed.  Returns the count as an int; 0 = not
    semi-supervised.  ValueError otherwise: not a whole number in [0, 128], no dictionary in front of the free atoms, a dictionary whose
    size is no multiple of 16 (the free block starts on an atom-group boundary), more than 1024 atoms in all, more than 2049 bins."""
    n = numFreeAtoms
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 0 <= n <= FREE_ATOMS_MAX:
        raise ValueError('numFreeAtoms must be a whole number from 0 to %d, got %r' % (FREE_ATOMS_MAX, n))
    n = int(n)
    if n == 0:
        return 0
    if isinstance(K_fixed, bool) or not isinstance(K_fixed, numbers.Integral) or K_fixed < 1:
        raise ValueError('free atoms need a dictionary of at least one atom in front of them, got %r' % (K_fixed,))
    if K_fixed % 16:
        raise ValueError('free atoms take a dictionary whose size is a multiple of 16, got %d atoms' % K_fixed)
    if K_fixed + n > SEMI_MAX_ATOMS:
        raise ValueError('dictionary and free atoms together may have at most %d atoms, got %d + %d' % (SEMI_MAX_ATOMS, K_fixed, n))
    if F is not None and not 2 <= F <= SEMI_MAX_BINS:
        raise ValueError('the semi-supervised call takes 2 to %d bins, got %r' % (SEMI_MAX_BINS, F))
    return n


DIVERGENCES = ('kl', 'is', 'euclidean')        # beta = 1, 0, 2
GCCNMF_FLAG_DIVERGENCE_IS = 1 << 26            # include/gccnmf_hip.h: Itakura-Saito NMF (bits 26-27 of the flags of gccnmf_klnmf / _stage / _plan)
GCCNMF_FLAG_DIVERGENCE_EUCLIDEAN = 2 << 26     # include/gccnmf_hip.h: Euclidean NMF
DIVERGENCE_FLAGS = {'kl': 0, 'is': GCCNMF_FLAG_DIVERGENCE_IS, 'euclidean': GCCNMF_FLAG_DIVERGENCE_EUCLIDEAN}
DIVERGENCE_MAX_ATOMS, DIVERGENCE_MAX_BINS = 1024, 2049      # the envelope of the IS / Euclidean call
_BETA_NAMES = {0: 'is', 1: 'kl', 2: 'euclidean'}


def check_divergence(divergence, F=None, K=None):
    """The ``divergence`` keyword of the engines, klnmf, klnmf_stage and klnmf_divergence, and the ``beta`` of performBetaNMF /
    getBetaDivergence; no device needed.  Takes 'kl', 'is' or 'euclidean', or beta = 1, 0 or 2 (a whole number, not a bool), and returns
    the name; ValueError otherwise -- a real-valued beta is not available -- and, for 'is' / 'euclidean' with F or K given, outside
    2 <= F <= 2049, 1 <= K <= 1024."""
    d = divergence
    if isinstance(d, str):
        if d not in DIVERGENCES:
            raise ValueError("divergence must be 'kl', 'is' or 'euclidean' (or beta = 1, 0, 2), got %r" % (d,))
    elif isinstance(d, bool) or not isinstance(d, numbers.Real) or d not in _BETA_NAMES:
        raise ValueError("divergence must be 'kl', 'is' or 'euclidean' (or beta = 1, 0, 2), got %r" % (d,))
    else:
        d = _BETA_NAMES[int(d)]
    if d != 'kl':
        if F is not None and not 2 <= F <= DIVERGENCE_MAX_BINS:
            raise ValueError('the %s iteration takes 2 to %d bins, got %r' % (d, DIVERGENCE_MAX_BINS, F))
        if K is not None and not 1 <= K <= DIVERGENCE_MAX_ATOMS:
            raise ValueError('the %s iteration takes 1 to %d atoms, got %r' % (d, DIVERGENCE_MAX_ATOMS, K))
    return d


def klnmf_divergence_extra_floats(Fp, Kp, Np, batch):
    """GCCNMF_KLNMF_DIVERGENCE_WORKSPACE_FLOATS(Fp, Kp, Np, batch) of include/gccnmf_hip.h: the floats an IS / Euclidean call needs behind
    the KL layout -- Q [batch][Fp][Np] | Ud [batch][Fp][Kp]."""
    return batch * Fp * (Np + Kp)


def klnmf_divergence_workspace_floats(F, N, K, batch, divergence='kl'):
    """Floats of the workspace of gccnmf_klnmf / gccnmf_klnmf_stage for this divergence: gccnmf_klnmf_workspace_floats, for 'is' and
    'euclidean' followed by the extra blocks above."""
    n = lib().gccnmf_klnmf_workspace_floats(F, N, K, batch)
    if check_divergence(divergence) == 'kl' or n < 0:
        return n
    return n + klnmf_divergence_extra_floats(-(-F // 16) * 16, -(-K // 64) * 64, -(-N // 64) * 64, batch)


def _divergence_flags(divergence, fixed_w=False, h_ones=False, groups=1, flags=0, free_atoms=0):
    """The flag bits of ``divergence``; 'is' / 'euclidean' combine with none of the other forms of the call."""
    d = check_divergence(divergence)
    if d != 'kl' and (fixed_w or h_ones or groups > 1 or free_atoms or flags & 6):
        raise ValueError('divergence=%r cannot be combined with a fixed dictionary, the all-ones start, free atoms, file groups or the '
                         'unfused W update' % (d,))
    return DIVERGENCE_FLAGS[d]


GCCNMF_FLAG_CONTINUITY = 1 << 28               # include/gccnmf_hip.h: temporal-continuity KL-NMF (the weight rides in K and batch)
GCCNMF_FLAG_CONTINUITY_STEREO = 1 << 29        # include/gccnmf_hip.h: ... inside two column segments [L | R]
CONTINUITY_MAX_ATOMS, CONTINUITY_MAX_BINS, CONTINUITY_MAX_BATCH = 1024, 2049, 65535      # the envelope of the temporal-continuity call


def check_continuity(weight, segments=1):
    """The ``continuity`` / ``segments`` keywords of klnmf and klnmf_stage, the ``temporalContinuity`` of the engines and of
    performTemporalKLNMF; no device needed.  Returns (weight as a float, segments as an int); ValueError unless the weight is a real,
    finite number >= 0 (not a bool) and segments is 1 or 2."""
    if isinstance(weight, bool) or not isinstance(weight, numbers.Real) or not math.isfinite(weight) or weight < 0:
        raise ValueError('the temporal-continuity weight must be a finite number >= 0, got %r' % (weight,))
    if isinstance(segments, bool) or not isinstance(segments, numbers.Integral) or segments not in (1, 2):
        raise ValueError('the temporal-continuity term runs inside 1 or 2 column segments, got %r' % (segments,))
    return float(weight), int(segments)


def klnmf_continuity_extra_floats(Kp, Np, batch):
    """GCCNMF_KLNMF_CONTINUITY_WORKSPACE_FLOATS(Kp, Np, batch) of include/gccnmf_hip.h: the floats a temporal-continuity call needs behind
    the KL layout -- Gm | Gp [batch][Kp][Np] each | E | D [batch][2][Kp] each."""
    return batch * Kp * (2 * Np + 4)


def klnmf_continuity_workspace_floats(F, N, K, batch):
    """Floats of the workspace of a temporal-continuity gccnmf_klnmf / gccnmf_klnmf_stage call: gccnmf_klnmf_workspace_floats followed
    by the extra blocks above."""
    n = lib().gccnmf_klnmf_workspace_floats(F, N, K, batch)
    return n if n < 0 else n + klnmf_continuity_extra_floats(-(-K // 64) * 64, -(-N // 64) * 64, batch)


def continuity_words(K, batch, weight):
    """(K, batch) arguments of a call with GCCNMF_FLAG_CONTINUITY: the float32 bits of the weight in their upper halves
    (GCCNMF_CONTINUITY_K / GCCNMF_CONTINUITY_BATCH of include/gccnmf_hip.h), as signed 32-bit values."""
    bits = ctypes.c_uint32.from_buffer_copy(ctypes.c_float(weight)).value
    signed = lambda v: ctypes.c_int32(v & 0xffffffff).value
    return signed(int(K) | (bits & 0xffff0000)), signed(int(batch) | ((bits & 0xffff) << 16))


def _continuity_words(continuity, segments, F, N, K, batch, flags, other):
    """(flags, K, batch) as the library takes them.  A weight of 0 sends the words of a call without the keyword; a weight above 0
    combines with none of the other forms of the call (``other``) and carries its envelope (ValueError before the library is touched)."""
    weight, segments = check_continuity(continuity, segments)
    if weight == 0:
        return flags, K, batch
    if other or flags & 6:
        raise ValueError('temporal continuity cannot be combined with a fixed dictionary, the all-ones start, free atoms, another '
                         'divergence, file groups or the unfused W update')
    if not 2 <= F <= CONTINUITY_MAX_BINS or not 1 <= K <= CONTINUITY_MAX_ATOMS or not 1 <= batch <= CONTINUITY_MAX_BATCH:
        raise ValueError('the temporal-continuity call takes 2 to %d bins, 1 to %d atoms and 1 to %d files, got F = %r, K = %r, batch = %r'
                         % (CONTINUITY_MAX_BINS, CONTINUITY_MAX_ATOMS, CONTINUITY_MAX_BATCH, F, K, batch))
    if ctypes.c_float(weight).value in (0.0, float('inf')):
        raise ValueError('the temporal-continuity weight %r is not a positive finite float32' % (weight,))
    if segments == 2 and N % 2:
        raise ValueError('two column segments need an even number of columns, got %d' % N)
    K, batch = continuity_words(K, batch, weight)
    return flags | GCCNMF_FLAG_CONTINUITY | (GCCNMF_FLAG_CONTINUITY_STEREO if segments == 2 else 0), K, batch


def klnmf(V, W, H, ws, F, N, K, batch, iterations, alpha, eps, fixed_w=False, h_ones=False, groups=1, flags=0, free_atoms=0, stream=None,
          divergence='kl', continuity=0.0, segments=1):
    """``iterations`` NMF iterations on W and H in place -- KL, or with divergence='is' / 'euclidean' Itakura-Saito / Euclidean (the
    workspace is then klnmf_divergence_workspace_floats(..., divergence) floats).  groups > 1: this call is one of that many concurrent ones
    (GCCNMF_FLAG_GROUPS(n) = 4 | n << 8: launch forms are chosen for all groups together); flags: further low flag bits.
    free_atoms = n > 0: semi-supervised -- columns [0, K - n) of every file's W are a dictionary that stays as it is, the last n atoms
    and all of H are learned (GCCNMF_FLAG_FREE_ATOMS(n)).
    continuity = weight > 0: KL-NMF with the temporal-continuity term inside ``segments`` (1 | 2) equal column runs (GCCNMF_FLAG_CONTINUITY;
    the workspace is then klnmf_continuity_workspace_floats floats); 0 sends exactly the words of a call without the keyword."""
    flags |= _divergence_flags(divergence, fixed_w, h_ones, groups, flags, free_atoms)
    flags, Kw, batchw = _continuity_words(continuity, segments, F, N, K, batch, flags,
                                          fixed_w or h_ones or groups > 1 or free_atoms or check_divergence(divergence) != 'kl')
    if free_atoms:
        if fixed_w or h_ones or groups > 1 or flags & 6:
            raise ValueError('free atoms cannot be combined with a fixed dictionary, the all-ones start, file groups or the unfused W update')
        flags |= GCCNMF_FLAG_FREE_ATOMS(check_free_atoms(free_atoms, K - free_atoms, F))
    flags |= (GCCNMF_FLAG_FIXED_W if fixed_w else 0) | (GCCNMF_FLAG_H_ONES if h_ones else 0) | (4 | groups << 8 if groups > 1 else 0)
    _stage('gccnmf_klnmf', V, W, H, ws, F, N, Kw, batchw, iterations, alpha, eps, flags, stream=stream)


def klnmf_stage(V, W, H, ws, F, N, K, batch, alpha, eps, stage, flags=0, free_atoms=0, stream=None, divergence='kl', continuity=0.0,
                segments=1):
    """One stage (0-7) of the iteration through gccnmf_klnmf_stage; flags: low flag bits, free_atoms / divergence / continuity / segments
    as for klnmf."""
    flags |= _divergence_flags(divergence, flags=flags, free_atoms=free_atoms)
    flags, Kw, batchw = _continuity_words(continuity, segments, F, N, K, batch, flags, free_atoms or check_divergence(divergence) != 'kl')
    if free_atoms:
        flags |= GCCNMF_FLAG_FREE_ATOMS(check_free_atoms(free_atoms, K - free_atoms, F))
    _stage('gccnmf_klnmf_stage', V, W, H, ws, F, N, Kw, batchw, alpha, eps, flags, int(stage), stream=stream)


def klnmf_divergence(V, W, H, ws, F, N, K, batch, fixed=False, stream=None, divergence='kl'):
    """One stage-7 launch of gccnmf_klnmf_stage: D(V || W.H) of every file of a padded batch -- the KL divergence, or with
    divergence='is' / 'euclidean' the Itakura-Saito divergence over the elements with V > 0 / half the squared Euclidean distance.  Returns the (batch,) float64 DEVICE
    view of the result inside the workspace `ws` (valid until the workspace is used again); asynchronous.  fixed: W is one shared
    [Fp][Kp] dictionary."""
    Fp, Np = -(-F // 16) * 16, -(-N // 64) * 64
    _stage('gccnmf_klnmf_stage', V, W, H, ws, F, N, K, batch, 0.0, 0.0, (GCCNMF_FLAG_FIXED_W if fixed else 0) | _divergence_flags(divergence, fixed_w=fixed),
           GCCNMF_STAGE_DIVERGENCE,
           stream=stream, what='gccnmf_klnmf_stage (divergence)')
    at = batch * Fp * Np
    return ws[at:at + 2 * batch].view(torch.float64)


def klnmf_chain_status(ws, F, N, K, batch):
    """Status word of the last chained KL-NMF launch in the workspace `ws` (0 = clean or not chained); the caller has synchronised."""
    st = c_int(0)
    check(lib().gccnmf_klnmf_chain_status(_ptr(ws), F, N, K, batch, ctypes.byref(st)), 'gccnmf_klnmf_chain_status')
    return st.value


def angular_nl_words(D, batch, alpha):
    """(D, batch) arguments of gccnmf_angular_spectrogram with GCC-NONLIN on: the float32 bits of alpha in their upper halves
    (GCCNMF_ANGULAR_NL_D / GCCNMF_ANGULAR_NL_BATCH of include/gccnmf_hip.h), as signed 32-bit values."""
    if not (0 < int(D) < 65536 and 0 < int(batch) < 65536):
        raise ValueError('GCC-NONLIN takes D and batch below 65536, got %r, %r' % (D, batch))
    bits = ctypes.c_uint32.from_buffer_copy(ctypes.c_float(alpha)).value
    signed = lambda v: ctypes.c_int32(v & 0xffffffff).value
    return signed(int(D) | (bits & 0xffff0000)), signed(int(batch) | ((bits & 0xffff) << 16))


def angular_spectrogram(CC, trig, F, T, D, batch, ang, mean_ang, nl_alpha=None, stream=None):
    """nl_alpha: None = GCC-PHAT, else the GCC-NONLIN spectrum with that alpha (only the localisation changes)."""
    if nl_alpha is not None:
        D, batch = angular_nl_words(D, batch, nl_alpha)
    _stage('gccnmf_angular_spectrogram', CC, trig, F, T, D, batch, ang, mean_ang, stream=stream)


def pick_tdoa_peaks(mean_ang, D, Dp, S, batch, idx, status, stream=None):
    """The S largest peaks of each file's mean angular spectrum [batch][Dp] -> idx [batch][S], status [batch]."""
    _stage('gccnmf_pick_tdoa_peaks', mean_ang, D, Dp, S, batch, idx, status, stream=stream)


TRACKS_MAX_FRAMES = (1 << 21) - 1


def peaks_tracks_word(S, L, T):
    """The S argument of gccnmf_pick_tdoa_peaks in its tracks mode: GCCNMF_PEAKS_TRACKS(S, L) of include/gccnmf_hip.h.  A window of
    2T - 1 frames or more is the whole file for every frame, so L is passed as min(L, 2T - 1)."""
    if not (1 <= int(S) <= 255 and 1 <= int(T) <= TRACKS_MAX_FRAMES and int(L) >= 1):
        raise ValueError('tracks take 1 <= S <= 255, 1 <= T < 2^21 and L >= 1, got %r, %r, %r' % (S, T, L))
    return int(S) | 0x100 | (min(int(L), 2 * int(T) - 1) << 9)


def pick_tdoa_tracks(ang, D, T, S, window, batch, tracks, status, stream=None):
    """The same entry point in its tracks mode: reads the angular spectrogram itself (the Dp argument carries T) and writes the peaks
    of every frame's windowed mean -> tracks [batch][S][Tp], status [batch][Tp]."""
    _stage('gccnmf_pick_tdoa_peaks', ang, D, T, peaks_tracks_word(S, window, T), batch, tracks, status, stream=stream,
           what='gccnmf_pick_tdoa_peaks (tracks)')


GCCNMF_SCORES_TRACKS = 0x100            # include/gccnmf_hip.h: per-(target, frame) indexes in gccnmf_target_scores_masks


def target_scores_masks(CC, trig, idx, W, F, T, K, D, S, batch, ws, scores, argmax, tracks=False, stream=None):
    """idx: one TDOA index per (file, target), or with tracks one per (file, target, frame) [batch][S][Tp]."""
    _stage('gccnmf_target_scores_masks', CC, trig, idx, W, F, T, K, D, S | GCCNMF_SCORES_TRACKS if tracks else S, batch, ws, scores,
           argmax, stream=stream)


GCCNMF_PEAKS_COUNT_BIT = 1 << 30        # include/gccnmf_hip.h: the count mode of gccnmf_pick_tdoa_peaks (numSources='auto')
GCCNMF_SCORES_COUNTED = 0x800           # include/gccnmf_hip.h: negative indexes are absent targets in gccnmf_target_scores_masks
MAX_AUTO_SOURCES = 8                    # the default cap of numSources='auto' (the ratio and spatial reconstructions' limit)
ENGINE_MAX_AUTO_TARGETS = 8             # GCCNMFEngine(numTargets='auto', maxTargets=...): RATIO_MAX_TARGETS, whatever the reconstruction


def check_auto_sources(numSources, maxSources=MAX_AUTO_SOURCES):
    """The ``numSources`` argument where 'auto' is accepted, and the cap that goes with it; no device needed.  Returns True for 'auto'
    (the count comes from the angular spectrum, ``maxSources`` at the most: a whole number from 1 to 255) and False for anything that is
    not a string (the callers' own rules for a fixed count apply: None, 0 and every other falsy value keep raising there).  ValueError:
    any other string, a cap that is no whole number in [1, 255]."""
    if isinstance(numSources, str):
        if numSources != 'auto':
            raise ValueError("numSources must be a number of sources or 'auto', got %r" % (numSources,))
        m = maxSources
        if isinstance(m, bool) or not isinstance(m, numbers.Integral) or not 1 <= m <= 255:
            raise ValueError('maxSources must be a whole number from 1 to 255, got %r' % (m,))
        return True
    return False


def check_auto_targets(numTargets, maxTargets, tdoaTracking=False):
    """The ``numTargets`` / ``maxTargets`` keywords of the engines; no device needed.  Returns (auto, S): for numTargets='auto' the
    buffers' target count S is ``maxTargets`` (default 4; a whole number from 1 to 8), otherwise S is ``numTargets`` as given.
    ValueError: 'auto' with tdoaTracking (the tracks kernel takes one count per launch), maxTargets without 'auto', another string."""
    if check_auto_sources(numTargets, 1):
        if tdoaTracking:
            raise ValueError("numTargets='auto' cannot be combined with tdoaTracking (every frame's peak set takes one count per launch)")
        m = 4 if maxTargets is None else maxTargets
        if isinstance(m, bool) or not isinstance(m, numbers.Integral) or not 1 <= m <= ENGINE_MAX_AUTO_TARGETS:
            raise ValueError('maxTargets must be a whole number from 1 to %d, got %r' % (ENGINE_MAX_AUTO_TARGETS, m))
        return True, int(m)
    if maxTargets is not None:
        raise ValueError("maxTargets needs numTargets='auto'")
    return False, numTargets


def peaks_count_word(maxSources):
    """The S argument of gccnmf_pick_tdoa_peaks in its count mode: GCCNMF_PEAKS_COUNT(Smax) of include/gccnmf_hip.h."""
    check_auto_sources('auto', maxSources)
    return int(maxSources) | GCCNMF_PEAKS_COUNT_BIT


def count_tdoa_peaks(mean_ang, D, Dp, maxSources, batch, idx, status, stream=None):
    """The same entry point in its count mode: every file keeps as many peaks as it has talkers (the exact 2-means split of its peak
    heights), ``maxSources`` at the most -> idx [batch][maxSources] (ascending, then -1), status [batch] (0, 1 = nothing to count,
    2 = capped)."""
    _stage('gccnmf_pick_tdoa_peaks', mean_ang, D, Dp, peaks_count_word(maxSources), batch, idx, status, stream=stream,
           what='gccnmf_pick_tdoa_peaks (count)')


def target_scores_masks_counted(CC, trig, idx, W, F, T, K, D, S, batch, ws, scores, argmax, counted=False, stream=None):
    """target_scores_masks with fixed indexes; counted: idx [batch][S] as count_tdoa_peaks writes it -- a negative index is a target
    the file does not have (NaN scores, never the arg-max).  counted=False is the plain call."""
    if not 1 <= int(S) <= 255:
        raise ValueError('the score stage takes 1 to 255 targets, got %r' % (S,))
    _stage('gccnmf_target_scores_masks', CC, trig, idx, W, F, T, K, D, int(S) | GCCNMF_SCORES_COUNTED if counted else int(S), batch, ws,
           scores, argmax, stream=stream, what='gccnmf_target_scores_masks (counted)' if counted else None)


GCCNMF_SCORES_ATOM_TDOA = 0x200         # include/gccnmf_hip.h: the full-grid atom TDOA arg-max, a mode of gccnmf_target_scores_masks
GCCNMF_SCORES_ENHANCEMENT_MASKS = 0x400  # include/gccnmf_hip.h: talker / noise masks from the atom TDOA image, likewise
ATOM_TDOA_MAX_D = 1024                  # csrc/atom_tdoa.h: the streaming limit
TARGET_MODE_BOXCAR, TARGET_MODE_MULTIPLE, TARGET_MODE_WINDOW_FUNCTION = 0, 1, 2      # gccNMF/realtime/gccNMFProcessor.py:35-37 (realtime.py exports the same)


def atom_tdoa_indexes(CC, trig, W, F, T, K, D, batch, atom_tdoa, atom_score=None, stream=None):
    """GCCNMF_ATOM_TDOA_INDEXES: every atom's arg-max over the whole TDOA grid -> atom_tdoa [batch][Kp][Tp] uint16 (a torch.int16
    tensor's bits), atom_score [batch][Kp][Tp] float32 or None.  No workspace."""
    _stage('gccnmf_target_scores_masks', CC, trig, None, W, F, T, K, D, GCCNMF_SCORES_ATOM_TDOA, batch, None, atom_score, atom_tdoa,
           stream=stream, what='gccnmf_target_scores_masks (atom TDOA)')


def check_enhancement_target(targetMode, targetTDOAEpsilon, targetTDOABeta, targetTDOANoiseFloor):
    """The mask settings of the enhancement path (gccNMF/realtime/config.py:56-58) as the library takes them; no device needed.
    Returns (window, eps, beta, noiseFloor): window 0 = TARGET_MODE_BOXCAR, 1 = TARGET_MODE_WINDOW_FUNCTION; eps > 0, beta > 0,
    noiseFloor >= 0, all finite (checked whatever the mode, so a bad value cannot wait for the switch).  ValueError otherwise."""
    modes = {'boxcar': 0, 'window': 1, TARGET_MODE_BOXCAR: 0, TARGET_MODE_WINDOW_FUNCTION: 1}
    if isinstance(targetMode, bool) or targetMode not in modes:
        raise ValueError("targetMode must be TARGET_MODE_BOXCAR / 'boxcar' or TARGET_MODE_WINDOW_FUNCTION / 'window', got %r" % (targetMode,))
    out = []
    for name, v, low_ok in (('targetTDOAEpsilon', targetTDOAEpsilon, False), ('targetTDOABeta', targetTDOABeta, False),
                            ('targetTDOANoiseFloor', targetTDOANoiseFloor, True)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v < 0 or (v == 0 and not low_ok):
            raise ValueError('%s must be a finite number %s 0, got %r' % (name, '>=' if low_ok else '>', v))
        v32 = ctypes.c_float(float(v)).value
        if not math.isfinite(v32) or (v32 == 0 and not low_ok):
            raise ValueError('%s=%r is not a float32 number %s 0' % (name, v, '>=' if low_ok else '>'))
        out.append(v32)
    return (modes[targetMode],) + tuple(out)


def enhancement_masks(atom_tdoa, target, T, K, batch, image, masks, window=0, eps=5.0, beta=2.0, noise_floor=0.0, per_frame=False, stream=None):
    """GCCNMF_ENHANCEMENT_MASKS: atom_tdoa [batch][Kp][Tp] uint16 and target [batch] int32 (per_frame: [batch][Tp]) -> image
    [batch][Kp][Tp] uint8 (0 talker, 1 noise) and / or masks [batch][2][Kp][Tp] float32 (talker, noise); either may be None.
    window: 0 = boxcar, 1 = window function.  (eps, beta, noise_floor) travel as three host floats, read during the call."""
    if window not in (0, 1):
        raise ValueError('window must be 0 (boxcar) or 1 (window function), got %r' % (window,))
    params = (c_float * 3)(eps, beta, noise_floor)
    word = GCCNMF_SCORES_ENHANCEMENT_MASKS | int(window) | (GCCNMF_SCORES_TRACKS if per_frame else 0)
    _stage('gccnmf_target_scores_masks', atom_tdoa, ctypes.addressof(params), target, None, 0, T, K, 0, word, batch, None, masks, image,
           stream=stream, what='gccnmf_target_scores_masks (enhancement masks)')


def argmax_targets(scores, K, T, S, batch, argmax, stream=None):
    _stage('gccnmf_argmax_targets', scores, K, T, S, batch, argmax, stream=stream)


RECONSTRUCTIONS = ('direct', 'ratio', 'spatial')
GCCNMF_RECONSTRUCT_RATIO = 0x100        # include/gccnmf_hip.h: the ratio-mask mode of gccnmf_reconstruct, above the low byte of S
RATIO_MAX_TARGETS = 8                   # csrc/ratio.h, csrc/spatial.h
GCCNMF_RECONSTRUCT_SPATIAL_BIT = 1 << 16  # include/gccnmf_hip.h: the spatial filter behind the ratio stage, in the upper half of gccnmf_reconstruct's batch
GCCNMF_SPATIAL_LOADING = 1e-3           # include/gccnmf_hip.h: the diagonal loading of the spatial covariances
GCCNMF_RECONSTRUCT_SPATIAL_ITERATIONS_SHIFT = 20   # include/gccnmf_hip.h: GCCNMF_RECONSTRUCT_SPATIAL_ITERATIONS(n), bits 20-27 of gccnmf_reconstruct's S
MAX_SPATIAL_ITERATIONS = 255


def check_reconstruction(reconstruction, numTargets):
    """The ``reconstruction`` keyword of the engines and of getTargetSpectrogramEstimates; ValueError before any device work."""
    if reconstruction not in RECONSTRUCTIONS:
        raise ValueError("reconstruction must be 'direct', 'ratio' or 'spatial', got %r" % (reconstruction,))
    if reconstruction != 'direct' and not 1 <= int(numTargets) <= RATIO_MAX_TARGETS:
        raise ValueError("reconstruction=%r takes 1 to %d targets, got %d" % (reconstruction, RATIO_MAX_TARGETS, int(numTargets)))
    return reconstruction


def check_spatial_iterations(spatialIterations, reconstruction):
    """The ``spatialIterations`` keyword (EM iterations behind reconstruction='spatial', csrc/spatial_em.hip); ValueError before any
    device work.  An int from 0 to 255; above 0 only with 'spatial'."""
    n = spatialIterations
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 0 <= int(n) <= MAX_SPATIAL_ITERATIONS:
        raise ValueError('spatialIterations must be an int from 0 to %d, got %r' % (MAX_SPATIAL_ITERATIONS, n))
    if int(n) and reconstruction != 'spatial':
        raise ValueError("spatialIterations=%d needs reconstruction='spatial', got %r" % (int(n), reconstruction))
    return int(n)


def reconstruct_word(S, mode, iterations=0):
    """The S argument of gccnmf_reconstruct: the target count with the mode above its low byte (GCCNMF_RECONSTRUCT_RATIO for 'ratio'
    and 'spatial', GCCNMF_RECONSTRUCT_SPATIAL_ITERATIONS(n) for the EM refinement of 'spatial')."""
    iterations = check_spatial_iterations(iterations, mode)
    word = int(S)
    if mode != 'direct':
        word |= GCCNMF_RECONSTRUCT_RATIO
    return word | (iterations << GCCNMF_RECONSTRUCT_SPATIAL_ITERATIONS_SHIFT)


def reconstruct_spatial_batch(batch):
    """The batch argument of gccnmf_reconstruct in its spatial mode: GCCNMF_RECONSTRUCT_SPATIAL_BATCH(batch) of include/gccnmf_hip.h."""
    if not 1 <= int(batch) <= 65535:
        raise ValueError('the spatial reconstruction takes 1 to 65535 files per call, got %r' % (batch,))
    return int(batch) | GCCNMF_RECONSTRUCT_SPATIAL_BIT


def reconstruct_spatial_workspace_floats(batch, S, Fp):
    """Floats of the covariance workspace of that mode: GCCNMF_RECONSTRUCT_SPATIAL_WORKSPACE_FLOATS(batch, S, Fp), Fp = round_up(F, 16)."""
    return 4 * int(batch) * int(S) * int(Fp)


def reconstruct_spatial_em_workspace_floats(batch, S, Fp, Tp):
    """Floats of that workspace with EM iterations: GCCNMF_RECONSTRUCT_SPATIAL_EM_WORKSPACE_FLOATS(batch, S, Fp, Tp), the covariances
    followed by the powers [batch][S][Fp][Tp]; Tp = round_up(T, 64)."""
    return reconstruct_spatial_workspace_floats(batch, S, Fp) + int(batch) * int(S) * int(Fp) * int(Tp)


def reconstruct_workspace_floats(mode, T, K, S, batch, Fp, iterations=0):
    """Floats of the workspace ``reconstruct`` takes in that mode: the masked H of 'direct', nothing for 'ratio' (one fused launch),
    the covariances [batch][S][Fp][4] of 'spatial', followed by the powers [batch][S][Fp][Tp] when it runs EM iterations."""
    iterations = check_spatial_iterations(iterations, mode)
    if mode == 'direct':
        return lib().gccnmf_reconstruct_workspace_floats(T, K, S, batch)
    if mode == 'spatial' and iterations:
        return reconstruct_spatial_em_workspace_floats(batch, S, Fp, -(-int(T) // 64) * 64)
    return reconstruct_spatial_workspace_floats(batch, S, Fp) if mode == 'spatial' else 0


def reconstruct(W, H, argmax, masks, X, V, F, T, K, S, batch, spec, mode='direct', workspace=None, iterations=0, stream=None):
    """Target spectrograms from the arg-max image or the masks (either may be None).  'ratio' reads neither V nor a workspace;
    'spatial' is the ratio launch, then the covariance reduction and the 2 x 2 filter over spec in place, with the covariances in
    ``workspace`` (a missing 'direct' workspace is the library's GCCNMF_ERR_ARG, as a missing V is); ``iterations`` EM iterations run
    between the two in one launch, and ``workspace`` then holds the powers too (reconstruct_workspace_floats(..., iterations))."""
    if mode not in RECONSTRUCTIONS:
        raise ValueError('unknown reconstruction mode %r' % (mode,))
    S = reconstruct_word(S, mode, iterations)
    if mode == 'spatial':
        if workspace is None:
            raise ValueError("reconstruction='spatial' needs its covariance workspace (reconstruct_workspace_floats)")
        batch = reconstruct_spatial_batch(batch)
    _stage('gccnmf_reconstruct', W, H, argmax, masks, X, V, F, T, K, S, batch, None if mode == 'ratio' else workspace, spec, stream=stream)


# frames_mode_bits of gccnmf_rt_process_block_ll (include/gccnmf_hip.h, csrc/rt.hip)
RT_FRAMES, RT_SKIP_LOCALIZE, RT_ONLY_LOCALIZE = 1, 2, 4
RT_BANK_LAYOUT, MAX_BANK_STREAMS = 1 << 3, 4096         # + (S - 1) << 8, bits 8..19
RT_MULTI_LAYOUT, MAX_SOURCES = 1 << 20, 8               # + (N - 1) << 21, bits 21..23
RT_ROW8_LAYOUT = 1 << 24                # single-stream call: the target row has 8 words, word 6 = gccPHATNLAlpha
RT_LOCALIZE = {'with': 0, 'skip': RT_SKIP_LOCALIZE, 'only': RT_ONLY_LOCALIZE}
RT_SEPARATION_SPATIAL = 2               # bit 1 of separation_enabled: the online spatial filter behind the mask kernel (csrc/rt_spatial.hip)
DEFAULT_SPATIAL_FILTER_FRAMES = 128.0   # spatialFilterFrames: the best tau of scripts/rt_spatial_filter_study.py


def rt_spatial_state_offset(D, numTDOAHistory, S=1):
    """Where the history ends and the spatial filter's state begins in the buffer behind ``hist``, in floats:
    GCCNMF_RT_SPATIAL_STATE_OFFSET(S, D, Lh) of include/gccnmf_hip.h, the first multiple of 4 behind the S history images."""
    return -(-(int(S) * int(D) * int(numTDOAHistory)) // 4) * 4


def rt_spatial_state_floats(F, NC, S=1):
    """Floats of that state, [S][NC][F][4]: GCCNMF_RT_SPATIAL_STATE_FLOATS(S, NC, F).  NC = 2 in the single-target modes (talker,
    residual), the number of targets in multiple mode."""
    return 4 * int(S) * int(NC) * int(F)


def check_spatial_filter(spatialFilterEnabled, spatialFilterFrames):
    """The ``spatialFilterEnabled`` / ``spatialFilterFrames`` settings of the real-time classes; no device needed.  Returns (enabled, tau):
    tau the time constant of the recursive covariance in frames, a finite number >= 1 that is a float32 (checked whether or not the
    filter is enabled, so a bad value cannot wait for the switch).  ValueError otherwise."""
    t = spatialFilterFrames
    if isinstance(t, bool) or not isinstance(t, numbers.Real) or not math.isfinite(t) or not t >= 1:
        raise ValueError('spatialFilterFrames must be a finite number of frames >= 1, got %r' % (t,))
    t32 = ctypes.c_float(float(t)).value
    if not math.isfinite(t32):
        raise ValueError('spatialFilterFrames=%r is not a float32' % (t,))
    return bool(spatialFilterEnabled), float(t32)


def rt_mode_word(frames=False, localize='with', streams=None, targets=None, nl_row=False, target_mode=TARGET_MODE_MULTIPLE):
    """frames_mode_bits for the keywords of ``rt_process_block``; ValueError for what the entry point rejects."""
    if not isinstance(localize, str) or localize not in RT_LOCALIZE:
        raise ValueError("localize must be 'with', 'skip' or 'only', got %r" % (localize,))
    word = (RT_FRAMES if frames else 0) | RT_LOCALIZE[localize] | (RT_ROW8_LAYOUT if nl_row else 0)
    if nl_row and (streams is not None or targets is not None):
        raise ValueError('nl_row is the single-stream, single-target row: the bank and multi-target rows always have word 6')
    if streams is not None:
        if frames:
            raise ValueError('a bank of streams has no frames mode')
        if not 1 <= int(streams) <= MAX_BANK_STREAMS:
            raise ValueError('a bank holds 1 to %d streams, got %r' % (MAX_BANK_STREAMS, streams))
        word |= RT_BANK_LAYOUT | (int(streams) - 1) << 8
    if targets is not None:
        if int(target_mode) != TARGET_MODE_MULTIPLE:
            raise ValueError('the multi-target layout needs TARGET_MODE_MULTIPLE, got target_mode %r' % (target_mode,))
        if not 1 <= int(targets) <= MAX_SOURCES:
            raise ValueError('the multi-target layout takes 1 to %d targets, got %r' % (MAX_SOURCES, targets))
        word |= RT_MULTI_LAYOUT | (int(targets) - 1) << 21
    return word


def rt_process_block(block_in, block_out, in_ring, out_ring, X, Y, C, HMask, argmaxTDOA, tfMask, hist, hist_pos, target, gccphat, W, cosT,
                     sinT, window, synthesis_window, twiddle, colsumW, Hcoef, Rv, windowSize, hopSize, blockSize, K, Kp, D, Dp, numTDOAHistory,
                     target_mode, separation_enabled, localization_enabled, localization_window, numHUpdates=0, out_delay_blocks=2,
                     frames=False, localize='with', streams=None, targets=None, nl_row=False, spatial=False, stream=None):
    """One real-time block call (csrc/rt.hip); the buffers and geometry in the header's order, the modes as keywords.
    frames: GCCNMFProcessor.processFrames on its own (in_ring / out_ring are the frames, no shift or overlap-add).
    localize: 'with' the tracking update, 'skip' it, or 'only' it ('skip' then 'only' = the same work in two calls, so that a host can
    fetch block_out before the tracking update has run).
    streams = S: the buffers hold a bank of S streams (8-word target rows).  targets = N: the multi-target layout of
    TARGET_MODE_MULTIPLE (16-word rows, N masks and outputs per stream).  nl_row: the single-stream target row has 8 words, word 6 =
    gccPHATNLAlpha (the other two layouts always have it).
    spatial: the online spatial filter runs behind the mask kernel for every stream whose row word 7 holds a time constant >= 1 frames
    (separation word 3 = 1 | RT_SEPARATION_SPATIAL; with the separation off the word is 0 and nothing is filtered).  ``hist`` is then
    followed by the filter's state (rt_spatial_state_offset, rt_spatial_state_floats); needs a row with a word 7, so nl_row in the
    single-stream, single-target call."""
    word = rt_mode_word(frames, localize, streams, targets, nl_row, target_mode)
    if spatial and not (nl_row or streams is not None or targets is not None):
        raise ValueError('spatial needs a target row with a word 7: nl_row, a bank of streams or the multi-target layout')
    separation = (1 | (RT_SEPARATION_SPATIAL if spatial else 0)) if separation_enabled else 0
    _stage('gccnmf_rt_process_block_ll', block_in, block_out, in_ring, out_ring, X, Y, C, HMask, argmaxTDOA, tfMask, hist, hist_pos, target,
           gccphat, W, cosT, sinT, window, synthesis_window, twiddle, colsumW, Hcoef, Rv, windowSize, hopSize, blockSize, K, Kp, D, Dp,
           numTDOAHistory, int(target_mode), separation, int(bool(localization_enabled)), localization_window, word,
           int(numHUpdates), int(out_delay_blocks), stream=stream)
