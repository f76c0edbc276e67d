"""ctypes binding of libgccnmf_array.so (include/gccnmf_array.h): the microphone-array stages of ``array.py``.

A library of its own beside libgccnmf_hip.so (the M-channel stages are not part of the stereo separation ABI), with the same conventions:
the status codes and ``HipLibraryError`` of ``_hip``, NO CPU fallback -- a missing library, a missing symbol or a missing device is an
error on every call path.  Below ``lib()``: one plain function per entry point (pointers are tensors, the stream defaults to torch's
current one).
"""
import ctypes
import os

from . import _hip
from ._hip import HipLibraryError, check, _ptr, _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libgccnmf_array.so')

c_int, c_void_p = ctypes.c_int, ctypes.c_void_p

MIN_CHANNELS = 2                     # include/gccnmf_array.h: GCCNMF_ARRAY_MIN_CHANNELS
MAX_CHANNELS = 8                     # include/gccnmf_array.h: GCCNMF_ARRAY_MAX_CHANNELS
MAX_TARGETS = 8                      # include/gccnmf_array.h: GCCNMF_ARRAY_MAX_TARGETS

# name -> (restype, argtypes); mirrors include/gccnmf_array.h declaration by declaration
SIGNATURES = {
    'gccnmf_array_version': (c_int, []),
    'gccnmf_array_features': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'gccnmf_array_reconstruct': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                         c_void_p, c_void_p]),
}

_lib = None


def lib():
    """The loaded shared library with typed prototypes; raises HipLibraryError if it cannot be used."""
    global _lib
    if _lib is None:
        _lib = _hip.load_library(LIB_PATH, SIGNATURES)
    return _lib


def require_device():
    """HipLibraryError unless the library loads and a ROCm device is visible."""
    _hip.require_device(lib, 'the microphone-array kernels have')


def num_pairs(M):
    return M * (M - 1) // 2


def pairs(M):
    """The microphone pairs (a, b), a < b, in the library's (lexicographic) order."""
    return [(a, b) for a in range(M) for b in range(a + 1, M)]


def features(X, M, F, T, batch, V, CC, stream=None):
    """X [batch][M][Fp][Tp][2] -> V [batch][Fp][Np] (magnitudes side by side) and CC [batch][2][P Fp][Tp] (the pairs' PHAT coherence,
    stacked along the bin axis); either output may be None."""
    check(lib().gccnmf_array_features(_ptr(X), M, F, T, batch, _ptr(V), _ptr(CC), _stream() if stream is None else stream),
          'gccnmf_array_features')


def reconstruct(W, H, argmax, masks, X, M, F, T, K, S, batch, nsig_pitch, spec, stream=None):
    """The ratio-mask reconstruction for M channels: spec [batch][nsig_pitch][Fp][Tp][2], slot i M + c; the one-hot form reads ``argmax``,
    the soft form ``masks`` (taken when given)."""
    check(lib().gccnmf_array_reconstruct(_ptr(W), _ptr(H), _ptr(argmax), _ptr(masks), _ptr(X), M, F, T, K, S, batch, nsig_pitch, _ptr(spec),
                                         _stream() if stream is None else stream), 'gccnmf_array_reconstruct')
