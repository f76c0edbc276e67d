"""ctypes binding of libgccnmf_array_em.so (include/gccnmf_array_em.h): the EM refinement of the M x M spatial (multichannel Wiener)
filter of ``array.py`` (``GCCNMFArrayEngine(reconstruction='spatial', spatialIterations=n)``).

A library of its own beside libgccnmf_array_spatial.so, with the same conventions: the status codes and ``HipLibraryError`` of ``_hip``,
NO CPU fallback -- a missing library, a missing symbol or a missing device is an error on every call path.  Below ``lib()``: one plain
function per entry point (pointers are tensors, the stream defaults to torch's current one).
"""
import ctypes
import os

from . import _hip
from ._hip import HipLibraryError, check, _ptr, _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libgccnmf_array_em.so')

c_int, c_long, c_void_p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p

MAX_ITERATIONS = 255                 # include/gccnmf_array_em.h: GCCNMF_ARRAY_EM_MAX_ITERATIONS

# name -> (restype, argtypes); mirrors include/gccnmf_array_em.h declaration by declaration
SIGNATURES = {
    'gccnmf_array_em_version': (c_int, []),
    'gccnmf_array_em_workspace_floats': (c_long, [c_int, c_int, c_int, c_int, c_int]),
    'gccnmf_array_em': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
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
    _hip.require_device(lib, 'the EM refinement of the array spatial filter has')


def workspace_floats(M, F, T, S, batch):
    """Floats of ``workspace``: cov [batch][S][Fp][M M], then the powers [batch][S][Fp][Tp]; HipLibraryError for a shape the library
    rejects."""
    need = lib().gccnmf_array_em_workspace_floats(M, F, T, S, batch)
    if need < 0:
        raise HipLibraryError('gccnmf_array_em_workspace_floats rejected M = %d, F = %d, T = %d, S = %d, batch = %d' % (M, F, T, S, batch))
    return need


def em(X, M, F, T, S, batch, nsig_pitch, n, workspace, spec, stream=None):
    """The covariance launch, n EM iterations (one launch) and the filter launch: spec [batch][nsig_pitch][Fp][Tp][2] (slot i M + c, the
    ratio-mode estimates) is overwritten in place with the filtered estimates; workspace holds the refined cov and the refined powers."""
    check(lib().gccnmf_array_em(_ptr(X), M, F, T, S, batch, nsig_pitch, n, _ptr(workspace), _ptr(spec),
                                _stream() if stream is None else stream), 'gccnmf_array_em')
