"""ctypes binding of libgccnmf_eval.so (include/gccnmf_eval.h): the scoring kernels of ``evaluation.py``.

A library of its own beside libgccnmf_hip.so (scoring is not part of the separation ABI), with the same conventions: the status codes
and ``HipLibraryError`` of ``_hip``, NO CPU fallback -- a missing library, a missing symbol or a missing device is an error on every
call path.  Below ``lib()``: one plain function per kernel (pointers are tensors, the stream defaults to torch's current one).
"""
import ctypes
import os

import torch

from . import _hip
from ._hip import STATUS, HipLibraryError, check, _ptr, _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libgccnmf_eval.so')

c_int, c_long, c_void_p = ctypes.c_int, ctypes.c_long, ctypes.c_void_p

GCCNMF_EVAL_SYMMETRIC = 1            # include/gccnmf_eval.h: B is A
GCCNMF_EVAL_BLOCK = 1024             # include/gccnmf_eval.h: samples per partial sum of the lag correlations
MAX_FILTER_LENGTH = 4096

# name -> (restype, argtypes); mirrors include/gccnmf_eval.h declaration by declaration
SIGNATURES = {
    'gccnmf_eval_version': (c_int, []),
    'gccnmf_eval_workspace_bytes': (c_long, [c_int, c_int, c_int, c_int, c_int]),
    'gccnmf_eval_lag_correlations': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'gccnmf_eval_project': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
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
    _hip.require_device(lib, 'the scoring kernels have')


def workspace_bytes(Ma, Mb, n, L, batch):
    """Bytes of the partial-sum workspace of ``lag_correlations``; HipLibraryError for arguments the call would reject."""
    size = lib().gccnmf_eval_workspace_bytes(Ma, Mb, n, L, batch)
    if size < 0:
        raise HipLibraryError('gccnmf_eval_workspace_bytes(%d, %d, %d, %d, %d): %s' % (Ma, Mb, n, L, batch, STATUS[1]))
    return size


def lag_correlations(A, B, L, workspace=None, R=None, stream=None):
    """A (batch, Ma, n), B (batch, Mb, n) float32 device tensors -> R (batch, Ma, Mb, 2L - 1) float64:
    R[a][b][l + L - 1] = sum_n A_a[n] B_b[n + l].  ``B is A`` (the same tensor) takes the symmetric form of the call: half the sums, R
    symmetric to the bit.  ``workspace``: a uint8 tensor of ``workspace_bytes`` or None to allocate one."""
    batch, Ma, n = A.shape
    Mb = B.shape[1]
    assert A.dtype == B.dtype == torch.float32 and A.is_contiguous() and B.is_contiguous() and B.shape == (batch, Mb, n)
    need = workspace_bytes(Ma, Mb, n, L, batch)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=A.device)
    assert workspace.numel() * workspace.element_size() >= need
    if R is None:
        R = torch.empty((batch, Ma, Mb, 2 * L - 1), dtype=torch.float64, device=A.device)
    assert R.dtype == torch.float64 and R.is_contiguous() and R.shape == (batch, Ma, Mb, 2 * L - 1)
    flags = GCCNMF_EVAL_SYMMETRIC if B is A else 0
    check(lib().gccnmf_eval_lag_correlations(_ptr(A), _ptr(B), Ma, Mb, n, L, batch, flags, _ptr(workspace), _ptr(R),
                                             _stream(A.device) if stream is None else stream), 'gccnmf_eval_lag_correlations')
    return R


def project(A, coef, ref_ranges, P=None, stream=None):
    """A (batch, Ma, n) float32, coef (batch, Q, Ma, L) float64, ref_ranges (Q, 2) int32 [first_ref, num_refs] device tensors ->
    P (batch, Q, n + L - 1) float64: P[q][m] = sum_{a in refs(q)} sum_tau coef[q][a][tau] A_a[m - tau]."""
    batch, Ma, n = A.shape
    Q, L = coef.shape[1], coef.shape[3]
    assert A.dtype == torch.float32 and A.is_contiguous()
    assert coef.dtype == torch.float64 and coef.is_contiguous() and coef.shape == (batch, Q, Ma, L)
    assert ref_ranges.dtype == torch.int32 and ref_ranges.is_contiguous() and ref_ranges.shape == (Q, 2)
    if P is None:
        P = torch.empty((batch, Q, n + L - 1), dtype=torch.float64, device=A.device)
    assert P.dtype == torch.float64 and P.is_contiguous() and P.shape == (batch, Q, n + L - 1)
    check(lib().gccnmf_eval_project(_ptr(A), _ptr(coef), _ptr(ref_ranges), Ma, Q, n, L, batch, _ptr(P),
                                    _stream(A.device) if stream is None else stream), 'gccnmf_eval_project')
    return P
