"""The chained launches of gccnmf_klnmf (tuning keys 21 / 23 / 24: gccnmf_gemm_chain_kernel, gccnmf_short_chain_kernel) and gccnmf_klnmf_ragged at the
smallest shapes that reach them, bit for bit against the plain launches -- include/gccnmf_hip.h, key 21: "Bitwise the same factors in every form".
tests/chained_small_cases.py is the case table and says what each shape is there for; tests/test_chained_small_cases_host.py shows on the host that
every call takes the form it is meant to.  The plain launches themselves are checked element by element against float64 at chain-capable shapes in
tests/test_gpu_klnmf_stages.py (test_chain_capable_shapes_on_the_plain_launches) and, here, against the oracle after a whole call.

Every call starts from a workspace of arbitrary bits.  After every call: the return code and the chain status are 0, W and H are finite, the padding
of W and H is exactly 0; after a one-iteration call every bin of V that is silent has an exactly-zero row of W and no other element of W is 0 (calls
of more iterations have no silent bin: the case table says why).  Every chained call is torch.equal to the plain one, padding included."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import chained_small_cases as C
import klnmf_stages_restatement as S
from oracle import gccnmf_oracle as O

pytestmark = pytest.mark.gpu


def _lib():
    from gcc_nmf_amd import _hip
    return _hip.lib()


@contextlib.contextmanager
def _tuning(*keys):
    lib, merged = _lib(), {}
    for k in keys:
        merged.update(k)
    try:
        for k, v in merged.items():
            assert lib.gccnmf_set_tuning(k, v) == 0, 'gccnmf_set_tuning(%d, %d) was refused: a product key, which every build accepts' % (k, v)
        yield lib
    finally:
        for k in merged:
            lib.gccnmf_set_tuning(k, C.DEFAULTS[k])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300)


def _up(n, m):
    return -(-n // m) * m


def _padded(arrays, rows, cols):
    """per-file 2-D arrays -> one zero-padded [files][rows][cols] device tensor"""
    t = torch.zeros((len(arrays), rows, cols), dtype=torch.float32)
    for b, a in enumerate(arrays):
        t[b, :a.shape[0], :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a))
    return t.cuda()


def _arbitrary_bits(n, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(1, 1 << 30, n).astype(np.int32)).cuda().view(torch.float32)


class Batch(object):
    """a uniform batch on the device: V, the initial factors (kept; every call gets copies) and the shape"""

    def __init__(self, V, W0, H0, K):
        self.V, self.B, self.F, self.N, self.K = V, len(V), V[0].shape[0], V[0].shape[1], K
        self.Fp, self.Kp, self.Np = _up(self.F, 16), _up(K, 64), _up(self.N, 64)
        self.dV = _padded(V, self.Fp, self.Np)
        self.dW0 = _padded(W0, self.Fp, self.Kp)
        self.dH0 = _padded(H0, self.Kp, self.Np)

    def call(self, lib, iterations, alpha, label):
        """gccnmf_klnmf under the tuning in force -> W, H; the per-call assertions of the module docstring"""
        F, N, K, B = self.F, self.N, self.K, self.B
        W, H = self.dW0.clone(), self.dH0.clone()
        ws = _arbitrary_bits(lib.gccnmf_klnmf_workspace_floats(F, N, K, B), B)
        rc = lib.gccnmf_klnmf(self.dV.data_ptr(), W.data_ptr(), H.data_ptr(), ws.data_ptr(), F, N, K, B, iterations, alpha, C.EPS, 0, _stream())
        assert rc == 0, '%s: gccnmf_klnmf returned %d' % (label, rc)
        torch.cuda.synchronize()
        st = ctypes.c_int(-1)
        assert lib.gccnmf_klnmf_chain_status(ws.data_ptr(), F, N, K, B, ctypes.byref(st)) == 0 and st.value == 0, '%s: chain status %d' % (label, st.value)
        _check_factors(W, H, F, [N] * B, K, label)
        if iterations == 1:
            silent = torch.from_numpy(np.stack([~v.any(axis=1) for v in self.V])).cuda()              # [B][F]
            assert silent.any(dim=1).all(), '%s: the problem has no silent bin' % label
            zero_rows = (W[:, :F, :K] == 0).all(dim=2)
            assert torch.equal(zero_rows, silent), '%s: the exactly-zero rows of W are not the silent bins of V' % label
            assert torch.equal((W[:, :F, :K] == 0).any(dim=2), silent), '%s: W has zeros outside the silent bins' % label
        return W, H


def _check_factors(W, H, F, lengths, K, label):
    assert torch.isfinite(W).all() and torch.isfinite(H).all(), '%s: W or H is not finite' % label
    assert not W[:, F:, :].any() and not W[:, :, K:].any() and not H[:, K:, :].any(), '%s: non-zero padding in W or in the rows of H' % label
    for f, n in enumerate(lengths):
        assert not H[f, :, n:].any(), '%s: file %d: H is not exactly 0 from column %d on' % (label, f, n)


def _same(got, want, label):
    for name, g, w in zip('WH', got, want):
        if not torch.equal(g, w):
            bad = (g != w).nonzero()
            raise AssertionError('%s: %s differs from the plain call in %d elements, first at %s: %r against %r'
                                 % (label, name, len(bad), tuple(bad[0].tolist()), g[tuple(bad[0])].item(), w[tuple(bad[0])].item()))


def _run_calls(case, base_keys, V, W0, H0):
    """every call of a case; -> the batch and the plain call's factors"""
    batch = Batch(V, W0, H0, case.K)
    plain = None
    for call in case.calls:
        label = '(%d, %d, %d) x %d, %d iterations, %s %s' % (case.F, case.N, case.K, case.B, case.iterations, call.name, call.keys)
        with _tuning(base_keys, call.keys) as lib:
            plan = lib.gccnmf_klnmf_plan(case.F, case.N, case.K, case.B, 0)
            assert plan & 15 == call.plan, '%s: gccnmf_klnmf_plan says %d, the case means %d' % (label, plan, call.plan)
            got = batch.call(lib, case.iterations, case.alpha, label)
        if plain is None:
            assert call.name == 'plain' and not plan & C.CHAINED
            plain = got
        else:
            # (a forced form the plan does not take -- the plain launch's lists at a batch that is no multiple of 8, the refused short shape -- has
            # been asserted above to BE the plain call; it ran, and the comparison costs nothing)
            _same(got, plain, label)
    return batch, plain


def _ids(cases):
    return ['%d-%d-%d-x%d-%dit' % c[:5] for c in cases]


# ---- B: the throughput chain ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.throughput_cases(), ids=_ids(C.throughput_cases()))
def test_throughput_chain_is_bitwise_the_plain_call(case):
    V, W0, H0 = C.throughput_problem(case)
    batch, (W, H) = _run_calls(case, C.THROUGHPUT_KEYS, V, W0, H0)
    assert sum(c.compared for c in case.calls) >= 4
    if case.oracle:
        # the reference side of the comparisons above, anchored: the plain call against the oracle on the files that start from ITS initial factors
        for b in (0, case.B - 1):
            Wr, Hr = O.performKLNMF(V[b], case.K, case.iterations, case.alpha, C.EPS, b)
            dW, dH = _rel(W[b, :case.F, :case.K].cpu().numpy(), Wr), _rel(H[b, :case.K, :case.N].cpu().numpy(), Hr)
            print('(%d, %d, %d) x %d file %d against performKLNMF: rel W %.3g, H %.3g' % (case.F, case.N, case.K, case.B, b, dW, dH))
            assert dW < 1e-4 and dH < 1e-4


# ---- C: the short-dictionary chain ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.short_cases(), ids=_ids(C.short_cases()))
def test_short_chain_is_bitwise_the_plain_call_at_any_batch(case):
    V, W0, H0 = C.problem(case.F, case.N, case.K, case.B, case.iterations)
    _run_calls(case, C.SHORT_KEYS, V, W0, H0)
    refused = (case.F, case.N, case.K, case.B) == C.SHORT_REFUSED
    assert all(bool(c.plan & C.CHAINED) != refused for c in case.calls[1:])


# ---- D: the ragged batch -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,K', C.RAGGED_FK)
@pytest.mark.parametrize('lengths', C.RAGGED_LENGTHS, ids=['16-files', '9-files'])
def test_ragged_batch_is_bitwise_the_uniform_plain_batches(F, K, lengths):
    files, by_length = C.ragged_problem(F, K, lengths)
    B, Nmax, iterations, alpha = len(lengths), C.RAGGED_NMAX, C.RAGGED_ITERATIONS, float(S.ALPHA)
    Fp, Kp, Np = _up(F, 16), _up(K, 64), _up(Nmax, 64)
    label = 'ragged (%d, %s, %d)' % (F, lengths, K)
    dV, W, H = _padded([f[0] for f in files], Fp, Np), _padded([f[1] for f in files], Fp, Kp), _padded([f[2] for f in files], Kp, Np)
    with _tuning(C.RAGGED_KEYS) as lib:
        n_ws = lib.gccnmf_klnmf_ragged_workspace_floats(F, Nmax, K, B)
        assert n_ws > 0 and n_ws % 4 == 0
        ws = _arbitrary_bits(n_ws, B)
        assert ws.numel() == lib.gccnmf_klnmf_ragged_workspace_floats(F, Nmax, K, B)
        rc = lib.gccnmf_klnmf_ragged(dV.data_ptr(), W.data_ptr(), H.data_ptr(), ws.data_ptr(), F, (ctypes.c_int * B)(*lengths), Nmax, K, B, iterations,
                                     alpha, C.EPS, 0, _stream())
        assert rc == 0, '%s: gccnmf_klnmf_ragged returned %d' % (label, rc)
        torch.cuda.synchronize()
        st = ctypes.c_int(-1)
        assert lib.gccnmf_klnmf_chain_status(ws.data_ptr(), F, Nmax, K, B, ctypes.byref(st)) == 0 and st.value == 0, '%s: chain status %d' % (label, st.value)
    _check_factors(W, H, F, lengths, K, label)
    for n, idx in by_length.items():
        uniform = Batch([files[f][0] for f in idx], [files[f][1] for f in idx], [files[f][2] for f in idx], K)
        with _tuning(C.RAGGED_KEYS, {21: 0}) as lib:
            assert lib.gccnmf_klnmf_plan(F, n, K, len(idx), 0) & 15 == 0
            Wu, Hu = uniform.call(lib, iterations, alpha, '%s: the uniform batch of length %d' % (label, n))
        for b, f in enumerate(idx):
            _same((W[f], H[f, :, :n]), (Wu[b], Hu[b, :, :n]), '%s: file %d of length %d' % (label, f, n))
