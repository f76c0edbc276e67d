"""KL-NMF coefficients against a fixed, pre-trained dictionary (gccnmf_klnmf with GCCNMF_FLAG_FIXED_W, csrc/nmf_fixed.hip).

The references are float64 / NumPy restatements of performKLNMF's H update (gccNMF/gccNMFFunctions.py:76) with W never updated."""
import numpy as np
import pytest
import torch

import gcc_checks as C
from oracle.rt_oracle import make_rt_dictionary

pytestmark = pytest.mark.gpu

FIXED_W, H_ONES = 1 << 16, 1 << 17


def _lib():
    from gcc_nmf_amd import _hip
    return _hip.lib()


def _geom(F, N, K):
    Fp, Kp, Np = -(-F // 16) * 16, -(-K // 64) * 64, -(-N // 64) * 64
    return Fp, Kp, Np


def _run(V, W, H0, iters, alpha=0.0, eps=1e-16, ones=False, nan_fill=True):
    """V (B, F, N), W (F, K), H0 (B, K, N) or None (ones) -> H (B, Kp, Np) full padded result, W after the call (Fp, Kp)."""
    lib = _lib()
    B, F, N = V.shape
    K = W.shape[1]
    Fp, Kp, Np = _geom(F, N, K)
    dev = 'cuda'
    Vd = torch.zeros((B, Fp, Np), dtype=torch.float32, device=dev)
    Vd[:, :F, :N] = torch.from_numpy(V).to(dev)
    Wd = torch.zeros((Fp, Kp), dtype=torch.float32, device=dev)
    Wd[:F, :K] = torch.from_numpy(W).to(dev)
    Hd = torch.full((B, Kp, Np), float('nan') if nan_fill else 0.0, dtype=torch.float32, device=dev)
    if H0 is not None:
        Hd[:, :K, :N] = torch.from_numpy(H0).to(dev)
    ws = torch.full((lib.gccnmf_klnmf_workspace_floats(F, N, K, B),), float('nan'), dtype=torch.float32, device=dev)
    flags = FIXED_W | (H_ONES if ones else 0)
    rc = lib.gccnmf_klnmf(Vd.data_ptr(), Wd.data_ptr(), Hd.data_ptr(), ws.data_ptr(), F, N, K, B, iters, alpha, eps, flags,
                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    import ctypes
    st = ctypes.c_int(-1)
    assert lib.gccnmf_klnmf_chain_status(ws.data_ptr(), F, N, K, B, ctypes.byref(st)) == 0
    assert st.value == 0
    return Hd.cpu().numpy(), Wd.cpu().numpy()


def _inputs(B, F, N, K, seed):
    rng = np.random.RandomState(seed)
    V = (rng.rand(B, F, N).astype(np.float32) + np.float32(0.01))
    W = make_rt_dictionary(seed + 1, F, K)
    H0 = rng.rand(B, K, N).astype(np.float32) + np.float32(0.01)
    V[:, -1, :] *= 100          # a dropped tail row / atom shows
    W[-1, :] *= 100
    W[:, -1] *= 100
    return V, W, H0


def _one_iteration_f64(V, W, H, alpha, eps):
    V, W, H = V.astype(np.float64), W.astype(np.float64), H.astype(np.float64)
    P = W @ H
    R = V / P
    U = W.T @ R
    den = (W.astype(np.float32).sum(0).astype(np.float64) + alpha + eps)[:, None]
    return H * U / den, R


SHAPES = [(129, 1, 1, 1), (129, 64, 77, 3), (257, 96, 1244, 1), (513, 128, 77, 3), (513, 200, 1244, 1), (2049, 1024, 77, 1),
          (257, 1024, 1, 1), (129, 200, 77, 64)]


@pytest.mark.parametrize('F,K,N,B', SHAPES)
def test_one_iteration_elementwise(F, K, N, B):
    V, W, H0 = _inputs(B, F, N, K, F + K + N)
    Hd, Wout = _run(V, W, H0, 1, alpha=0.1)
    Fp, Kp, Np = _geom(F, N, K)
    for b in range(B):
        ref, R = _one_iteration_f64(V[b], W, H0[b], 0.1, 1e-16)
        # bound: the P error (F x K products) carried through R, plus the U reduction over F
        P_abs = W.astype(np.float64) @ H0[b].astype(np.float64)
        relP = C.gemm_bound(P_abs, K) / P_abs + 2 ** -23
        absU = W.T.astype(np.float64) @ (np.abs(R) * (1 + relP))
        bound = H0[b] * (C.gemm_bound(absU, F) + W.T.astype(np.float64) @ (np.abs(R) * relP)) / \
            (W.astype(np.float32).sum(0).astype(np.float64) + 0.1)[:, None] + 4 * 2 ** -24 * np.abs(ref)
        got = Hd[b, :K, :N].astype(np.float64)
        assert np.isfinite(got).all()
        assert (np.abs(got - ref) <= bound * 2).all(), np.abs(got - ref).max()
        C.check_zero(Hd[b, K:, :], 'H padding rows')
        C.check_zero(Hd[b, :, N:], 'H padding columns')
    assert np.array_equal(Wout[:F, :K], W)


def _numpy_fixed(V, W, H, iters, alpha, eps=1e-16):
    H = H.copy()
    for _ in range(iters):
        H *= np.dot(W.T, V / np.dot(W, H)) / (np.sum(W, axis=0)[:, np.newaxis] + alpha + eps)
    return H


@pytest.mark.parametrize('alpha', [0.0, 0.1])
@pytest.mark.parametrize('init', ['random', 'ones'])
def test_hundred_iterations_against_numpy(alpha, init):
    from gcc_nmf_amd.engine import klnmf_initial_factors
    F, K, N, B = 513, 128, 1244, 2
    rng = np.random.RandomState(5)
    V = rng.rand(B, F, N).astype(np.float32) + np.float32(0.01)
    W = make_rt_dictionary(3, F, K)
    H0 = klnmf_initial_factors(F, N, K)[1] if init == 'random' else np.ones((K, N), np.float32)
    Hd, Wout = _run(V, W, None if init == 'ones' else np.broadcast_to(H0, (B, K, N)).copy(), 100, alpha=alpha, ones=init == 'ones')
    assert np.array_equal(Wout[:F, :K], W), 'W changed'
    for b in range(B):
        ref = _numpy_fixed(V[b], W, H0, 100, alpha)
        assert np.abs(Hd[b, :K, :N] - ref).max() <= 1e-4 * np.abs(ref).max()


def test_descent():
    F, K, N, B = 257, 64, 500, 2
    V, W, H0 = _inputs(B, F, N, K, 11)
    prev = None
    for it in [0, 1, 2, 5, 20, 100]:
        Hd, _ = _run(V, W, H0, it)
        H = Hd[:, :K, :N].astype(np.float64)
        WH = np.einsum('fk,bkn->bfn', W.astype(np.float64), H)
        Vd = V.astype(np.float64)
        D = (Vd * np.log(Vd / WH) - Vd + WH).sum()
        if prev is not None:
            assert D <= prev * (1 + 1e-6), (it, D, prev)
        prev = D


def test_bitwise_batch_independence():
    F, K, N, B = 513, 1024, 1244, 64
    V, W, H0 = _inputs(B, F, N, K, 21)
    whole, _ = _run(V, W, H0, 3)
    alone, _ = _run(V[37:38], W, H0[37:38], 3)
    assert np.array_equal(whole[37], alone[0])
    perm = np.random.RandomState(0).permutation(B)
    permuted, _ = _run(V[perm], W, H0[perm], 3)
    assert np.array_equal(permuted, whole[perm])


@pytest.mark.parametrize('K', [128, 1024])
def test_engine_with_dictionary_on_dev1(dev1, K):
    from gcc_nmf_amd.engine import GCCNMFEngine, inferKLNMFCoefficients
    x, sr = dev1
    x = np.asarray(x, np.float32)
    W = make_rt_dictionary(7, 513, K)
    blind = GCCNMFEngine(x.shape[-1], sampleRate=sr, dictionarySize=K, numIterations=2)
    fixed = GCCNMFEngine(x.shape[-1], sampleRate=sr, dictionaryW=W, numIterations=100)
    yb = blind.separate(x)
    y = fixed.separate(x)
    assert not fixed.chain_failed()
    assert np.array_equal(blind.get_tdoa_indexes(), fixed.get_tdoa_indexes())
    Wg, Hg = fixed.get_WH()
    assert np.array_equal(Wg[0], W)
    V = fixed.get_V()
    assert np.array_equal(Hg[0], inferKLNMFCoefficients(V[0], W, 100))
    assert np.isfinite(y).all() and y.shape == yb.shape
    y2 = list(fixed.separate_batches([x[None], x[None]]))
    assert np.array_equal(y2[0], y) and np.array_equal(y2[1], y)
    pcm = (np.clip(x.T, -1, 1) * 32767).astype(np.int16)
    out = fixed.separate_pcm16(pcm)
    assert out.shape[:2] == (1, fixed.g.S)


def test_ragged_with_dictionary():
    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_mixture
    W = make_rt_dictionary(9, 513, 128)
    lengths = [16000, 24000, 16000, 40000]
    xs = [synthetic_mixture(i, n) for i, n in enumerate(lengths)]
    rag = GCCNMFEngine(lengths=lengths, dictionaryW=W, numIterations=20)
    out = rag.separate(xs)
    for n in sorted(set(lengths)):
        idx = [i for i, m in enumerate(lengths) if m == n]
        e = GCCNMFEngine(n, batch=len(idx), dictionaryW=W, numIterations=20)
        y = e.separate(np.stack([xs[i] for i in idx]))
        for k, i in enumerate(idx):
            assert np.array_equal(out[i], y[k])


# ---- the fused launch element by element, at every wave shape (tests/fixed_dictionary_restatement.py derives the bars and the table) ------------
# Through the C ABI, on a workspace and an H padding pre-filled with NaN.  Every comparison prints its worst share of the bar before it
# asserts; every call is held to the ownership rules (Call).
import ctypes                                      # noqa: E402
import functools                                   # noqa: E402

import fixed_dictionary_restatement as R           # noqa: E402
import klnmf_stages_restatement as S               # noqa: E402

ALPHA, EPS = float(S.ALPHA), float(S.EPS)
POOL = 5                                           # files per shape; a case takes the first `files` of them, or those it picks
STATUS_WORDS = 32                                  # the chain-status words: the last 32 floats of the workspace


@functools.lru_cache(maxsize=None)
def _problem(F, N, K, frame=False):
    return R.problem(F, N, K, POOL, frame)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Call(object):
    """One gccnmf_klnmf(..., GCCNMF_FLAG_FIXED_W [| GCCNMF_FLAG_H_ONES]) of V (B, F, N), W (F, K), H0 (B, K, N) or None.  On entry V and W are
    zero padded, the padding of H (H0 None: all of H) and the whole workspace hold NaN.  Checked on every call: V and all of W bit for bit
    unchanged; every workspace float behind the documented head den [Kp] | Wt [Kp][round_up(F, 32)] still its NaN bits, but for the
    chain-status words, which are cleared and report 0; the padding of H (rows >= K, columns >= N, up to Kp x Np) bit for bit +0."""

    def __init__(self, V, W, H0, iterations, alpha=ALPHA, eps=EPS, ones=False, label=''):
        lib = _lib()
        B, F, N = V.shape
        K = W.shape[1]
        Fp, Kp, Np = _geom(F, N, K)
        Fq = -(-F // 32) * 32
        self.shape, self.label = (B, F, N, K, Kp, Fq), label
        Vd = torch.zeros((B, Fp, Np), dtype=torch.float32, device='cuda')
        Vd[:, :F, :N] = torch.from_numpy(np.array(V)).cuda()
        Wd = torch.zeros((Fp, Kp), dtype=torch.float32, device='cuda')
        Wd[:F, :K] = torch.from_numpy(np.array(W)).cuda()
        Hd = torch.full((B, Kp, Np), float('nan'), dtype=torch.float32, device='cuda')
        if H0 is not None:
            Hd[:, :K, :N] = torch.from_numpy(np.array(H0, dtype=np.float32)).cuda()
        floats = lib.gccnmf_klnmf_workspace_floats(F, N, K, B)
        ws = torch.full((floats,), float('nan'), dtype=torch.float32, device='cuda')
        V_in, W_in, ws_in = Vd.cpu().numpy(), Wd.cpu().numpy(), ws.cpu().numpy()
        assert np.isnan(ws_in).all()
        rc = lib.gccnmf_klnmf(Vd.data_ptr(), Wd.data_ptr(), Hd.data_ptr(), ws.data_ptr(), F, N, K, B, iterations, alpha, eps,
                              R.FIXED_W | (R.H_ONES if ones else 0), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, '%s: gccnmf_klnmf returned %d' % (label, rc)
        torch.cuda.synchronize()
        st = ctypes.c_int(-1)
        assert lib.gccnmf_klnmf_chain_status(ws.data_ptr(), F, N, K, B, ctypes.byref(st)) == 0 and st.value == 0, label
        self.Hfull, self.ws = Hd.cpu().numpy(), ws.cpu().numpy()
        self.H = self.Hfull[:, :K, :N]
        assert np.array_equal(_bits(Vd.cpu().numpy()), _bits(V_in)), '%s: V changed' % label
        assert np.array_equal(_bits(Wd.cpu().numpy()), _bits(W_in)), '%s: W changed' % label
        head = Kp * (1 + Fq)
        assert head <= floats - STATUS_WORDS
        same = _bits(self.ws[head:floats - STATUS_WORDS]) == _bits(ws_in[head:floats - STATUS_WORDS])
        assert same.all(), '%s: workspace float %d behind the head was written' % (label, head + int(np.argwhere(~same)[0, 0]))
        assert not _bits(self.ws[floats - STATUS_WORDS:]).any(), '%s: the chain-status words are not cleared' % label
        assert not _bits(self.Hfull[:, K:, :]).any() and not _bits(self.Hfull[:, :, N:]).any(), '%s: the padding of H is not +0' % label

    def check_head(self, W, alpha, eps):
        """den [Kp] | Wt [Kp][round_up(F, 32)] at the start of the workspace -> worst share of den's bar"""
        B, F, N, K, Kp, Fq = self.shape
        den, Wt = self.ws[:Kp], self.ws[Kp:Kp * (1 + Fq)].reshape(Kp, Fq)
        ref_den, ref_Wt = R.prepare(W, np.float32(alpha), np.float32(eps))
        worst, miss = S.share(den[:K], ref_den, R.bar_den(F))
        print('%s: den: worst share of the bar (%.0f * 2^-24) %.3f' % (self.label, R.bar_den(F) / S.U24, worst))
        assert miss is None, '%s: den%s is %r, reference %r' % (self.label, miss, den[miss], ref_den[miss])
        assert (den[K:] == 1).all(), '%s: den of a padding atom is not 1' % self.label
        assert np.array_equal(_bits(Wt[:K, :F]), _bits(ref_Wt)), '%s: Wt is not W^T bit for bit' % self.label
        assert not _bits(Wt[K:, :]).any() and not _bits(Wt[:, F:]).any(), '%s: Wt is not +0 outside F x K' % self.label
        return worst


def _label(F, K, N, files, what):
    return '(F, K, N) = (%d, %d, %d) x %d, KB = %d, nw = %d, %s' % ((F, K, N, files) + R.fixed_shape(K)[1:] + (what,))


@pytest.mark.parametrize('F,K,N,files', R.SHAPES)
def test_one_iteration_against_the_restatement(F, K, N, files):
    _, W, H0 = _problem(F, N, K)
    H0 = H0[:files]
    dead, bar = R.dead_atom(K), R.bar_iteration(F, K)
    for alpha, frame in ((ALPHA, False), (0.0, False), (ALPHA, True)):
        V = _problem(F, N, K, frame)[0][:files]
        label = _label(F, K, N, files, 'alpha = %g%s' % (alpha, ', a silent frame' if frame else ''))
        c = Call(V, W, H0, 1, alpha, label=label)
        assert np.isfinite(c.H).all(), label
        worst, misses = 0.0, []
        for b in range(files):
            ref = R.iteration(V[b], W, H0[b], np.float32(alpha), S.EPS)
            w, miss = S.share(c.H[b], ref, bar)
            worst = max(worst, w)
            if miss is not None:
                misses.append('file %d element %s: %r, reference %r' % (b, miss, c.H[b][miss], ref[miss]))
            # the exact zeros the reference holds: the dead atom, the zeros of H0, the silent frame
            if dead is not None:
                assert not ref[dead].any() and not c.H[b, dead].any(), label
            for k, n in R.h_zeros(K, N, b):
                assert ref[k, n] == 0 and c.H[b, k, n] == 0, label
            n0 = S.zero_lines(F, N, b)[1]
            if frame and n0 is not None:
                assert not ref[:, n0].any() and not c.H[b, :, n0].any(), label
        print('%s: H: worst share of the bar (%.0f * 2^-24) %.3f' % (label, bar / S.U24, worst))
        assert not misses, '%s: H misses its bar of %.0f * 2^-24 relative: %s' % (label, bar / S.U24, '; '.join(misses[:4]))
        c.check_head(W, alpha, EPS)


@pytest.mark.parametrize('F,K,N,files', R.SHAPES)
def test_three_iterations_in_one_call_are_three_calls(F, K, N, files):
    """the prefetch's wrap to chunk 0 of the next iteration, the LDS buffer toggle across iterations, the register-resident H"""
    V, W, H0 = _problem(F, N, K)
    V, H0 = V[:files], H0[:files]
    label = _label(F, K, N, files, 'three iterations')
    one = Call(V, W, H0, 3, label=label)
    H, bar, worst = H0, R.bar_iteration(F, K), 0.0
    for it in range(3):
        step = Call(V, W, H, 1, label=label)
        for b in range(files):                                               # every one of the three against the restatement from ITS input
            w, miss = S.share(step.H[b], R.iteration(V[b], W, H[b]), bar)
            worst = max(worst, w)
            assert miss is None, '%s: call %d, file %d element %s misses its bar' % (label, it, b, miss)
        H = step.H
    print('%s: H of each of the three calls: worst share of the bar (%.0f * 2^-24) %.3f' % (label, bar / S.U24, worst))
    assert np.isfinite(one.H).all() and not np.array_equal(_bits(one.H), _bits(H0)), label
    assert np.array_equal(_bits(one.Hfull), _bits(step.Hfull)), '%s: one call of 3 iterations differs from 3 calls of one' % label


@pytest.mark.parametrize('F,K,N,files', R.SHAPES)
def test_zero_iterations(F, K, N, files):
    V, W, H0 = _problem(F, N, K)
    V, H0 = V[:files], H0[:files]
    label = _label(F, K, N, files, 'no iteration')
    c = Call(V, W, H0, 0, label=label)                                       # (Call: the padding, NaN on entry, is +0)
    assert np.array_equal(_bits(c.H), _bits(H0)), '%s: H changed' % label
    c = Call(V, W, None, 0, ones=True, label=label)
    assert np.array_equal(_bits(c.H), _bits(np.ones_like(H0))), '%s: H is not all ones' % label


@pytest.mark.parametrize('F,K,N,files', R.SHAPES)
def test_h_ones_is_an_explicit_all_ones_start(F, K, N, files):
    V, W, H0 = _problem(F, N, K)
    V = V[:files]
    for iterations in (1, 3):
        label = _label(F, K, N, files, 'H_ONES, %d iterations' % iterations)
        flag = Call(V, W, None, iterations, ones=True, label=label)          # H is NaN throughout on entry: it is not read
        explicit = Call(V, W, np.ones_like(H0[:files]), iterations, label=label)
        assert np.isfinite(flag.H).all(), label
        assert np.array_equal(_bits(flag.Hfull), _bits(explicit.Hfull)), label


BATCH_SHAPES = [s for s in R.SHAPES if s[3] >= 2 and R.fixed_shape(s[1])[1] >= 2]


@pytest.mark.parametrize('F,K,N,files', BATCH_SHAPES)
def test_a_file_has_the_same_bits_alone_in_its_batch_and_in_a_permuted_batch_of_five(F, K, N, files):
    V, W, H0 = _problem(F, N, K)
    label = _label(F, K, N, files, 'batch independence')
    batch = Call(V[:files], W, H0[:files], 3, label=label)
    perm = [4, 2, 3, 0, 1]
    five = Call(V[perm], W, H0[perm], 3, label=label)
    assert np.isfinite(five.H).all(), label
    for b in range(files):
        alone = Call(V[b:b + 1], W, H0[b:b + 1], 3, label=label)
        assert np.array_equal(_bits(alone.Hfull[0]), _bits(batch.Hfull[b])), '%s: file %d alone' % (label, b)
        assert np.array_equal(_bits(five.Hfull[perm.index(b)]), _bits(batch.Hfull[b])), '%s: file %d in the batch of five' % (label, b)


def test_the_batch_independence_cases_cover_kb_2_3_and_4():
    assert {R.fixed_shape(K)[1] for _, K, _, _ in BATCH_SHAPES} == {2, 3, 4}


@pytest.mark.parametrize('F,K,N,files', [(64, 300, 70, 2), (65, 516, 40, 2)])
def test_inferKLNMFCoefficients_is_the_c_abi_call(F, K, N, files):
    from gcc_nmf_amd.engine import inferKLNMFCoefficients, klnmf_initial_factors
    assert (F, K, N, files) in R.SHAPES and R.fixed_shape(K)[1] == (2 if K == 300 else 3)
    V, W, _ = _problem(F, N, K)
    V = V[:files]
    H = inferKLNMFCoefficients(np.array(V), np.array(W), 3)          # (copies: the pool is read-only)
    H0 = np.broadcast_to(klnmf_initial_factors(F, N, K)[1], (files, K, N))
    c = Call(V, W, H0, 3, alpha=0.0, eps=1e-16, label=_label(F, K, N, files, 'inferKLNMFCoefficients'))
    assert H.dtype == np.float32 and H.shape == (files, K, N) and np.isfinite(H).all()
    assert np.array_equal(_bits(H), _bits(c.H))
