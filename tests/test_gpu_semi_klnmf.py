"""Semi-supervised KL-NMF on the device (GCCNMF_FLAG_FREE_ATOMS, csrc/nmf_semi.hip): free atoms learned beside a pre-trained dictionary.

  * stage 4 (U_free = R . H_free^T, rowsumH_free) and stage 5 (the free columns' W update) of gccnmf_klnmf_stage, element by element
    against the float64 restatement (tests/semi_klnmf_restatement.py) evaluated on the float32 values the device held before the stage, with
    the derived bars of tests/klnmf_stages_restatement.py -- at every shape of the table.  The workspace is NaN wherever it is not an input:
    whatever belongs to a fixed atom, and every other word, must keep its bits;
  * a file's stage results are bit for bit the same alone and as file 2 of a batch of 3 and of 9;
  * one whole iteration through gccnmf_klnmf against the restatement (bars compounded from the stage bars: iteration_bars);
  * a blind call gives identical factors before and after a semi-supervised call in the same process, on the same workspace;
  * 100 iterations against float32 NumPy; descent of the divergence; the engine on the committed dev1 mixture.

Every check prints its figure before it asserts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gcc_checks as C
import klnmf_stages_restatement as S
import semi_klnmf_restatement as M
from oracle.rt_oracle import make_rt_dictionary
from test_gpu_klnmf_stages import Layout, _bits

pytestmark = pytest.mark.gpu

NAN = float('nan')


def _lib():
    from gcc_nmf_amd import _hip
    return _hip.lib()


def _pad(a, shape, fill=0.0):
    t = torch.full(shape, fill, dtype=torch.float32, device='cuda')
    t[tuple(slice(0, n) for n in a.shape)] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return t


def _stream():
    return torch.cuda.current_stream().cuda_stream


class StageRun(object):
    """Device state of one stage-4 / stage-5 experiment: V, W, H padded with zeros, the workspace all NaN but for what the test writes."""

    def __init__(self, V, W, H, Kf, n):
        self.lib = _lib()
        B, F, N = V.shape
        K = Kf + n
        self.B, self.F, self.N, self.K, self.Kf, self.n = B, F, N, K, Kf, n
        self.L = L = Layout(F, N, K, B)
        self.Vd, self.Wd, self.Hd = _pad(V, (B, L.Fp, L.Np)), _pad(W, (B, L.Fp, L.Kp)), _pad(H, (B, L.Kp, L.Np))
        self.ws = torch.full((self.lib.gccnmf_klnmf_workspace_floats(F, N, K, B),), NAN, dtype=torch.float32, device='cuda')

    def block(self, name):
        at, shape = self.L.blocks[name]
        return self.ws[at:at + int(np.prod(shape))].view(shape)

    def stage(self, stage):
        rc = self.lib.gccnmf_klnmf_stage(self.Vd.data_ptr(), self.Wd.data_ptr(), self.Hd.data_ptr(), self.ws.data_ptr(), self.F, self.N, self.K,
                                         self.B, float(S.ALPHA), float(S.EPS), M.FREE_ATOMS(self.n), stage, _stream())
        assert rc == 0, 'stage %d returned %d' % (stage, rc)
        torch.cuda.synchronize()

    def snapshot(self):
        torch.cuda.synchronize()
        ws = self.ws.cpu().numpy()
        st = dict(ws=ws, V=self.Vd.cpu().numpy(), W=self.Wd.cpu().numpy(), H=self.Hd.cpu().numpy())
        for name in ('R', 'U', 'colsumW', 'rowsumH', 's'):
            st[name] = self.L.view(ws, name)
        return st


def _within(label, got, ref, bar):
    worst, miss = S.share(got, ref, bar)
    print('%s: worst share of the bar (%.1f * 2^-24) %.3f' % (label, bar / S.U24, worst))
    assert miss is None, '%s misses its bar of %.1f * 2^-24 relative at %s: %r, reference %r' % (label, bar / S.U24, miss, np.asarray(got)[miss], np.asarray(ref)[miss])


def _same_outside(label, was, now, name, owned):
    """block `name` of two snapshots: bit for bit the same wherever `owned` (a boolean mask of the block) is False"""
    diff = (_bits(was[name]) != _bits(now[name])) & ~owned
    assert not diff.any(), '%s changed %s at %s, which it does not own' % (label, name, tuple(np.argwhere(diff)[0]))


def _stages_4_and_5(V, W, H, Kf, n, label, b0=0):
    """-> the snapshot after stage 5 (and, under 'after4', after stage 4), every check of the module's docstring done on the way.
    b0: the index the first file has in its problem (its silent bin follows from it)"""
    B, F, N = V.shape
    K = Kf + n
    run = StageRun(V, W, H, Kf, n)
    L = run.L
    # the float32 R a stage 3 leaves: zero padded, the silent bin and frame exactly zero
    R = np.stack([np.asarray(S.stage3(V[b], W[b], H[b]), np.float32) for b in range(B)])
    run.block('R').copy_(_pad(R, (B, L.Fp, L.Np)))
    rng = np.random.RandomState(F + N + K)
    colsum0, s0 = (rng.rand(B, L.Kp) + 0.5).astype(np.float32), (0.5 + 1.5 * rng.rand(B, L.Kp)).astype(np.float32)
    run.block('colsumW').copy_(torch.from_numpy(colsum0).cuda())
    run.block('s').copy_(torch.from_numpy(s0).cuda())
    was = run.snapshot()

    run.stage(4)
    now = run.snapshot()
    free_U = np.zeros((B, L.Fp, L.Kp), bool)
    free_U[:, :F, Kf:K] = True
    free_vec = np.zeros((B, L.Kp), bool)
    free_vec[:, Kf:K] = True
    for name in ('V', 'W', 'H', 'R', 'colsumW', 's'):
        _same_outside(label + ' stage 4', was, now, name, np.zeros(was[name].shape, bool))
    _same_outside(label + ' stage 4', was, now, 'U', free_U)
    _same_outside(label + ' stage 4', was, now, 'rowsumH', free_vec)
    assert np.array_equal(_bits(was['ws'][L.blocks['s'][0] + B * L.Kp:]), _bits(now['ws'][L.blocks['s'][0] + B * L.Kp:])), label + ': stage 4 wrote behind the K-vectors'
    for b in range(B):
        U, rs = M.stage4_free(R[b], H[b], n)
        _within('%s file %d stage 4 U_free' % (label, b), now['U'][b, :F, Kf:K], U, S.bar_U(N))
        _within('%s file %d stage 4 rowsumH_free' % (label, b), now['rowsumH'][b, Kf:K], rs, S.bar_rowsumH(N))
        assert not _bits(now['U'][b, S.zero_lines(F, N, b0 + b)[0], Kf:K]).any(), label + ': the silent bin of U_free is not exactly zero'
    after4 = now

    run.stage(5)
    was, now = now, run.snapshot()
    for name in ('V', 'H', 'R', 'U', 'rowsumH'):
        _same_outside(label + ' stage 5', was, now, name, np.zeros(was[name].shape, bool))
    _same_outside(label + ' stage 5', was, now, 'W', free_U)
    _same_outside(label + ' stage 5', was, now, 'colsumW', free_vec)
    _same_outside(label + ' stage 5', was, now, 's', free_vec)
    assert np.array_equal(_bits(was['ws'][L.blocks['s'][0] + B * L.Kp:]), _bits(now['ws'][L.blocks['s'][0] + B * L.Kp:])), label + ': stage 5 wrote behind the K-vectors'
    assert not _bits(now['W'][:, F:, :]).any() and not _bits(now['W'][:, :, K:]).any(), label + ': stage 5 left non-zero padding in W'
    for b in range(B):
        Wn, s, cs = M.stage5_free(W[b], was['U'][b, :F, Kf:K], was['rowsumH'][b, Kf:K], n)
        _within('%s file %d stage 5 W_free' % (label, b), now['W'][b, :F, Kf:K], Wn, S.bar_W(F))
        _within('%s file %d stage 5 s_free' % (label, b), now['s'][b, Kf:K], s, S.bar_s(F))
        _within('%s file %d stage 5 colsumW_free' % (label, b), now['colsumW'][b, Kf:K], cs, S.bar_colsumW(F))
    now['after4'] = after4
    return now


@pytest.mark.parametrize('F,N,Kf,n,B', M.SHAPES)
def test_stage_4_and_stage_5_elementwise(F, N, Kf, n, B):
    assert _lib().gccnmf_klnmf_plan(F, N, Kf + n, B, M.FREE_ATOMS(n)) == 32
    V, W, H, _ = M.problem(F, N, Kf, n, max(B, 2))
    _stages_4_and_5(V[:B], W[:B], H[:B], Kf, n, '(%d, %d, %d + %d) x %d' % (F, N, Kf, n, B))


@pytest.mark.parametrize('F,N,Kf,n', [(513, 130, 128, 16), (40, 65, 16, 33), (641, 96, 64, 128)])
def test_a_file_does_not_depend_on_its_batch(F, N, Kf, n):
    """the same R and H for one file alone and as file 2 of a batch of 3 and of 9"""
    V, W, H, _ = M.problem(F, N, Kf, n, 9)
    K = Kf + n
    alone = _stages_4_and_5(V[2:3], W[2:3], H[2:3], Kf, n, 'alone', b0=2)
    for B in (3, 9):
        many = _stages_4_and_5(V[:B], W[:B], H[:B], Kf, n, 'file 2 of %d' % B)
        # (s and colsumW hold the test's own stand-in values until stage 5 writes them: compared after stage 5 only)
        for st_a, st_m, names in ((alone['after4'], many['after4'], ('U', 'rowsumH')), (alone, many, ('U', 'rowsumH', 'W', 's', 'colsumW'))):
            idx = dict(U=(slice(0, F), slice(Kf, K)), rowsumH=(slice(Kf, K),), W=(slice(0, F), slice(0, K)), s=(slice(Kf, K),), colsumW=(slice(Kf, K),))
            for name in names:
                assert np.array_equal(_bits(st_a[name][0][idx[name]]), _bits(st_m[name][2][idx[name]])), '%s of file 2 depends on the batch of %d' % (name, B)


def _klnmf(V, W, H, iterations, flags, alpha=float(S.ALPHA), eps=float(S.EPS), ws=None):
    """gccnmf_klnmf on padded copies: V (B, F, N), W (B, F, K), H (B, K, N) -> padded W, H after the call, the workspace, the chain status"""
    lib = _lib()
    B, F, N = V.shape
    K = W.shape[2]
    L = Layout(F, N, K, B)
    Vd, Wd, Hd = _pad(V, (B, L.Fp, L.Np)), _pad(W, (B, L.Fp, L.Kp)), _pad(H, (B, L.Kp, L.Np))
    if ws is None:
        ws = torch.full((lib.gccnmf_klnmf_workspace_floats(F, N, K, B),), NAN, dtype=torch.float32, device='cuda')
    rc = lib.gccnmf_klnmf(Vd.data_ptr(), Wd.data_ptr(), Hd.data_ptr(), ws.data_ptr(), F, N, K, B, iterations, alpha, eps, flags, _stream())
    assert rc == 0, 'gccnmf_klnmf returned %d' % rc
    torch.cuda.synchronize()
    st = ctypes.c_int(-1)
    assert lib.gccnmf_klnmf_chain_status(ws.data_ptr(), F, N, K, B, ctypes.byref(st)) == 0
    return Wd.cpu().numpy(), Hd.cpu().numpy(), ws, st.value


@pytest.mark.parametrize('F,N,Kf,n,B', M.SHAPES)
def test_one_iteration_against_the_restatement(F, N, Kf, n, B):
    K = Kf + n
    V, W, H, _ = M.problem(F, N, Kf, n, max(B, 2), silent_frame=False)
    V, W, H = V[:B], W[:B], H[:B]
    Wg, Hg, _, status = _klnmf(V, W, H, 1, M.FREE_ATOMS(n))
    assert status == 0
    bars = M.iteration_bars(F, N, K)
    label = '(%d, %d, %d + %d) x %d' % (F, N, Kf, n, B)
    for b in range(B):
        assert np.array_equal(_bits(Wg[b, :F, :Kf]), _bits(W[b][:, :Kf])), '%s: the dictionary of file %d changed' % (label, b)
        Wr, Hr = M.iteration(V[b], W[b], H[b], n)
        _within('%s file %d W_free' % (label, b), Wg[b, :F, Kf:K], Wr[:, Kf:], bars['W_free'])
        _within('%s file %d H of the fixed atoms' % (label, b), Hg[b, :Kf, :N], Hr[:Kf], bars['H_fixed'])
        _within('%s file %d H of the free atoms' % (label, b), Hg[b, Kf:K, :N], Hr[Kf:], bars['H_free'])
        assert not _bits(Wg[b, S.zero_lines(F, N, b)[0], Kf:K]).any(), label + ': the silent bin of W_free is not exactly zero'
    C.check_zero(Hg[:, K:, :], 'padding atoms of H')
    C.check_zero(Hg[:, :, N:], 'padding columns of H')
    C.check_zero(Wg[:, F:, :], 'padding rows of W')
    C.check_zero(Wg[:, :, K:], 'padding atoms of W')


@pytest.mark.parametrize('F,N,K,n,B', [(513, 65, 80, 16, 2), (513, 130, 144, 16, 9), (129, 70, 48, 16, 5)])
def test_a_blind_call_is_not_disturbed(F, N, K, n, B):
    """the same blind call -- same inputs, same workspace -- before and after a semi-supervised call in this process: identical W and H"""
    V, W, H, _ = M.problem(F, N, K - n, n, B, silent_frame=False)
    plan = _lib().gccnmf_klnmf_plan(F, N, K, B, 0)
    W1, H1, ws, st1 = _klnmf(V, W, H, 3, 0)
    Ws, Hs, ws, sts = _klnmf(V, W, H, 3, M.FREE_ATOMS(n), ws=ws)
    W2, H2, ws, st2 = _klnmf(V, W, H, 3, 0, ws=ws)
    assert st1 == sts == st2 == 0 and _lib().gccnmf_klnmf_plan(F, N, K, B, 0) == plan
    assert np.array_equal(_bits(W1), _bits(W2)) and np.array_equal(_bits(H1), _bits(H2))
    assert np.array_equal(_bits(Ws[:, :F, :K - n]), _bits(W[:, :, :K - n])) and not np.array_equal(Ws, W1)


# ---- 100 iterations against float32 NumPy --------------------------------------------------------------------------------------------------------
LONG = dict(F=513, N=1244, Kf=128, n=16, B=2)


@functools.lru_cache(maxsize=None)
def _long_problem():
    from gcc_nmf_amd.engine import semi_supervised_initial_factors
    from kl_divergence_restatement import low_rank_plus_noise
    F, N, Kf, n, B = (LONG[k] for k in ('F', 'N', 'Kf', 'n', 'B'))
    V = np.stack([low_rank_plus_noise(F, N, 12, 0.5, 40 + b, zeros=0) for b in range(B)])
    W0, H0 = semi_supervised_initial_factors(make_rt_dictionary(5, F, Kf), n, N, 1e-16, 0)
    for a in (V, W0, H0):
        a.flags.writeable = False
    return V, W0, H0


@pytest.mark.parametrize('alpha', [0.0, 0.1])
def test_100_iterations_against_float32_numpy(alpha):
    """relative Frobenius error of W_free and H below 1e-4, the project's bar for the blind call (tests/test_gpu_kernels.py).
    Measured: DESIGN section 2c."""
    V, W0, H0 = _long_problem()
    B, Kf, n = LONG['B'], LONG['Kf'], LONG['n']
    Wg, Hg, _, status = _klnmf(V, np.stack([W0] * B), np.stack([H0] * B), 100, M.FREE_ATOMS(n), alpha=alpha, eps=1e-16)
    assert status == 0
    F, N, K = LONG['F'], LONG['N'], Kf + n
    for b in range(B):
        Wr, Hr = M.run(V[b], W0, H0, n, 100, np.float32(alpha), np.float32(1e-16), np.float32)
        assert np.array_equal(_bits(Wg[b, :F, :Kf]), _bits(W0[:, :Kf]))
        eW = np.linalg.norm(Wg[b, :F, Kf:K] - Wr[:, Kf:]) / np.linalg.norm(Wr[:, Kf:])
        eH = np.linalg.norm(Hg[b, :K, :N] - Hr) / np.linalg.norm(Hr)
        print('alpha %.1f file %d: relative Frobenius error after 100 iterations: W_free %.3g, H %.3g' % (alpha, b, eW, eH))
        assert eW < 1e-4 and eH < 1e-4


def test_descent():
    F, Kf, n, N, B = 257, 64, 16, 500, 2
    rng = np.random.RandomState(11)
    V = rng.rand(B, F, N).astype(np.float32) + np.float32(0.01)
    W = np.concatenate([make_rt_dictionary(12, F, Kf), rng.rand(F, n).astype(np.float32) + np.float32(0.01)], axis=1)
    H0 = rng.rand(B, Kf + n, N).astype(np.float32) + np.float32(0.01)
    prev = None
    for it in [0, 1, 2, 5, 20, 100]:
        Wg, Hg, _, status = _klnmf(V, np.stack([W] * B), H0, it, M.FREE_ATOMS(n), alpha=0.0, eps=1e-16)
        assert status == 0
        D = sum(M.divergence(V[b], Wg[b, :F, :Kf + n], Hg[b, :Kf + n, :N]) for b in range(B))
        print('iterations %d: D = %.6f' % (it, D))
        if prev is not None:
            assert D <= prev * (1 + 1e-6), (it, D, prev)
        prev = D


def test_engine_with_free_atoms_on_dev1(dev1):
    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.gccNMFFunctions import performSemiSupervisedKLNMF
    x, sr = dev1
    x = np.asarray(x, np.float32)
    W = make_rt_dictionary(7, 513, 128)
    iters = 30
    fixed = GCCNMFEngine(x.shape[-1], sampleRate=sr, dictionaryW=W, numIterations=iters)
    semi = GCCNMFEngine(x.shape[-1], sampleRate=sr, dictionaryW=W, numFreeAtoms=16, numIterations=iters)
    fixed.separate(x)
    y = semi.separate(x)
    assert not semi.chain_failed() and semi.g.K == 144
    Wg, Hg = semi.get_WH()
    assert Wg.shape[1:] == (513, 144) and np.array_equal(Wg[0][:, :128], W)
    norms = np.linalg.norm(Wg[0][:, 128:].astype(np.float64), axis=0)
    assert np.abs(norms - 1).max() <= S.bar_W(513)            # every element of a free atom is within bar_W of the unit-norm column
    V = semi.get_V()
    Wf, Hf = performSemiSupervisedKLNMF(V[0], W, 16, iters, 0)
    assert np.array_equal(Hg[0], Hf) and np.array_equal(Wg[0], Wf)
    D_semi, D_fixed = semi.get_divergence()[0], fixed.get_divergence()[0]
    print('dev1, %d iterations: D with the dictionary alone %.1f, with 16 free atoms %.1f' % (iters, D_fixed, D_semi))
    assert D_semi < D_fixed
    assert np.isfinite(y).all() and np.isfinite(Wg).all() and np.isfinite(Hg).all()
    y2 = list(semi.separate_batches([x[None], x[None]]))
    assert np.array_equal(y2[0], y) and np.array_equal(y2[1], y)
    out = semi.separate_pcm16((np.clip(x.T, -1, 1) * 32767).astype(np.int16))
    assert out.shape[:2] == (1, semi.g.S)
    stop = GCCNMFEngine(x.shape[-1], sampleRate=sr, dictionaryW=W, numFreeAtoms=16, numIterations=iters, tolerance=1e-3, checkEvery=5)
    stop.separate(x)
    trace = stop.get_divergence_trace()[:, 0]
    print('tolerance 1e-3: %d iterations, trace %s' % (stop.get_iterations()[0], trace))
    assert stop.get_iterations()[0] <= iters and all(b <= a for a, b in zip(trace, trace[1:]))
    assert np.array_equal(stop.get_WH()[0][0][:, :128], W)
