"""Itakura-Saito and Euclidean NMF (gccnmf_klnmf / gccnmf_klnmf_stage with GCCNMF_FLAG_DIVERGENCE_*, csrc/nmf_beta.hip) through the C ABI
and through the Python layers.  Every stage 0-6 is compared element by element with the float64 restatement of that stage
(tests/beta_nmf_restatement.py, which derives the bars) evaluated on the float32 state the device held before it; the intermediates are
read at the offsets include/gccnmf_hip.h documents.  Every comparison prints its worst share of the bar before it asserts.

The shapes (beta_nmf_restatement.SHAPES) are the smallest at which the kernels can still go wrong: one file with N % 64 != 0; the
F % 128 == 1 tail bin with K % 64 != 0; K > 128 (two row tiles of the H update, three column tiles of R.H^T); the workload's own F."""
import functools

import numpy as np
import pytest
import torch

import beta_nmf_restatement as B
import klnmf_stages_restatement as S

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
BETAS = [B.IS, B.EUCLIDEAN]
ALPHA, EPS = float(S.ALPHA), float(S.EPS)
POOL = 5                                                    # problems per shape; a Run takes the first `files` of them, or those it picks


def _lib():
    from gcc_nmf_amd import _hip
    return _hip.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _problem(F, N, K, files):
    return B.problem(F, N, K, files)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Layout(object):
    """Where an IS / Euclidean call keeps its intermediates (include/gccnmf_hip.h, at gccnmf_klnmf_stage), in floats: the KL layout --
    R | Un | colsumW | rowsumH | s | ... -- of gccnmf_klnmf_workspace_floats floats, then Q | Ud."""

    def __init__(self, lib, F, N, K, files):
        self.F, self.N, self.K, self.B = F, N, K, files
        self.Fp, self.Kp, self.Np = -(-F // 16) * 16, -(-K // 64) * 64, -(-N // 64) * 64
        Fp, Kp, Np = self.Fp, self.Kp, self.Np
        self.kl = lib.gccnmf_klnmf_workspace_floats(F, N, K, files)
        self.floats = self.kl + files * Fp * (Np + Kp)              # GCCNMF_KLNMF_DIVERGENCE_WORKSPACE_FLOATS behind the KL layout
        self.blocks, at = {}, 0
        for name, shape in (('R', (files, Fp, Np)), ('Un', (files, Fp, Kp)), ('colsumW', (files, Kp)), ('rowsumH', (files, Kp)), ('s', (files, Kp))):
            self.blocks[name] = (at, shape)
            at += int(np.prod(shape))
        assert at <= self.kl - 32
        self.blocks['Q'] = (self.kl, (files, Fp, Np))
        self.blocks['Ud'] = (self.kl + files * Fp * Np, (files, Fp, Kp))

    def view(self, ws, name):
        at, shape = self.blocks[name]
        return ws[at:at + int(np.prod(shape))].reshape(shape)


class Run(object):
    """`files` problems on the device with zero-padded V, W, H and a workspace pre-filled with NaN."""
    NAMES = ['V', 'W', 'H', 'R', 'Q', 'Un', 'Ud', 'colsumW', 's']

    def __init__(self, F, N, K, files, beta, label, pick=None):
        self.lib, self.beta, self.label, self.flags = _lib(), beta, label, B.FLAGS[beta]
        self.L = L = Layout(self.lib, F, N, K, files)
        V, W, H, s = _problem(F, N, K, POOL)                 # (always the same pool: a file is the same problem in every batch)
        idx = list(range(files)) if pick is None else list(pick)
        self.V0, self.W0, self.H0, self.s0 = V[idx], W[idx], H[idx], s[idx]
        self.Vd, self.Wd, self.Hd = self._pad(self.V0, (files, L.Fp, L.Np)), self._pad(self.W0, (files, L.Fp, L.Kp)), self._pad(self.H0, (files, L.Kp, L.Np))
        self.ws = torch.full((L.floats,), float('nan'), dtype=torch.float32, device='cuda')
        self.state = self.snapshot()

    @staticmethod
    def _pad(a, shape):
        t = torch.zeros(shape, dtype=torch.float32, device='cuda')
        t[tuple(slice(0, n) for n in a.shape)] = torch.from_numpy(np.array(a)).cuda()
        return t

    def snapshot(self):
        torch.cuda.synchronize()
        ws = self.ws.cpu().numpy()
        st = dict(V=self.Vd.cpu().numpy(), W=self.Wd.cpu().numpy(), H=self.Hd.cpu().numpy())
        for name in self.NAMES[3:]:
            st[name] = self.L.view(ws, name)
        return st

    def poke(self, name, values):
        """overwrite the whole workspace block `name` (B, ...) on the device"""
        at, shape = self.L.blocks[name]
        self.ws[at:at + int(np.prod(shape))].view(shape)[tuple(slice(0, n) for n in np.shape(values))] = torch.from_numpy(np.array(values, dtype=np.float32)).cuda()
        self.state = self.snapshot()

    def poison(self, *names):
        for name in names:
            at, shape = self.L.blocks[name]
            self.ws[at:at + int(np.prod(shape))] = float('nan')
        self.state = self.snapshot()

    def stage(self, stage, owned):
        L = self.L
        rc = self.lib.gccnmf_klnmf_stage(self.Vd.data_ptr(), self.Wd.data_ptr(), self.Hd.data_ptr(), self.ws.data_ptr(), L.F, L.N, L.K, L.B, ALPHA, EPS,
                                         self.flags, stage, _stream())
        assert rc == OK, '%s: stage %d returned %d' % (self.label, stage, rc)
        was, now = self.state, self.snapshot()
        self.state = now
        for name in self.NAMES:
            if name not in owned:
                same = _bits(now[name]) == _bits(was[name])
                assert same.all(), '%s: stage %d changed %s at %s (it does not own it)' % (self.label, stage, name, tuple(np.argwhere(~same)[0]))
        for name, rows, cols in (('W', L.F, L.K), ('H', L.K, L.N)):
            a = now[name]
            assert not _bits(a[:, rows:, :]).any() and not _bits(a[:, :, cols:]).any(), '%s: stage %d left non-zero padding in %s' % (self.label, stage, name)
        return was, now

    def zero_padded(self, stage, st, *names):
        """every element of R / Q outside f < F, n < N reads 0 (bit for bit +0)"""
        L = self.L
        for name in names:
            a = st[name]
            assert not _bits(a[:, L.F:, :]).any() and not _bits(a[:, :, L.N:]).any(), '%s: stage %d: %s is not zero outside F x N' % (self.label, stage, name)

    def within(self, stage, output, got, refs, bar):
        worst, misses = 0.0, []
        for b, ref in enumerate(refs):
            g = got[b][tuple(slice(0, n) for n in ref.shape)]
            assert np.isfinite(g).all(), '%s: stage %d %s of file %d is not finite' % (self.label, stage, output, b)
            if bar == 0:
                ok = np.array_equal(_bits(g), _bits(np.asarray(ref, np.float32)))
                if not ok:
                    misses.append('file %d is not its reference bit for bit' % b)
                continue
            w, miss = S.share(g, ref, bar)
            worst = max(worst, w)
            if miss is not None:
                misses.append('file %d element %s: %r, reference %r' % (b, miss, g[miss], ref[miss]))
        print('%s: stage %d %s: worst share of the bar (%.1f * 2^-24) %.3f' % (self.label, stage, output, bar / S.U24, worst))
        assert not misses, '%s: stage %d %s misses its bar of %.1f * 2^-24 relative: %s' % (self.label, stage, output, bar / S.U24, '; '.join(misses[:4]))

    def files(self, st, *names):
        L = self.L
        corner = dict(V=(L.F, L.N), W=(L.F, L.K), H=(L.K, L.N), R=(L.F, L.N), Q=(L.F, L.N), Un=(L.F, L.K), Ud=(L.F, L.K), colsumW=(L.K,), s=(L.K,))
        return [[st[n][b][tuple(slice(0, m) for m in corner[n])] for n in names] for b in range(L.B)]

    def call(self, iterations, flags=None):
        L = self.L
        return self.lib.gccnmf_klnmf(self.Vd.data_ptr(), self.Wd.data_ptr(), self.Hd.data_ptr(), self.ws.data_ptr(), L.F, L.N, L.K, L.B, iterations,
                                     ALPHA, EPS, self.flags if flags is None else flags, _stream())


CASES = [(beta,) + shape for beta in BETAS for shape in B.SHAPES]


@pytest.mark.parametrize('beta,F,N,K,files', CASES)
def test_every_stage_against_the_restatement(beta, F, N, K, files):
    r = Run(F, N, K, files, beta, '%s (%d, %d, %d) x %d' % (B.NAMES[beta], F, N, K, files))
    L = r.L
    # stage 0: colsumW, s = 1, R = Q = 0
    was, now = r.stage(0, {'R', 'Q', 'colsumW', 's'})
    r.within(0, 'colsumW', now['colsumW'], [S.stage0(W)[0] for W, in r.files(was, 'W')], S.bar_colsum0(F))
    assert (now['s'][:, :K] == 1).all() and not _bits(now['R']).any() and not _bits(now['Q']).any()
    # stage 1 meets a lazy scale in every iteration but the first; R and Q hold NaN again: the stage writes the whole padded blocks itself
    r.poke('s', r.s0)
    r.poison('R', 'Q')
    was, now = r.stage(1, {'R', 'Q'})
    refs = [B.stage13(V, W, H, s, beta) for V, W, H, s in r.files(was, 'V', 'W', 'H', 's')]
    r.within(1, 'R', now['R'], [x[0] for x in refs], B.bar_R(K, beta))
    r.within(1, 'Q', now['Q'], [x[1] for x in refs], B.bar_Q(K))
    r.zero_padded(1, now, 'R', 'Q')
    # stage 2
    was, now = r.stage(2, {'H'})
    r.within(2, 'H', now['H'], [B.stage2(W, H, s, R, Q) for W, H, s, R, Q in r.files(was, 'W', 'H', 's', 'R', 'Q')], B.bar_H(F))
    # stage 3 (no scale: H carries it)
    r.poison('R', 'Q')
    was, now = r.stage(3, {'R', 'Q'})
    refs = [B.stage13(V, W, H, None, beta) for V, W, H in r.files(was, 'V', 'W', 'H')]
    r.within(3, 'R', now['R'], [x[0] for x in refs], B.bar_R(K, beta))
    r.within(3, 'Q', now['Q'], [x[1] for x in refs], B.bar_Q(K))
    r.zero_padded(3, now, 'R', 'Q')
    # stage 4
    was, now = r.stage(4, {'Un', 'Ud'})
    refs = [B.stage4(R, Q, H) for R, Q, H in r.files(was, 'R', 'Q', 'H')]
    r.within(4, 'Un', now['Un'], [x[0] for x in refs], B.bar_U(N))
    r.within(4, 'Ud', now['Ud'], [x[1] for x in refs], B.bar_U(N))
    # stage 5
    was, now = r.stage(5, {'W', 'colsumW', 's'})
    refs = [B.stage5(W, Un, Ud) for W, Un, Ud in r.files(was, 'W', 'Un', 'Ud')]
    r.within(5, 'W', now['W'], [x[0] for x in refs], B.bar_W(F))
    r.within(5, 's', now['s'], [x[1] for x in refs], B.bar_s(F))
    r.within(5, 'colsumW', now['colsumW'], [x[2] for x in refs], B.bar_colsumW(F))
    # stage 6: one float32 product per element -- exact
    was, now = r.stage(6, {'H'})
    for b, (H, s) in enumerate(r.files(was, 'H', 's')):
        assert np.array_equal(_bits(now['H'][b, :K, :N]), _bits(S.stage6(H, s))), '%s: stage 6: H of file %d is not s * H bit for bit' % (r.label, b)
    # after the full iteration: nothing non-finite came out (the workspace started as NaN), the padding of W and H is exactly 0 (r.stage)
    assert np.isfinite(now['W']).all() and np.isfinite(now['H']).all()


@pytest.mark.parametrize('beta,F,N,K,files', CASES)
def test_the_call_is_the_sequence_of_stage_calls(beta, F, N, K, files):
    from gcc_nmf_amd import _hip
    label = '%s (%d, %d, %d) x %d' % (B.NAMES[beta], F, N, K, files)
    a, b = Run(F, N, K, files, beta, label), Run(F, N, K, files, beta, label)
    assert a.call(5) == OK
    for stage in [0] + 5 * [1, 2, 3, 4, 5] + [6]:
        assert b.lib.gccnmf_klnmf_stage(b.Vd.data_ptr(), b.Wd.data_ptr(), b.Hd.data_ptr(), b.ws.data_ptr(), F, N, K, files, ALPHA, EPS, b.flags, stage,
                                        _stream()) == OK
    sa, sb = a.snapshot(), b.snapshot()
    for name in ('W', 'H'):
        assert np.isfinite(sa[name]).all()
        assert np.array_equal(_bits(sa[name]), _bits(sb[name])), '%s: %s of the call differs from the stage calls' % (label, name)
    assert not np.array_equal(_bits(sa['W'][:, :F, :K]), _bits(a.W0))
    # the call cleared the chain-status words (the workspace held NaN there); the stage calls do not touch them
    assert _hip.klnmf_chain_status(a.ws, F, N, K, files) == 0
    L = a.L
    assert not _bits(a.ws[L.kl - 32:L.kl].cpu().numpy()).any() and np.isnan(b.ws[L.kl - 32:L.kl].cpu().numpy()).all()


@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('F,N,K', [(129, 130, 40), (130, 70, 136)])
def test_a_file_has_the_same_bits_in_a_batch_of_two_and_of_five(beta, F, N, K):
    label = '%s (%d, %d, %d)' % (B.NAMES[beta], F, N, K)
    two, five = Run(F, N, K, 2, beta, label, pick=(0, 1)), Run(F, N, K, 5, beta, label, pick=(4, 2, 3, 0, 1))
    assert two.call(3) == OK and five.call(3) == OK
    s2, s5 = two.snapshot(), five.snapshot()
    for name in ('W', 'H'):
        assert np.isfinite(s5[name]).all()
        assert np.array_equal(_bits(s2[name][0]), _bits(s5[name][3])) and np.array_equal(_bits(s2[name][1]), _bits(s5[name][4])), (label, name)


@pytest.mark.parametrize('beta,F,N,K,files', CASES)
def test_stage_7_against_the_float64_divergence(beta, F, N, K, files):
    """the divergence of positive random factors, V = 0 elements included (low_rank_plus_noise carries five isolated zeros); bit for bit
    the same for a file alone and in its batch"""
    r = Run(F, N, K, files, beta, 'stage 7')
    assert (r.V0 == 0).any()
    L = r.L

    def stage7(run):
        before = [t.clone() for t in (run.Vd, run.Wd, run.Hd)]
        assert run.lib.gccnmf_klnmf_stage(run.Vd.data_ptr(), run.Wd.data_ptr(), run.Hd.data_ptr(), run.ws.data_ptr(), F, N, K, run.L.B, 0.0, 0.0, run.flags, 7,
                                          _stream()) == OK
        torch.cuda.synchronize()
        for t, was in zip((run.Vd, run.Wd, run.Hd), before):
            assert torch.equal(t, was)
        at = run.L.B * L.Fp * L.Np
        return run.ws[at:at + 2 * run.L.B].view(torch.float64).cpu().numpy().copy()
    D = stage7(r)
    for b in range(files):
        want, bar = B.divergence(r.V0[b], r.W0[b], r.H0[b], beta), B.divergence_bar(r.V0[b], r.W0[b], r.H0[b], beta)
        print('%s stage 7 (%d, %d, %d) file %d of %d: D = %.17g, reference %.17g, |error| = %.3g = %.3g of the bar %.3g'
              % (B.NAMES[beta], F, N, K, b, files, D[b], want, abs(D[b] - want), abs(D[b] - want) / bar, bar))
        assert np.isfinite(D[b]) and abs(D[b] - want) <= bar
    alone = stage7(Run(F, N, K, 1, beta, 'stage 7 alone', pick=(files - 1,)))
    assert alone[0].tobytes() == D[files - 1].tobytes()


def test_plan_bit_and_error_codes_launch_nothing():
    lib = _lib()
    F, N, K, files = 129, 130, 40, 3
    for beta in BETAS:
        bit = B.FLAGS[beta]
        assert lib.gccnmf_klnmf_plan(F, N, K, files, bit) == 64 and lib.gccnmf_klnmf_plan(F, N, K, files, 0) & 64 == 0
        r = Run(F, N, K, files, beta, 'errors')
        for t in (r.Wd, r.Hd, r.ws):
            t.fill_(7.0)                                    # sentinels: a rejected call writes nothing
        n = torch.full((files,), N, dtype=torch.int32).numpy()
        import ctypes
        n_c = (ctypes.c_int * files)(*n.tolist())
        rejected = [(3 << 26, ERR_ARG), (bit | (1 << 16), ERR_ARG), (bit | (1 << 16) | (1 << 17), ERR_ARG), (bit | (1 << 17), ERR_ARG),
                    (bit | (8 << 18), ERR_ARG), (bit | 4, ERR_ARG), (bit | 4 | (2 << 8), ERR_ARG), (bit | 2, ERR_ARG)]
        for flags, status in rejected:
            assert r.call(3, flags) == status, hex(flags)
            assert lib.gccnmf_klnmf_plan(F, N, K, files, flags) == -1
            for stage in range(8):
                assert lib.gccnmf_klnmf_stage(r.Vd.data_ptr(), r.Wd.data_ptr(), r.Hd.data_ptr(), r.ws.data_ptr(), F, N, K, files, ALPHA, EPS, flags, stage,
                                              _stream()) == ERR_ARG, (hex(flags), stage)
        assert lib.gccnmf_klnmf_ragged(r.Vd.data_ptr(), r.Wd.data_ptr(), r.Hd.data_ptr(), r.ws.data_ptr(), F, n_c, N, K, files, 3, ALPHA, EPS, bit,
                                       _stream()) == ERR_ARG
        assert lib.gccnmf_klnmf(r.Vd.data_ptr(), r.Wd.data_ptr(), r.Hd.data_ptr(), r.ws.data_ptr() + 8, F, N, K, files, 3, ALPHA, EPS, bit, _stream()) == ERR_ARG
        assert lib.gccnmf_klnmf_stage(r.Vd.data_ptr(), r.Wd.data_ptr(), r.Hd.data_ptr(), r.ws.data_ptr(), F, N, K, files, ALPHA, EPS, bit, 8, _stream()) == ERR_ARG
        # outside the envelope (the sizes alone decide: nothing is read)
        assert lib.gccnmf_klnmf(r.Vd.data_ptr(), r.Wd.data_ptr(), r.Hd.data_ptr(), r.ws.data_ptr(), 2050, N, K, files, 3, ALPHA, EPS, bit, _stream()) == ERR_UNSUPPORTED
        assert lib.gccnmf_klnmf(r.Vd.data_ptr(), r.Wd.data_ptr(), r.Hd.data_ptr(), r.ws.data_ptr(), F, N, 1025, files, 3, ALPHA, EPS, bit, _stream()) == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        for t in (r.Wd, r.Hd, r.ws):
            assert bool((t == 7.0).all())


def test_engine_run_under_itakura_saito():
    import gcc_nmf_amd.gccNMFFunctions as G
    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_batch
    eng = GCCNMFEngine(16000, batch=2, dictionarySize=16, numIterations=10, divergence='is')
    assert eng.nmf_groups == 1 and eng.divergence == 'is'
    y = eng.separate(synthetic_batch(0, 2, numSamples=16000).astype(np.float32))
    assert y.shape[:3] == (2, 3, 2) and np.isfinite(y).all()
    D10 = eng.get_divergence()
    V = eng.get_V()
    W, H = eng.get_WH()
    for b in range(2):
        want = G.getBetaDivergence(V[b], W[b], H[b], 'is')
        print('engine IS file %d: D after 10 iterations %.17g, getBetaDivergence %.17g' % (b, D10[b], want))
        assert np.isfinite(D10[b]) and D10[b].tobytes() == np.float64(want).tobytes()
    eng.iters = 5
    eng.klnmf()
    D5 = eng.get_divergence()
    print('engine IS: D after 5 iterations %s, after 10 %s' % (D5, D10))
    assert (D10 < D5).all()


@pytest.mark.parametrize('beta', BETAS)
def test_performBetaNMF_against_the_float64_trajectory(beta):
    """three iterations of the smallest shape against beta_nmf_restatement.iterate from the same initial factors, within the accumulated
    bars (trajectory_bars: the worst case compounds to 0.67 / 0.40 for IS and 0.047 / 0.030 for Euclid on W / H, so the printed shares
    are the informative figures); the same bits as gccnmf_klnmf on those factors; beta = 1 is performKLNMF bit for bit."""
    import gcc_nmf_amd.gccNMFFunctions as G
    from oracle import gccnmf_oracle as O
    F, N, K = 33, 70, 16
    V = B.low_rank_plus_noise(F, N, 6, 0.3, 3, 5)
    W, H = G.performBetaNMF(V, K, 3, beta, sparsityAlpha=ALPHA, epsilon=EPS)
    assert W.dtype == np.float32 and H.dtype == np.float32 and W.shape == (F, K) and H.shape == (K, N)
    W0, H0 = O.initKLNMF(F, N, K, EPS, 0)
    Wr, Hr = B.iterate(V, W0, H0, beta, np.float32(ALPHA), np.float32(EPS), 3)
    bw, bh = B.trajectory_bars(beta, F, N, K, 3)
    for name, got, ref, bar in (('W', W, Wr, bw), ('H', H, Hr, bh)):
        worst, miss = S.share(got, ref, bar)
        print('performBetaNMF beta = %d, 3 iterations: %s worst |error| / |reference| = %.3g = %.3g of the accumulated bar %.3g'
              % (beta, name, worst * bar, worst, bar))
        assert miss is None, (name, miss, got[miss], ref[miss])
    lib = _lib()
    L = Layout(lib, F, N, K, 1)
    Vd, Wd, Hd = Run._pad(V[None], (1, L.Fp, L.Np)), Run._pad(W0[None], (1, L.Fp, L.Kp)), Run._pad(H0[None], (1, L.Kp, L.Np))
    ws = torch.full((L.floats,), float('nan'), dtype=torch.float32, device='cuda')
    assert lib.gccnmf_klnmf(Vd.data_ptr(), Wd.data_ptr(), Hd.data_ptr(), ws.data_ptr(), F, N, K, 1, 3, ALPHA, EPS, B.FLAGS[beta], _stream()) == OK
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Wd[0, :F, :K].cpu().numpy()), _bits(W)) and np.array_equal(_bits(Hd[0, :K, :N].cpu().numpy()), _bits(H))
    if beta == BETAS[0]:
        kl, one = G.performKLNMF(V, K, 3, ALPHA, EPS), G.performBetaNMF(V, K, 3, 'kl', sparsityAlpha=ALPHA, epsilon=EPS)
        assert np.array_equal(_bits(kl[0]), _bits(one[0])) and np.array_equal(_bits(kl[1]), _bits(one[1]))
        d = G.getBetaDivergence(V, W, H, beta)
        assert abs(d - B.divergence(V, W, H, beta)) <= B.divergence_bar(V, W, H, beta)
        assert G.getBetaDivergence(V, W, H, 1).tobytes() == G.getKLDivergence(V, W, H).tobytes()
