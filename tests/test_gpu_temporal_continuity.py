"""Temporal-continuity KL-NMF (gccnmf_klnmf / gccnmf_klnmf_stage with GCCNMF_FLAG_CONTINUITY, csrc/nmf_smooth.hip) through the C ABI and
through the Python layers.  Every stage 0-6 is compared element by element with the float64 restatement of that stage
(tests/temporal_continuity_restatement.py and klnmf_stages_restatement.py, which derive the bars) evaluated on the float32 state the device
held before it; the intermediates -- E, D, Gm and Gp among them -- are read at the offsets include/gccnmf_hip.h documents.  The workspace
starts as NaN and so does the padding of H.  Every comparison prints its worst share of the bar before it asserts.

The shapes (temporal_continuity_restatement.SHAPES) are the smallest that reach each way to go wrong: the segment boundary inside a
64-column tile (T = 40), exactly on a tile edge (T = 64), neighbours across a tile edge and a row of one more than a pass of the row
launch's wave (T = 65), T = 1 and T = 2, one segment with N odd; K in {1, 33, 100, 130}, F in {2, 33, 513}.  The weights: 10, at which a
Gauss-Seidel neighbour (a value the same launch has already updated) or a neighbour from the padding or from the other segment moves H far
beyond its bar, and 0 with the bit set (the device's own path, not the KL call's)."""
import ctypes
import functools
import struct

import numpy as np
import pytest
import torch

import klnmf_stages_restatement as S
import temporal_continuity_restatement as C

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
ALPHA, EPS = float(S.ALPHA), float(S.EPS)
POOL = 5                                                    # problems per shape; a Run takes the first `files` of them, or those it picks
WEIGHTS = [10.0, 0.0]


def _lib():
    from gcc_nmf_amd import _hip
    return _hip.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _problem(F, T, K, segments, zero_row):
    return C.problem(F, T, K, segments, POOL, zero_row)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def words(K, batch, weight):
    """GCCNMF_CONTINUITY_K(K, bits), GCCNMF_CONTINUITY_BATCH(batch, bits) of include/gccnmf_hip.h"""
    b = struct.unpack('<I', struct.pack('<f', weight))[0]
    signed = lambda v: ctypes.c_int32(v & 0xffffffff).value
    return signed(K | (b & 0xffff0000)), signed(batch | ((b & 0xffff) << 16))


class Layout(object):
    """Where a temporal-continuity call keeps its intermediates (include/gccnmf_hip.h, at gccnmf_klnmf_stage), in floats: the KL layout --
    R | U | colsumW | rowsumH | s | ... -- of gccnmf_klnmf_workspace_floats floats, then Gm | Gp | E | D."""

    def __init__(self, lib, F, N, K, files):
        self.F, self.N, self.K, self.B = F, N, K, files
        self.Fp, self.Kp, self.Np = -(-F // 16) * 16, -(-K // 64) * 64, -(-N // 64) * 64
        Fp, Kp, Np = self.Fp, self.Kp, self.Np
        self.kl = lib.gccnmf_klnmf_workspace_floats(F, N, K, files)
        self.floats = self.kl + files * Kp * (2 * Np + 4)          # GCCNMF_KLNMF_CONTINUITY_WORKSPACE_FLOATS behind the KL layout
        self.blocks, at = {}, 0
        for name, shape in (('R', (files, Fp, Np)), ('U', (files, Fp, Kp)), ('colsumW', (files, Kp)), ('rowsumH', (files, Kp)), ('s', (files, Kp))):
            self.blocks[name] = (at, shape)
            at += int(np.prod(shape))
        assert at <= self.kl - 32
        at = self.kl
        for name, shape in (('Gm', (files, Kp, Np)), ('Gp', (files, Kp, Np)), ('E', (files, 2, Kp)), ('D', (files, 2, Kp))):
            self.blocks[name] = (at, shape)
            at += int(np.prod(shape))
        assert at == self.floats

    def view(self, ws, name):
        at, shape = self.blocks[name]
        return ws[at:at + int(np.prod(shape))].reshape(shape)


class Run(object):
    """`files` problems on the device: zero-padded V and W, H padded with NaN, a workspace pre-filled with NaN."""

    def __init__(self, F, T, K, segments, files, weight, label, pick=None, zero_row=False):
        self.lib, self.weight, self.segments, self.label, self.flags = _lib(), weight, segments, label, C.flags(segments)
        N = T * segments
        self.L = L = Layout(self.lib, F, N, K, files)
        self.Kw, self.Bw = words(K, files, weight)
        V, W, H, s = _problem(F, T, K, segments, zero_row)      # (always the same pool: a file is the same problem in every batch)
        idx = list(range(files)) if pick is None else list(pick)
        self.V0, self.W0, self.H0, self.s0 = V[idx], W[idx], H[idx], s[idx]
        self.Vd, self.Wd = self._pad(self.V0, (files, L.Fp, L.Np)), self._pad(self.W0, (files, L.Fp, L.Kp))
        self.Hd = self._pad(self.H0, (files, L.Kp, L.Np), float('nan'))
        self.ws = torch.full((L.floats,), float('nan'), dtype=torch.float32, device='cuda')
        self.state = self.snapshot()

    @staticmethod
    def _pad(a, shape, fill=0.0):
        t = torch.full(shape, fill, dtype=torch.float32, device='cuda')
        t[tuple(slice(0, n) for n in a.shape)] = torch.from_numpy(np.array(a)).cuda()
        return t

    def snapshot(self):
        torch.cuda.synchronize()
        ws = self.ws.cpu().numpy()
        st = dict(V=self.Vd.cpu().numpy(), W=self.Wd.cpu().numpy(), H=self.Hd.cpu().numpy(), ws=ws)
        for name in self.L.blocks:
            st[name] = self.L.view(ws, name)
        return st

    def poke(self, name, values):
        """overwrite the corner of the workspace block `name` (B, ...) on the device"""
        at, shape = self.L.blocks[name]
        self.ws[at:at + int(np.prod(shape))].view(shape)[tuple(slice(0, n) for n in np.shape(values))] = torch.from_numpy(np.array(values, dtype=np.float32)).cuda()
        self.state = self.snapshot()

    def poison(self, *names):
        for name in names:
            at, shape = self.L.blocks[name]
            self.ws[at:at + int(np.prod(shape))] = float('nan')
        self.state = self.snapshot()

    def raw_stage(self, stage):
        L = self.L
        return self.lib.gccnmf_klnmf_stage(self.Vd.data_ptr(), self.Wd.data_ptr(), self.Hd.data_ptr(), self.ws.data_ptr(), L.F, L.N, self.Kw, self.Bw, ALPHA,
                                           EPS, self.flags, stage, _stream())

    def stage(self, stage, owned):
        """run one stage; V and everything the stage does not own -- the factors and EVERY float of the workspace outside the owned blocks
        -- keep their bits"""
        L = self.L
        rc = self.raw_stage(stage)
        assert rc == OK, '%s: stage %d returned %d' % (self.label, stage, rc)
        was, now = self.state, self.snapshot()
        self.state = now
        for name in ('V', 'W', 'H'):
            if name not in owned:
                same = _bits(now[name]) == _bits(was[name])
                assert same.all(), '%s: stage %d changed %s at %s (it does not own it)' % (self.label, stage, name, tuple(np.argwhere(~same)[0]))
        free = np.ones(L.floats, bool)
        for name in owned:
            if name in L.blocks:
                at, shape = L.blocks[name]
                free[at:at + int(np.prod(shape))] = False
        same = (_bits(now['ws']) == _bits(was['ws'])) | ~free
        assert same.all(), '%s: stage %d wrote the workspace at float %d, outside %s' % (self.label, stage, int(np.argwhere(~same)[0]), sorted(owned))
        a = now['W']
        assert not _bits(a[:, L.F:, :]).any() and not _bits(a[:, :, L.K:]).any(), '%s: stage %d left non-zero padding in W' % (self.label, stage)
        return was, now

    def zero_padded(self, stage, st, name):
        """every element of R outside f < F, n < N reads 0 (bit for bit +0)"""
        L = self.L
        a = st[name]
        assert not _bits(a[:, L.F:, :]).any() and not _bits(a[:, :, L.N:]).any(), '%s: stage %d: %s is not zero outside F x N' % (self.label, stage, name)

    def within(self, stage, output, got, refs, bar):
        worst, misses = 0.0, []
        for b, ref in enumerate(refs):
            g = got[b][tuple(slice(0, n) for n in ref.shape)]
            assert np.isfinite(g).all(), '%s: stage %d %s of file %d is not finite' % (self.label, stage, output, b)
            w, miss = S.share(g, ref, bar)
            worst = max(worst, w)
            if miss is not None:
                misses.append('file %d element %s: %r, reference %r' % (b, miss, g[miss], ref[miss]))
        print('%s: stage %d %s: worst share of the bar (%.1f * 2^-24) %.3f' % (self.label, stage, output, bar / S.U24, worst))
        assert not misses, '%s: stage %d %s misses its bar of %.1f * 2^-24 relative: %s' % (self.label, stage, output, bar / S.U24, '; '.join(misses[:4]))

    def files(self, st, *names):
        L = self.L
        corner = dict(V=(L.F, L.N), W=(L.F, L.K), H=(L.K, L.N), R=(L.F, L.N), U=(L.F, L.K), colsumW=(L.K,), rowsumH=(L.K,), s=(L.K,))
        return [[st[n][b][tuple(slice(0, m) for m in corner[n])] for n in names] for b in range(L.B)]

    def check_stage_2(self, was, now):
        """E, D, Gm, Gp and H of stage 2 against the restatement of the state before it; what the launch leaves alone"""
        L, seg = self.L, self.segments
        K, N = L.K, L.N
        refs = [C.terms(H, s, seg) for H, s in self.files(was, 'H', 's')]
        self.within(2, 'E', now['E'][:, :seg, :K].transpose(0, 2, 1), [x[0] for x in refs], C.bar_ED())
        self.within(2, 'D', now['D'][:, :seg, :K].transpose(0, 2, 1), [x[1] for x in refs], C.bar_ED())
        self.within(2, 'Gm', now['Gm'], [x[2] for x in refs], C.bar_G())
        self.within(2, 'Gp', now['Gp'], [x[3] for x in refs], C.bar_G())
        for name in ('Gm', 'Gp'):                           # written inside k < K, n < N alone: the rest is the NaN it was
            a = now[name]
            assert np.isnan(a[:, K:, :]).all() and np.isnan(a[:, :, N:]).all(), '%s: stage 2 wrote the padding of %s' % (self.label, name)
        for name in ('E', 'D'):
            a = now[name]
            assert np.isnan(a[:, :, K:]).all() and np.isnan(a[:, seg:, :]).all(), '%s: stage 2 wrote %s beyond its atoms and segments' % (self.label, name)
        self.within(2, 'H', now['H'], [C.stage2(W, H, s, R, c, self.weight, seg) for W, H, s, R, c in self.files(was, 'W', 'H', 's', 'R', 'colsumW')],
                    C.bar_H(L.F))
        H = now['H']
        assert not _bits(H[:, :K, N:]).any(), '%s: stage 2 did not write +0 into the padding columns of H' % self.label
        assert np.isnan(H[:, K:, :]).all(), '%s: stage 2 wrote the padding rows of H' % self.label

    def call(self, iterations, flags=None, ws_offset=0, F=None, K=None):
        L = self.L
        Kw = self.Kw if K is None else words(K, L.B, self.weight)[0]
        return self.lib.gccnmf_klnmf(self.Vd.data_ptr(), self.Wd.data_ptr(), self.Hd.data_ptr(), self.ws.data_ptr() + ws_offset, L.F if F is None else F, L.N,
                                     Kw, self.Bw, iterations, ALPHA, EPS, self.flags if flags is None else flags, _stream())


def _label(F, T, K, segments, files, weight):
    return 'continuity %g (%d, %d x %d, %d) x %d' % (weight, F, segments, T, K, files)


CASES = [(weight,) + shape for weight in WEIGHTS for shape in C.SHAPES]


@pytest.mark.parametrize('weight,F,T,K,segments,files', CASES)
def test_every_stage_against_the_restatement(weight, F, T, K, segments, files):
    r = Run(F, T, K, segments, files, weight, _label(F, T, K, segments, files, weight))
    N = T * segments
    # stage 0: colsumW, s = 1, R = 0
    was, now = r.stage(0, {'R', 'colsumW', 's'})
    r.within(0, 'colsumW', now['colsumW'], [S.stage0(W)[0] for W, in r.files(was, 'W')], S.bar_colsum0(F))
    assert (now['s'][:, :K] == 1).all() and not _bits(now['R']).any()
    # stage 1 meets a lazy scale in every iteration but the first; R holds NaN again: the stage writes the whole padded block itself
    r.poke('s', r.s0)
    r.poison('R')
    was, now = r.stage(1, {'R'})
    r.within(1, 'R', now['R'], [S.stage1(V, W, H, s) for V, W, H, s in r.files(was, 'V', 'W', 'H', 's')], S.bar_R(K))
    r.zero_padded(1, now, 'R')
    # stage 2: the continuity launch and the H update
    was, now = r.stage(2, {'H', 'Gm', 'Gp', 'E', 'D'})
    r.check_stage_2(was, now)
    if weight == 0:                                         # ... which at weight 0 is the KL stage
        r.within(2, 'H (KL)', now['H'], [S.stage2(W, H, s, R, c) for W, H, s, R, c in r.files(was, 'W', 'H', 's', 'R', 'colsumW')], C.bar_H(F))
    # stage 3 (no scale: H carries it)
    r.poison('R')
    was, now = r.stage(3, {'R'})
    r.within(3, 'R', now['R'], [S.stage3(V, W, H) for V, W, H in r.files(was, 'V', 'W', 'H')], S.bar_R(K))
    r.zero_padded(3, now, 'R')
    # stage 4
    was, now = r.stage(4, {'U', 'rowsumH'})
    refs = [S.stage4(R, H) for R, H in r.files(was, 'R', 'H')]
    r.within(4, 'U', now['U'], [x[0] for x in refs], S.bar_U(N))
    r.within(4, 'rowsumH', now['rowsumH'], [x[1] for x in refs], S.bar_rowsumH(N))
    # stage 5
    was, now = r.stage(5, {'W', 'colsumW', 's'})
    refs = [S.stage5(W, U, rs) for W, U, rs in r.files(was, 'W', 'U', 'rowsumH')]
    r.within(5, 'W', now['W'], [x[0] for x in refs], S.bar_W(F))
    r.within(5, 's', now['s'], [x[1] for x in refs], S.bar_s(F))
    r.within(5, 'colsumW', now['colsumW'], [x[2] for x in refs], S.bar_colsumW(F))
    # stage 6: one float32 product per element -- exact
    was, now = r.stage(6, {'H'})
    for b, (H, s) in enumerate(r.files(was, 'H', 's')):
        assert np.array_equal(_bits(now['H'][b, :K, :N]), _bits(S.stage6(H, s))), '%s: stage 6: H of file %d is not s * H bit for bit' % (r.label, b)
    assert np.isfinite(now['W']).all() and np.isfinite(now['H'][:, :K, :N]).all()


@pytest.mark.parametrize('F,T,K,segments,files', [(33, 40, 33, 2, 2), (33, 71, 100, 1, 3)])
def test_an_all_zero_row_of_H(F, T, K, segments, files):
    """E = 0: Gm = Gp = 0 (not 0 / 0), the row stays exactly zero, its neighbours in k are untouched by it"""
    r = Run(F, T, K, segments, files, 10.0, _label(F, T, K, segments, files, 10.0) + ', a dead row', zero_row=True)
    assert not r.H0[0, 1].any() and r.H0[1, 1].all()
    r.stage(0, {'R', 'colsumW', 's'})
    r.poke('s', r.s0)
    r.stage(1, {'R'})
    was, now = r.stage(2, {'H', 'Gm', 'Gp', 'E', 'D'})
    r.check_stage_2(was, now)
    for name in ('Gm', 'Gp', 'H'):
        assert not _bits(now[name][0, 1, :T * segments]).any(), name
    assert not _bits(now['E'][0, :segments, 1]).any() and not _bits(now['D'][0, :segments, 1]).any()


@pytest.mark.parametrize('F,T,K,segments,files', C.SHAPES)
def test_the_call_is_the_sequence_of_stage_calls(F, T, K, segments, files):
    from gcc_nmf_amd import _hip
    label = _label(F, T, K, segments, files, 10.0)
    a, b = Run(F, T, K, segments, files, 10.0, label), Run(F, T, K, segments, files, 10.0, label)
    V = a.Vd.clone()
    assert a.call(3) == OK
    for stage in [0] + 3 * [1, 2, 3, 4, 5] + [6]:
        assert b.raw_stage(stage) == OK
    sa, sb = a.snapshot(), b.snapshot()
    N = T * segments
    for name, rows, cols in (('W', F, K), ('H', K, N)):
        assert np.isfinite(sa[name][:, :rows, :cols]).all()
        assert np.array_equal(_bits(sa[name]), _bits(sb[name])), '%s: %s of the call differs from the stage calls' % (label, name)
    assert not np.array_equal(_bits(sa['W'][:, :F, :K]), _bits(a.W0)) and torch.equal(a.Vd, V)
    # the call cleared the chain-status words (the workspace held NaN there); the stage calls do not touch them
    L = a.L
    assert _hip.klnmf_chain_status(a.ws, F, N, K, files) == 0
    assert not _bits(a.ws[L.kl - 32:L.kl].cpu().numpy()).any() and np.isnan(b.ws[L.kl - 32:L.kl].cpu().numpy()).all()
    # and the weight matters: the same call at weight 0 leaves other factors (T = 1 has no term at all)
    c = Run(F, T, K, segments, files, 0.0, label)
    assert c.call(3) == OK
    assert np.array_equal(_bits(c.snapshot()['H']), _bits(sa['H'])) == (T == 1)


@pytest.mark.parametrize('F,T,K,segments', [(33, 65, 130, 2), (513, 64, 100, 2), (33, 71, 100, 1), (33, 40, 33, 2)])
def test_a_file_has_the_same_bits_alone_in_a_batch_of_two_and_in_a_permuted_batch_of_five(F, T, K, segments):
    label = 'continuity 10 (%d, %d x %d, %d)' % (F, segments, T, K)
    one = Run(F, T, K, segments, 1, 10.0, label, pick=(1,))
    two, five = Run(F, T, K, segments, 2, 10.0, label, pick=(0, 1)), Run(F, T, K, segments, 5, 10.0, label, pick=(4, 2, 3, 0, 1))
    assert one.call(3) == OK and two.call(3) == OK and five.call(3) == OK
    s1, s2, s5 = one.snapshot(), two.snapshot(), five.snapshot()
    for name, rows, cols in (('W', F, K), ('H', K, T * segments)):
        assert np.isfinite(s5[name][:, :rows, :cols]).all()
        assert np.array_equal(_bits(s2[name][0]), _bits(s5[name][3])) and np.array_equal(_bits(s2[name][1]), _bits(s5[name][4])), (label, name)
        assert np.array_equal(_bits(s1[name][0]), _bits(s2[name][1])), (label, name)


def test_plan_bit_and_error_codes_launch_nothing():
    lib = _lib()
    F, T, K, segments, files = 33, 40, 33, 2, 2
    N = T * segments
    for seg in (1, 2):
        bit = C.flags(seg)
        Kw, Bw = words(K, files, 10.0)
        assert lib.gccnmf_klnmf_plan(F, N, Kw, Bw, bit) == C.PLAN_BIT and lib.gccnmf_klnmf_plan(F, N, K, files, 0) & C.PLAN_BIT == 0
        r = Run(F, T, K, segments, files, 10.0, 'errors')
        r.flags = bit
        for t in (r.Wd, r.Hd, r.ws):
            t.fill_(7.0)                                    # sentinels: a rejected call writes nothing
        n_c = (ctypes.c_int * files)(*([N] * files))
        rejected = [C.STEREO, bit | (1 << 16), bit | (1 << 16) | (1 << 17), bit | (1 << 17), bit | (8 << 18), bit | (1 << 26), bit | (2 << 26), bit | 4,
                    bit | 4 | (2 << 8), bit | 2]
        for flags in rejected:
            assert r.call(3, flags) == ERR_ARG, hex(flags)
            assert lib.gccnmf_klnmf_plan(F, N, Kw, Bw, flags) == -1
            r.flags = flags
            for stage in range(8):
                assert r.raw_stage(stage) == ERR_ARG, (hex(flags), stage)
            r.flags = bit
        for weight in (-1.0, float('nan'), float('inf')):
            r.Kw, r.Bw = words(K, files, weight)
            assert r.call(3) == ERR_ARG and r.raw_stage(2) == ERR_ARG and lib.gccnmf_klnmf_plan(F, N, r.Kw, r.Bw, bit) == -1, weight
        r.Kw, r.Bw = Kw, Bw
        assert lib.gccnmf_klnmf_ragged(r.Vd.data_ptr(), r.Wd.data_ptr(), r.Hd.data_ptr(), r.ws.data_ptr(), F, n_c, N, K, files, 3, ALPHA, EPS, bit,
                                       _stream()) == ERR_ARG
        assert r.call(3, ws_offset=8) == ERR_ARG and r.raw_stage(8) == ERR_ARG
        if seg == 2:                                        # two segments, N odd
            assert lib.gccnmf_klnmf(r.Vd.data_ptr(), r.Wd.data_ptr(), r.Hd.data_ptr(), r.ws.data_ptr(), F, N - 1, Kw, Bw, 3, ALPHA, EPS, bit, _stream()) == ERR_ARG
        # outside the envelope (the sizes alone decide: nothing is read)
        assert r.call(3, F=2050) == ERR_UNSUPPORTED and r.call(3, K=1025) == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        for t in (r.Wd, r.Hd, r.ws):
            assert bool((t == 7.0).all())


def test_engine_runs_with_a_weight_and_with_lengths():
    """the engine's factors are performTemporalKLNMF's on its own V bit for bit (one launch form: a file's bits do not follow the batch),
    get_divergence() stays the KL divergence, weight 0 is the engine without the keyword, and lengths= runs each length as a batch of its own"""
    import gcc_nmf_amd.gccNMFFunctions as G
    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_batch
    x = synthetic_batch(0, 2, numSamples=16000).astype(np.float32)
    kw = dict(batch=2, dictionarySize=16, numIterations=10)
    eng = GCCNMFEngine(16000, temporalContinuity=1.0, **kw)
    assert eng.nmf_groups == 1 and eng.temporalContinuity == 1.0
    y = eng.separate(x)
    assert y.shape[:3] == (2, 3, 2) and np.isfinite(y).all()
    D, V = eng.get_divergence(), eng.get_V()
    W, H = eng.get_WH()
    plain = GCCNMFEngine(16000, **kw)
    plain.separate(x)
    W0, H0 = plain.get_WH()
    zero = GCCNMFEngine(16000, temporalContinuity=0.0, **kw)
    zero.separate(x)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(zero.get_WH(), (W0, H0)))
    for b in range(2):
        Wf, Hf = G.performTemporalKLNMF(V[b], 16, 10, 0, 1.0, 2)
        assert np.array_equal(_bits(Wf), _bits(W[b])) and np.array_equal(_bits(Hf), _bits(H[b])), b
        want = G.getKLDivergence(V[b], W[b], H[b])
        c1, c0 = G.getTemporalContinuity(H[b], 2), G.getTemporalContinuity(H0[b], 2)
        print('engine, temporalContinuity = 1, file %d: KL divergence %.17g (getKLDivergence %.17g), continuity cost %.6g against %.6g at weight 0'
              % (b, D[b], want, c1, c0))
        assert np.isfinite(D[b]) and D[b].tobytes() == np.float64(want).tobytes()
        assert not np.array_equal(_bits(H[b]), _bits(H0[b]))
    lengths = [16000, 12032, 16000]
    rag = GCCNMFEngine(lengths=lengths, temporalContinuity=1.0, dictionarySize=16, numIterations=10)
    mixtures = [x[0], x[1][:, :12032], x[1]]
    out = rag.separate(mixtures)
    assert rag.ragged is None and rag.ragged_klnmf_used is False and all(np.isfinite(o).all() for o in out)
    long = rag.sub[16000]
    assert long.temporalContinuity == 1.0
    Wl, Hl = long.get_WH()
    assert np.array_equal(_bits(Wl), _bits(W)) and np.array_equal(_bits(Hl), _bits(H))          # files 0 and 2 are the batch above


def test_performTemporalKLNMF_against_the_float64_trajectory():
    """three iterations of a small shape against temporal_continuity_restatement.iterate from the same initial factors, within the
    accumulated bars (trajectory_bars: the worst case compounds, so the printed shares are the informative figures); the same bits as
    gccnmf_klnmf on those factors; weight 0 is performKLNMF bit for bit."""
    import gcc_nmf_amd.gccNMFFunctions as G
    from oracle import gccnmf_oracle as O
    F, T, K, segments, weight = 33, 35, 16, 2, 1.0
    N = T * segments
    V = S.low_rank_plus_noise(F, N, 6, 0.3, 3, 5)
    W, H = G.performTemporalKLNMF(V, K, 3, ALPHA, weight, segments, EPS)
    assert W.dtype == np.float32 and H.dtype == np.float32 and W.shape == (F, K) and H.shape == (K, N)
    W0, H0 = O.initKLNMF(F, N, K, EPS, 0)
    Wr, Hr = np.asarray(W0, np.float64), np.asarray(H0, np.float64)
    kappa = 0.0
    for _ in range(3):
        kappa = max(kappa, C.conditioning(Hr, segments))
        Wr, Hr = C.iterate(V, Wr, Hr, weight, segments, np.float32(ALPHA), np.float32(EPS), 1)
    bw, bh = C.trajectory_bars(F, N, K, 3, kappa)
    assert max(bw, bh) < 1.0
    for name, got, ref, bar in (('W', W, Wr, bw), ('H', H, Hr, bh)):
        worst, miss = S.share(got, ref, bar)
        print('performTemporalKLNMF weight %g, 3 iterations (sqrt(E / D) <= %.3g): %s worst |error| / |reference| = %.3g = %.3g of the accumulated bar %.3g'
              % (weight, kappa, name, worst * bar, worst, bar))
        assert miss is None, (name, miss, got[miss], ref[miss])
    lib = _lib()
    L = Layout(lib, F, N, K, 1)
    Vd, Wd, Hd = Run._pad(V[None], (1, L.Fp, L.Np)), Run._pad(W0[None], (1, L.Fp, L.Kp)), Run._pad(H0[None], (1, L.Kp, L.Np))
    ws = torch.full((L.floats,), float('nan'), dtype=torch.float32, device='cuda')
    Kw, Bw = words(K, 1, weight)
    assert lib.gccnmf_klnmf(Vd.data_ptr(), Wd.data_ptr(), Hd.data_ptr(), ws.data_ptr(), F, N, Kw, Bw, 3, ALPHA, EPS, C.flags(segments), _stream()) == OK
    torch.cuda.synchronize()
    assert np.array_equal(_bits(Wd[0, :F, :K].cpu().numpy()), _bits(W)) and np.array_equal(_bits(Hd[0, :K, :N].cpu().numpy()), _bits(H))
    kl, zero = G.performKLNMF(V, K, 3, ALPHA, EPS), G.performTemporalKLNMF(V, K, 3, ALPHA, 0.0, segments, EPS)
    assert np.array_equal(_bits(kl[0]), _bits(zero[0])) and np.array_equal(_bits(kl[1]), _bits(zero[1]))
    assert G.getTemporalContinuity(H, segments) == C.cost(H, segments)
