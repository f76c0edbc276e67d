"""Every stage of the KL-NMF iteration (gccnmf_klnmf_stage, stages 0-6) in the launch forms the stage entry point dispatches to -- the direct
kernels, the small-batch and the throughput tile (LDS-DMA and register-staged; full, narrow and half-height items), K1 + K2 and K3 + K4a
fused, the W update in the R.H^T epilogue of either GEMM kernel, the three W-update kernels, the plain launches at the smallest shapes the chained
launches exist for -- each element of each output against the
float64 restatement of that stage (tests/klnmf_stages_restatement.py, which derives the bars) evaluated on the state the device held
BEFORE the stage -- rounding never compounds from stage to stage, and one wrong bin, frame or atom cannot hide in a norm.

_run drives stages 0, 1, ... 6 one call at a time through the C ABI with a synchronisation and a download after each.  The workspace holds
arbitrary bits before stage 0 (stage 0 must establish everything the later stages read); the padding of V, W and H is zero (the contract).
After every stage: every element of what the stage produced within its bar (a reference of exactly 0 -- the silent bin and the silent
frame of V -- demands exactly 0), the padding of W, H and of each file's R block exactly zero, and every other buffer, V first of all, bit
for bit what it was.  Two things are written by the helper between stages, both to reach states an iteration really meets:
  * after stage 0 (whose s = 1 is asserted) the lazy scale s is replaced by values in [0.5, 2): stages 1 and 2 of every iteration but the
    first run with s != 1;
  * after the H update the silent frame's column of H -- exactly 0, asserted -- gets its old values back: stage 3 would divide 0 by 0 in
    that frame (the reference does; tests/test_klnmf_stages_host.py shows it) and the NaN would swallow U and W.  With the column restored
    the frame's R is again exactly 0 in stage 3 and contributes exactly nothing to U.
Forms that do not materialise an intermediate are checked on what they do produce, where they produce it: K1 + K2 fused -- stage 1 returns
the updated H, R stays zero, stage 2 changes nothing; K3 + K4a fused -- stage 3 writes U and rowsumH; the W update in the epilogue of
R.H^T -- stage 4 writes W, colsumW and s, stage 5 changes nothing; the direct kernels -- stage 3 writes R transposed (Rt) and, of R itself,
only bin F - 1, and keep transposed copies Wt, Ht beside W and H.

Every check prints its worst share of the bar before it asserts; DESIGN section 2b records the figures."""
import contextlib

import numpy as np
import pytest
import torch

import klnmf_stages_restatement as S

pytestmark = pytest.mark.gpu

DEFAULTS = {2: 0, 3: 1, 9: 1, 10: 1, 16: 1, 17: 1}
NO_XCD_AFFINITY, UNFUSED_W_UPDATE = S.NO_XCD_AFFINITY, S.UNFUSED_W_UPDATE


def GROUPS(n):
    return 4 | (n << 8)


def _lib():
    from gcc_nmf_amd import _hip
    return _hip.lib()


@contextlib.contextmanager
def _tuning(keys):
    lib = _lib()
    try:
        for k, v in keys.items():
            assert lib.gccnmf_set_tuning(k, v) == 0, 'gccnmf_set_tuning(%d, %d) was refused: a product key, which every build accepts' % (k, v)
        yield lib
    finally:
        for k in keys:
            lib.gccnmf_set_tuning(k, DEFAULTS[k])


class Form(object):
    """The launch form a call takes, restated by hand from plan_klnmf (csrc/nmf.hip; its fields direct, fused12, head34 and w_in_rht are
    `direct`, `f12`, `f34` and `fw` here) and launch_rht_update_w: which stage produces what.  `direct`, `f12` and `f34` are asserted against
    gccnmf_klnmf_plan, so they cannot go stale unnoticed.  `fw` has no plan bit: a wrong value fails through the ownership check (stage 4 or stage 5 would
    write what the case says it does not own), not by name.  Which kernel carries the W update -- `dma_updw` for the fused one, the
    branch of launch_update_w for stage 5 -- is observable nowhere: it is restated here and in the case comments only, and a change of
    those rules in the library has to be followed here by hand."""

    def __init__(self, F, N, K, B, flags, keys):
        k = dict(DEFAULTS)
        k.update(keys)
        groups = max((flags >> 8) & 255, 2) if flags & 4 else 1
        tail = F % 128 == 1
        Fm = F - 1 if tail else F
        self.direct = bool(k[10]) and k[2] == 0 and B * groups <= 4
        short = k[2] == 0 and not self.direct and B >= 2 and tail and 64 <= Fm <= 512 and K <= 128
        assert not short or (k[16] != 1 and k[17] != 1), 'a short-dictionary case leaves keys 16 / 17 to the cost model'
        self.f12 = short and k[16] == 2
        self.f34 = short and k[17] == 2 and (Fm // 64) * 16 >= 32 * -(-K // 32)
        self.fw = (not self.direct and not self.f34 and not flags & UNFUSED_W_UPDATE and 128 < Fm <= 512 and k[2] != 2
                   and (k[2] == 1 or B * groups * -(-K // 64) >= 256))
        # launch_rht_update_w: the LDS-DMA kernel carries the full-tile form of the epilogue only; anything else the register-staged kernel
        self.dma_updw = self.fw and bool(k[3]) and Fm % 128 == 0 and K % 64 == 0
        self.direct_tail = self.direct and F > 16 and F % 16 == 1
        self.plan = (1 if self.direct else 0) | (2 if self.f12 else 0) | (4 if self.f34 else 0)

    def __str__(self):
        return '+'.join(n for n, on in (('direct', self.direct), ('K1K2', self.f12), ('K3K4a', self.f34), ('K4aK4b LDS-DMA', self.dma_updw),
                                         ('K4aK4b register-staged', self.fw and not self.dma_updw)) if on) or 'four launches'


class Layout(object):
    """Where klnmf_stage keeps its intermediates in the workspace (include/gccnmf_hip.h, at gccnmf_klnmf_stage), in floats."""

    def __init__(self, F, N, K, B):
        self.F, self.N, self.K, self.B = F, N, K, B
        self.Fp, self.Kp, self.Np = -(-F // 16) * 16, -(-K // 64) * 64, -(-N // 64) * 64
        Fp, Kp, Np = self.Fp, self.Kp, self.Np
        self.blocks, at = {}, 0
        for name, shape in (('R', (B, Fp, Np)), ('U', (B, Fp, Kp)), ('colsumW', (B, Kp)), ('rowsumH', (B, Kp)), ('s', (B, Kp))):
            self.blocks[name] = (at, shape)
            at += int(np.prod(shape))
        if B == 1:
            at += 4 * (max(Fp * Np, Fp * Kp) + Kp)                     # (one file: room the lab build's split reductions use)
        for name, shape in (('Wt', (B, Kp, Fp)), ('Ht', (B, Np, Kp)), ('Rt', (B, Np, Fp))):       # the direct kernels' transposed copies (B <= 8)
            self.blocks[name] = (at, shape)
            at += int(np.prod(shape))

    def view(self, ws, name):
        at, shape = self.blocks[name]
        return ws[at:at + int(np.prod(shape))].reshape(shape)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Run(object):
    def __init__(self, lib, F, N, K, B, flags, form, label):
        self.lib, self.L, self.flags, self.form, self.label = lib, Layout(F, N, K, B), flags, form, label
        L = self.L
        self.V0, self.W0, self.H0, self.s0 = (a[:B] for a in S.problem(F, N, K, max(B, 2)))
        self.Vd = self._pad(self.V0, (B, L.Fp, L.Np))
        self.Wd = self._pad(self.W0, (B, L.Fp, L.Kp))
        self.Hd = self._pad(self.H0, (B, L.Kp, L.Np))
        n_ws = lib.gccnmf_klnmf_workspace_floats(F, N, K, B)
        assert n_ws >= max(at + int(np.prod(shape)) for name, (at, shape) in L.blocks.items() if form.direct or name not in ('Wt', 'Ht', 'Rt'))
        self.ws = torch.from_numpy(np.random.RandomState(1).randint(1, 1 << 30, n_ws).astype(np.int32)).cuda().view(torch.float32)   # arbitrary bits
        self.names = ['V', 'W', 'H', 'R', 'U', 'colsumW', 'rowsumH', 's'] + (['Wt', 'Ht', 'Rt'] if form.direct else [])
        self.shares = {}
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
        for name in self.names[3:]:
            st[name] = self.L.view(ws, name)
        return st

    def poke(self, name, b, index, values):
        """write `values` into file b's block `name` at `index` on the device (W, H or a workspace block)"""
        t = {'W': self.Wd, 'H': self.Hd}.get(name)
        if t is None:
            at, shape = self.L.blocks[name]
            t = self.ws[at:at + int(np.prod(shape))].view(shape)
        t[b][index] = torch.from_numpy(np.array(values, dtype=np.float32)).cuda()

    def stage(self, stage, owned):
        """run one stage; -> (state before, state after), having asserted that everything outside `owned` is bit for bit what it was and
        that the padding of W, H, R (and Rt) is zero"""
        L = self.L
        rc = self.lib.gccnmf_klnmf_stage(self.Vd.data_ptr(), self.Wd.data_ptr(), self.Hd.data_ptr(), self.ws.data_ptr(), L.F, L.N, L.K, L.B,
                                         float(S.ALPHA), float(S.EPS), self.flags, stage, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, 'stage %d returned %d' % (stage, rc)
        was, now = self.state, self.snapshot()
        self.state = now
        for name in self.names:
            if name not in owned:
                same = _bits(now[name]) == _bits(was[name])
                assert same.all(), '%s: stage %d changed %s at %s (it does not own it)' % (self.label, stage, name, tuple(np.argwhere(~same)[0]))
        for name, rows, cols in (('W', L.F, L.K), ('H', L.K, L.N), ('R', L.F, L.N)) + ((('Rt', L.N, L.F),) if self.form.direct else ()):
            a = now[name]
            assert not _bits(a[:, rows:, :]).any() and not _bits(a[:, :, cols:]).any(), '%s: stage %d left non-zero padding in %s' % (self.label, stage, name)
        return was, now

    def within(self, stage, output, got, refs, bar):
        """got (B, ...) against the per-file references, element by element; prints the worst share of the bar first"""
        worst, misses = 0.0, []
        for b, ref in enumerate(refs):
            g = got[b][tuple(slice(0, n) for n in ref.shape)]
            w, miss = S.share(g, ref, bar)
            worst = max(worst, w)
            if miss is not None:
                misses.append('file %d element %s: %r, reference %r' % (b, miss, g[miss], ref[miss]))
        key = 'stage %d %s' % (stage, output)
        self.shares[key] = max(self.shares.get(key, 0.0), worst)
        print('%s: %s: worst share of the bar (%.1f * 2^-24) %.3f' % (self.label, key, bar / S.U24, worst))
        assert not misses, '%s: %s misses its bar of %.1f * 2^-24 relative: %s' % (self.label, key, bar / S.U24, '; '.join(misses[:4]))

    def files(self, st, *names):
        """per file, the valid corner of each named block of a state (what the restatement takes)"""
        L = self.L
        corner = dict(V=(L.F, L.N), W=(L.F, L.K), H=(L.K, L.N), R=(L.F, L.N), U=(L.F, L.K), colsumW=(L.K,), rowsumH=(L.K,), s=(L.K,))
        return [[st[n][b][tuple(slice(0, m) for m in corner[n])] for n in names] for b in range(L.B)]

    def zero_lines(self, st, stage, name, row=False, col=False):
        """the exact zeros of the silent bin (a row of R, U, W) and the silent frame (a column of R, H)"""
        width = self.L.N if name in ('R', 'Rt') else self.L.K               # (U's padding is nobody's operand: it keeps the workspace's bits)
        for b in range(self.L.B):
            f0, n0 = S.zero_lines(self.L.F, self.L.N, b)
            if row:
                assert not _bits(st[name][b, f0, :width]).any(), '%s: stage %d %s: the silent bin %d of file %d is not exactly zero' % (self.label, stage, name, f0, b)
            if col and n0 is not None:
                assert not _bits(st[name][b, :, n0]).any(), '%s: stage %d %s: the silent frame %d of file %d is not exactly zero' % (self.label, stage, name, n0, b)

    def restore_silent_frame(self, H_before):
        for b in range(self.L.B):
            n0 = S.zero_lines(self.L.F, self.L.N, b)[1]
            if n0 is not None:
                col = H_before[b, :self.L.K, n0]
                self.poke('H', b, (slice(0, self.L.K), n0), col)
                if self.form.direct:
                    self.poke('Ht', b, (n0, slice(0, self.L.K)), col)
        self.state = self.snapshot()

    def transposed_copy(self, stage, copy, of):
        now = self.state
        assert np.array_equal(_bits(now[copy]), _bits(now[of].transpose(0, 2, 1))), '%s: stage %d: %s is not the transpose of %s' % (self.label, stage, copy, of)

    # ---- the stages ----
    def stage0(self):
        L, d = self.L, self.form.direct
        was, now = self.stage(0, {'R', 'colsumW', 's'} | ({'Wt', 'Ht', 'Rt'} if d else set()))
        self.within(0, 'colsumW', now['colsumW'], [S.stage0(W)[0] for W, in self.files(was, 'W')], S.bar_colsum0(L.F))
        assert (now['s'][:, :L.K] == 1).all() and not _bits(now['R']).any(), '%s: stage 0: s is not 1 or R is not zero' % self.label
        if d:
            self.transposed_copy(0, 'Wt', 'W')
            assert not _bits(now['Ht']).any() and not _bits(now['Rt']).any()
        for b in range(L.B):
            self.poke('s', b, slice(0, L.K), self.s0[b])
        self.state = self.snapshot()

    def stage12(self):
        L, f = self.L, self.form
        if f.f12:
            was, now = self.stage(1, {'H'})
            self.within(1, 'H (K1 + K2)', now['H'], [S.fused12(*a) for a in self.files(was, 'V', 'W', 'H', 's', 'colsumW')], S.bar_H(L.F, L.K))
            self.zero_lines(now, 1, 'H', col=True)
            self.stage(2, set())
        else:
            was, now = self.stage(1, {'R'})
            self.within(1, 'R', now['R'], [S.stage1(*a) for a in self.files(was, 'V', 'W', 'H', 's')], S.bar_R(L.K))
            self.zero_lines(now, 1, 'R', row=True, col=True)
            was, now = self.stage(2, {'H'} | ({'Ht'} if f.direct else set()))
            self.within(2, 'H', now['H'], [S.stage2(*a) for a in self.files(was, 'W', 'H', 's', 'R', 'colsumW')], S.bar_H(L.F))
            self.zero_lines(now, 2, 'H', col=True)
            if f.direct:
                self.transposed_copy(2, 'Ht', 'H')
        self.restore_silent_frame(was['H'])

    def stage34(self):
        L, f = self.L, self.form
        if f.f34:
            was, now = self.stage(3, {'U', 'rowsumH'})
            refs = [S.fused34(*a) for a in self.files(was, 'V', 'W', 'H')]
            self.within(3, 'U (K3 + K4a)', now['U'], [r[0] for r in refs], S.bar_U(L.N, L.K))
            self.within(3, 'rowsumH (K3 + K4a)', now['rowsumH'], [r[1] for r in refs], S.bar_rowsumH(L.N))
            self.zero_lines(now, 3, 'U', row=True)
            self.stage(4, set())
            return
        was, now = self.stage(3, {'R', 'Rt'} if f.direct else {'R'})
        refs = [S.stage3(*a) for a in self.files(was, 'V', 'W', 'H')]
        if f.direct:
            # the direct K3 writes Rt [n][f], K4a's operand; of R itself only bin F - 1 (F = 16 n + 1), the rest keeps stage 1's values
            R_of_K4a = np.ascontiguousarray(now['Rt'].transpose(0, 2, 1))
            self.within(3, 'Rt', R_of_K4a, refs, S.bar_R(L.K))
            rows = np.arange(L.Fp) != (L.F - 1 if f.direct_tail else -1)
            assert np.array_equal(_bits(now['R'][:, rows]), _bits(was['R'][:, rows])), '%s: stage 3 changed R outside bin F - 1' % self.label
            if f.direct_tail:
                assert np.array_equal(_bits(now['R'][:, L.F - 1]), _bits(R_of_K4a[:, L.F - 1])), '%s: stage 3: bin F - 1 of R and of Rt differ' % self.label
            self.zero_lines(dict(Rt=R_of_K4a), 3, 'Rt', row=True, col=True)
        else:
            R_of_K4a = now['R']
            self.within(3, 'R', now['R'], refs, S.bar_R(L.K))
            self.zero_lines(now, 3, 'R', row=True, col=True)
        held = [(R_of_K4a[b, :L.F, :L.N], H) for b, (H,) in enumerate(self.files(now, 'H'))]
        if f.fw:
            was, now = self.stage(4, {'W', 'colsumW', 's'})
            refs = [S.fused_w(W, R, H) for (W,), (R, H) in zip(self.files(was, 'W'), held)]
            self.w_update(4, now, refs, L.N, ' (K4a + K4b)')
            self.stage(5, set())
            return
        was, now = self.stage(4, {'U', 'rowsumH'})
        refs = [S.stage4(R, H) for R, H in held]
        self.within(4, 'U', now['U'], [r[0] for r in refs], S.bar_U(L.N))
        self.within(4, 'rowsumH', now['rowsumH'], [r[1] for r in refs], S.bar_rowsumH(L.N))
        self.zero_lines(now, 4, 'U', row=True)

    def w_update(self, stage, now, refs, N, tag=''):
        L = self.L
        self.within(stage, 'W' + tag, now['W'], [r[0] for r in refs], S.bar_W(L.F, N))
        self.within(stage, 's' + tag, now['s'], [r[1] for r in refs], S.bar_s(L.F, N))
        self.within(stage, 'colsumW' + tag, now['colsumW'], [r[2] for r in refs], S.bar_colsumW(L.F, N))

    def stage5(self, lines=True):
        was, now = self.stage(5, {'W', 'colsumW', 's'} | ({'Wt'} if self.form.direct else set()))
        self.w_update(5, now, [S.stage5(*a) for a in self.files(was, 'W', 'U', 'rowsumH')], None)
        if lines:
            self.zero_lines(now, 5, 'W', row=True)
        if self.form.direct:
            self.transposed_copy(5, 'Wt', 'W')

    def stage6(self):
        L = self.L
        was, now = self.stage(6, {'H'})
        for b, (H, s) in enumerate(self.files(was, 'H', 's')):
            same = _bits(now['H'][b, :L.K, :L.N]) == _bits(S.stage6(H, s))
            assert same.all(), '%s: stage 6: H of file %d is not the float32 product H * s at %s' % (self.label, b, tuple(np.argwhere(~same)[0]))

    def summary(self):
        print('SHARES | %s | %s | %s' % (self.form, self.label, ' | '.join('%s %.3f' % kv for kv in sorted(self.shares.items()))))


def _run(F, N, K, B, flags=0, keys=None, want=None):
    """stages 0 ... 6 of one call shape under one tuning, every check of the module's docstring; `want`: the Form attributes the case means to reach"""
    keys = keys or {}
    form = Form(F, N, K, B, flags, keys)
    for attr, value in (want or {}).items():
        assert getattr(form, attr) == value, 'the case means %s = %s' % (attr, value)
    label = '(%d, %d, %d) x %d flags %#x keys %s [%s]' % (F, N, K, B, flags, keys, form)
    with _tuning(keys) as lib:
        assert lib.gccnmf_klnmf_plan(F, N, K, B, flags) & 7 == form.plan, '%s: gccnmf_klnmf_plan says %d' % (label, lib.gccnmf_klnmf_plan(F, N, K, B, flags))
        run = Run(lib, F, N, K, B, flags, form, label)
        run.stage0()
        run.stage12()
        run.stage34()
        if not form.fw:
            run.stage5()
        run.stage6()
        run.summary()
    return run


# ---- the direct latency kernels (csrc/direct.hip): the defaults, a handful of files -------------------------------------------------------------
#   (513, 70, 65)  F = 128 n + 1: the VALU tail bin, a ragged second column tile, a ragged second atom group
#   (145, 1, 1)    F = 16 n + 1 but not 128 n + 1; one frame, one atom
#   (17, 64, 64)   the smallest shape with the direct tail bin
#   (40, 65, 17)   no tail bin, Fp > F
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('F,N,K', S.DIRECT_SHAPES)
def test_direct_kernels(F, N, K, B):
    run = _run(F, N, K, B, want=dict(direct=True, direct_tail=F != 40))
    # stage 5 here: launch_update_w with B * (Kp / 64) < 256 and F <= 576 -> the one-pass kernel, 16 atoms per workgroup (not wide: B * Kp / 32 < 256)
    assert 'stage 5 W' in run.shares and 'stage 3 Rt' in run.shares


# ---- the small-batch tile (tuning key 2 = 2: 128 x 64 per workgroup, 128 x 256 for outputs of at most 128 rows) ------------------------------------
#   K1 / K3 / K4a take the tail bin only at (513, 70, 65); K2 takes its rank-1 term at 513, 145 and 17 (F = 16 n + 1)
#   stage 5: the one-pass 16-atom kernel, as above
@pytest.mark.parametrize('F,N,K', S.DIRECT_SHAPES)
def test_small_batch_tile(F, N, K):
    run = _run(F, N, K, 2, keys={2: 2, 10: 0}, want=dict(direct=False, f12=False, f34=False, fw=False))
    assert 'stage 4 U' in run.shares and 'stage 5 W' in run.shares


# ---- the throughput tile (tuning key 2 = 1: 512 x 64) -----------------------------------------------------------------------------------------------
#   (513, 96, 65)    the last column tile has exactly 32 columns: the narrow item
#   (513, 97, 65)    33 columns: not narrow
#   (641, 96, 70)    Fm = 640 > 512: no fused W update; F > 576: launch_update_w takes nmf_update_w_kernel<16> (B * Kp / 64 < 256), not the one-pass kernel
#   (200, 130, 130)  no tail bin, outputs of at most 256 rows (half-height), three atom groups with a ragged last one
# The W update rides the R.H^T epilogue at F = 513 and F = 200 unless flag 2 is set (then stage 5 is the one-pass 16-atom kernel).  At THESE
# shapes it is the REGISTER-STAGED kernel's epilogue whatever key 3 says: the LDS-DMA kernel carries it only for Fm a multiple of 128 AND K a
# multiple of 64 (launch_rht_update_w), and K = 65 / F = 200 are neither.  test_w_update_in_the_lds_dma_epilogue below is the LDS-DMA one.
# S.throughput_cases says how the knob values are laid over the shapes (all four values of key 9 where it acts: with key 3 = 1).
@pytest.mark.parametrize('F,N,K,B,flags,dma,split', S.throughput_cases())
def test_throughput_tile(F, N, K, B, flags, dma, split):
    fw = F != 641 and not flags & 2
    run = _run(F, N, K, B, flags, keys={2: 1, 3: dma, 9: split}, want=dict(direct=False, f12=False, f34=False, fw=fw, dma_updw=False))
    assert ('stage 4 W (K4a + K4b)' if fw else 'stage 5 W') in run.shares


# (513, 96, 128): Fm = 512 = 4 * 128 and K = 2 * 64 -> with key 3 = 1 gccnmf_launch_gemm_dma<.., EPI_UPDW> -- what a batch at scale runs for
# K > 128 at F = 513, and what the chained launches are pinned to bit for bit; with key 3 = 0 the register-staged epilogue on the same
# problem.  Batch 9: the XCD-affine block map.  The last column tile has 32 columns (the narrow item of K1 / K3).
@pytest.mark.parametrize('B', [2, 9])
@pytest.mark.parametrize('dma', [1, 0])
def test_w_update_in_the_lds_dma_epilogue(dma, B):
    F, N, K = S.DMA_UPDW_SHAPE
    run = _run(F, N, K, B, 0, keys={2: 1, 3: dma}, want=dict(direct=False, f12=False, f34=False, fw=True, dma_updw=dma == 1))
    assert 'stage 4 W (K4a + K4b)' in run.shares and 'stage 5 W' not in run.shares


# ---- the smallest chain-capable shapes (S.CHAIN_SHAPES: F in {257, 385, 513}, K a multiple of 128 from 256 on) on the plain launches -------------------
# What the chained and ragged launches are pinned to bit for bit at these shapes (tests/test_gpu_chained_small_shapes.py), here element by element:
#   (257, 70, 256)  K2 on half-height tiles (256 rows); the fused W update at Fm = 256 with four atom tiles
#   (385, 96, 384)  K2's 384 rows: one row tile; Fm = 384; the last column tile of exactly 32 columns; six atom tiles
#   (513, 33, 640)  K2's 640 rows: two row tiles; ONE column tile; K1 / K3 with a reduction of 640; ten atom tiles
# Key 9 decides the item form of K1 / K2 / K3 in the LDS-DMA launcher: 1 (default) prices a launch this small onto half-height tiles; 0 is full-height
# wide tiles only -- K2 at K > 256 as a chained launch runs it --; 2 every tile as two narrow halves of a full-height tile.  The first two (dma, split)
# pairs are the default form in both staging kernels, the last two the full-height forms.  The W update rides the LDS-DMA epilogue with key 3 = 1
# (Fm a multiple of 128, K of 64), the register-staged kernel's with key 3 = 0.
@pytest.mark.parametrize('B', [2, 9])
@pytest.mark.parametrize('dma,split', [(1, 1), (0, 1), (1, 0), (1, 2)])
@pytest.mark.parametrize('F,N,K', S.CHAIN_SHAPES)
def test_chain_capable_shapes_on_the_plain_launches(F, N, K, dma, split, B):
    keys = {2: 1, 3: dma} if split == 1 else {2: 1, 3: dma, 9: split}
    run = _run(F, N, K, B, 0, keys=keys, want=dict(direct=False, f12=False, f34=False, fw=True, dma_updw=dma == 1))
    assert {'stage 1 R', 'stage 2 H', 'stage 3 R', 'stage 4 W (K4a + K4b)'} <= set(run.shares) and 'stage 5 W' not in run.shares


# ---- short dictionaries: K1 + K2 and K3 + K4a as one launch each (tuning keys 16 / 17 = 2; key 10 = 0 keeps two files off the direct kernels) -------
#   (129, 65, 20), (513, 1, 128), (513, 130, 128), (257, 64, 33): both launches exist.  (129, 65, 33) is the shape the slab launch refuses -- its
#   Fm / 64 = 2 slabs hold 2 * 16 = 32 atoms' worth of U columns, 32 * ceil(33 / 32) = 64 are needed -- so with key 17 = 2 the plan bit stays clear
#   and the case checks the two launches.  (At (257, 64, 33) it is 4 * 16 = 64 >= 64: not refused.)  Form restates the rule; the plan is asserted.
@pytest.mark.parametrize('B', [2, 5])
@pytest.mark.parametrize('k16,k17', [(2, 2), (2, 0), (0, 2)])
@pytest.mark.parametrize('F,N,K', S.SHORT_SHAPES)
def test_short_dictionary_fused_launches(F, N, K, k16, k17, B):
    slabs_hold_K = ((F - 1) // 64) * 16 >= 32 * -(-K // 32)
    run = _run(F, N, K, B, keys={10: 0, 16: k16, 17: k17}, want=dict(direct=False, f12=k16 == 2, f34=k17 == 2 and slabs_hold_K, fw=False))
    assert ('stage 1 H (K1 + K2)' if k16 == 2 else 'stage 2 H') in run.shares
    assert ('stage 3 U (K3 + K4a)' if k17 == 2 and slabs_hold_K else 'stage 4 U') in run.shares


# ---- the W-update kernels a batch at scale takes, at small shapes: stage 5 alone ----------------------------------------------------------------------
# GCCNMF_FLAG_GROUPS(n) sizes the launch as B * n files (launch_update_w's `sized`); K = 50 -> Kp = 64, a ragged 32-atom / 64-atom group.
#   n = 64:  sized = 128: sized * Kp / 64 < 256 and F <= 576 -> one pass; K <= 128 and sized * Kp / 32 = 256 >= 256 -> nmf_update_w_onepass_kernel<32>
#   n = 128: sized = 256: sized * Kp / 64 >= 256 -> nmf_update_w_kernel<64>
# flag 2 keeps stage 5 a launch of its own at F = 513, n = 128 (the launch size alone would put the W update into stage 4's epilogue); keys 16 /
# 17 = 0 keep the short-dictionary cost model out of it.  U and rowsumH are written by the test: positive, U with the silent bin's zero row.
@pytest.mark.parametrize('n', [64, 128])
@pytest.mark.parametrize('F,N,K', S.UPDATE_W_SHAPES)
def test_batch_scale_w_update_kernels(F, N, K, n):
    B, flags, keys = 2, GROUPS(n) | UNFUSED_W_UPDATE, {16: 0, 17: 0}
    form = Form(F, N, K, B, flags, keys)
    assert not form.direct and not form.fw and not form.f34
    label = '(%d, %d, %d) x %d as %d files [stage 5 alone]' % (F, N, K, B, B * n)
    with _tuning(keys) as lib:
        run = Run(lib, F, N, K, B, flags, form, label)
        run.stage0()
        rng = np.random.RandomState(n + F)
        for b in range(B):
            U = (rng.rand(F, K) + 0.01).astype(np.float32)
            U[S.zero_lines(F, N, b)[0]] = 0
            run.poke('U', b, (slice(0, F), slice(0, K)), U)
            run.poke('rowsumH', b, slice(0, K), (rng.rand(K) * N + 0.5).astype(np.float32))
        run.state = run.snapshot()
        run.stage5()
        run.summary()
