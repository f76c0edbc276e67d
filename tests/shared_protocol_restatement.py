"""What each call of the shared-dictionary KL-NMF protocol (include/gccnmf_hip.h: gccnmf_klnmf_shared_begin / _step_a / _step_b / _finish and
the one-call gccnmf_klnmf_shared_run) must leave, as a function of the state before it: the reference for
tests/test_shared_protocol_host.py and tests/test_gpu_shared_protocol.py.  Plain NumPy, no GPU.

Every reference and every bar is tests/klnmf_stages_restatement.py's (S below: stage0 ... stage6, fused12, the bar functions, share), and its
rule applies: a comparison takes the float32 values the device held BEFORE the call, a reference of exactly 0 demands exactly 0, every
check prints its worst share of the bar before it asserts.  No tolerance is stated here: a check is one of S's bars or bit-for-bit equality.

    begin    colsumW = stage0(W), hscale = 1, all of R zero (a single-file shard: also Wt, Ht, Rt zero)
    step A   H         fused12(V, W, H, hscale, colsumW)            bar_H(F, K): K1's R is overwritten by K3's before the call returns,
                                                                     so the H update is observable only as the composition
             R         stage3(V, W, H after)                        bar_R(K)     (a direct shard: R is what Rt holds, transposed)
             Upart     stage4(R after, H after)[0], per file        bar_U(N)
             rowsum    stage4(R after, H after)[1], per file        bar_rowsumH(N)
             partial   num = float32 sum of the device's Upart, den of its rowsum_part: per shard s = 0; s += part[b] over the files in
                       ascending order, then partial = s for the first shard and partial + s for every later one.  Additions only, no
                       product to contract: BIT FOR BIT.
    step B   W, hscale, colsumW = stage5(W, num, den)               bar_W(F), bar_s(F), bar_colsumW(F)
    finish   H = stage6(H, hscale) BIT FOR BIT (one rounding per element), then hscale = 1

The state the checks take is LOGICAL -- valid corners only, one array per file:
    dict(W (F, K), colsumW (K,), hscale (K,), num (F, K), den (K,),
         shards = [dict(V = [(F, N)] * batch, H = [(K, N)] * batch, R = [(F, N)] * batch, U = [(F, K)] * batch, rowsum = [(K,)] * batch)])
so the same check_* functions judge the float32 NumPy emulation of the host test (and its wrong variants: the checks have teeth) and the
device.  What is not logical -- padding, ownership of every buffer, the workspace layout -- is `Shard` below and the GPU test's.

The problems are S.problem(..., frames=False): the silent bin and the isolated zeros, not the silent frame -- step A runs K2 then K3 with no
chance to restore the frame's column of H in between, so a zero column would be 0 / 0 in K3 (in the reference too).  Every file has its
silent bin at a row of its own (S.zero_lines), so with ONE dictionary for several files num[f0] is a sum over all files and stays positive:
W keeps that row, a second iteration meets the silent bins again, and every multi-file case -- the one-call run's included -- keeps them.
The one exception is a case that has a SINGLE file in total and runs a second iteration ('one column block of pitch Np'): there the first W
update makes that bin's row of W exactly 0, as it must, and the second step A divides V = 0 by W.H = 0 in the whole bin -- NaN in the reference
and on the device alike, and through W^T.R in every element of H.  That case alone takes lines=False (the isolated exact zeros stay)."""
import re

import numpy as np

import klnmf_stages_restatement as S

f32 = np.float32
SPLITS = 4                                   # GCCNMF_SPLITS (csrc/nmf.hip): room the lab build's split reductions use in a single-file shard
DEFAULT_KEYS = {2: 0, 3: 1, 8: 3, 10: 1}     # the tuning keys the cases touch: tile policy, LDS-DMA, file groups, direct kernels


def _up(n, m):
    return -(-n // m) * m


def partial_floats(F, K):
    """partial = num [Fp][Kp] | den [Kp]"""
    return _up(F, 16) * _up(K, 64) + _up(K, 64)


class Shard(object):
    """One gccnmf_shared_shard: `batch` files of N columns, whole padded matrices back to back (ld = 0: V [batch][Fp][Np], H [batch][Kp][Np])
    or column blocks of one matrix of row pitch ld (file b = columns [col0 + b N, col0 + b N + N) of V [Fp][ld], H [Kp][ld]; col0 is where
    the caller pointed V and H, the library does not know it) -- and where its scratch lies, in floats from the shard's workspace:
        R [batch][Fp][Np]  (ld > 0: [Fp][ld], file b at columns [b N, b N + N): NOT offset by col0)
        Upart [batch][Fp][Kp] | rowsum_part [batch][Kp]
        a single-file shard in the plain layout (batch = 1, and ld == 0 or ld == Np):  SPLITS (max(Fp Np, Fp Kp) + Kp) floats of split scratch, then
        Wt [Kp][Fp] | Ht [Np][Kp] | Rt [Np][Fp]
        `vectors` (the four-call workspace; gccnmf_klnmf_shared_run takes them as its caller's `vec`):  colsumW [Kp] | hscale [Kp]"""

    def __init__(self, F, K, N, batch, ld=0, col0=0, vectors=False):
        self.F, self.K, self.N, self.batch, self.ld, self.col0 = F, K, N, batch, ld, col0
        self.Fp, self.Kp, self.Np = _up(F, 16), _up(K, 64), _up(N, 64)
        Fp, Kp, Np = self.Fp, self.Kp, self.Np
        assert ld == 0 or (ld % 4 == 0 and col0 + batch * N <= ld and col0 + (batch - 1) * N + Np <= ld and (batch == 1 or N % 64 == 0))
        self.single = batch == 1 and ld in (0, Np)
        blocks = [('R', (Fp, ld) if ld else (batch, Fp, Np)), ('Upart', (batch, Fp, Kp)), ('rowsum_part', (batch, Kp))]
        if self.single:
            blocks += [('split', (SPLITS * (max(Fp * Np, Fp * Kp) + Kp),)), ('Wt', (Kp, Fp)), ('Ht', (Np, Kp)), ('Rt', (Np, Fp))]
        if vectors:
            blocks += [('colsumW', (Kp,)), ('hscale', (Kp,))]
        self.blocks, at = {}, 0
        for name, shape in blocks:
            self.blocks[name] = (at, shape)
            at += int(np.prod(shape))
        self.floats = at

    def view(self, ws, name):
        at, shape = self.blocks[name]
        return ws[at:at + int(np.prod(shape))].reshape(shape)

    # ---- which launches the shard takes, restated by hand from make_shard / shared_step_a_all (csrc/nmf.hip) ----
    def direct(self, keys=None):
        """the direct-to-register kernels: a single-file shard in the plain layout under key 10 = 1, key 2 = 0 (one file <= key 12, always)"""
        k = dict(DEFAULT_KEYS)
        k.update(keys or {})
        return self.single and bool(k[10]) and k[2] == 0

    def direct_tail(self, keys=None):
        return self.direct(keys) and self.F > 16 and self.F % 16 == 1

    def groups(self, keys=None):
        """file groups step A deals the shard into: tiles = batch ceil(N / 64); 1 if tiles >= 512 else clamp(tiles // 64, 1, min(batch, key 8))"""
        k = dict(DEFAULT_KEYS)
        k.update(keys or {})
        tiles = self.batch * -(-self.N // 64)
        return 1 if tiles >= 512 else max(1, min(tiles // 64, self.batch, k[8]))

    def group_files(self, keys=None):
        g = self.groups(keys)
        return [(self.batch * q // g, self.batch * (q + 1) // g) for q in range(g)]

    # ---- a file's part of the arrays as the device holds them ----
    def file_of(self, a, b, of_R=False):
        """file b's rows x N valid columns of V / H (or, of_R, of R) as laid out for this shard"""
        if not self.ld:
            return a[b][:, :self.N]
        c = (0 if of_R else self.col0) + b * self.N
        return a[:, c:c + self.N]

    def valid(self, shape, rows, of_R=False):
        """boolean mask of the elements of a V / H / R array of `shape` that belong to this shard's files (everything else is padding, or
        another shard's)"""
        m = np.zeros(shape, bool)
        if not self.ld:
            m[:, :rows, :self.N] = True
        else:
            c = 0 if of_R else self.col0
            m[:rows, c:c + self.batch * self.N] = True
        return m


class Case(object):
    """One rank's training: F, K, its shards (N, batch, col0) -- of one matrix of pitch `ld`, or plain (ld = 0) --, the tuning keys, and what
    the case is in the table for (`claims`: checked by the host test against Shard.direct / .groups, so the table reaches what it says)."""

    def __init__(self, name, F, K, shards, ld=0, keys=None, claims=None, iterations=2):
        self.name, self.F, self.K, self.ld, self.keys, self.claims = name, F, K, ld, dict(keys or {}), dict(claims or {})
        self.iterations = iterations
        self.spec = list(shards)
        assert len({N for N, _, _ in self.spec}) == len(self.spec), 'S.problem seeds by (F, N, K): shards of one case need different N'

    def shards(self, vectors=False):
        return [Shard(self.F, self.K, N, batch, self.ld, col0, vectors) for N, batch, col0 in self.spec]

    @property
    def id(self):
        """the pytest id of the case"""
        keys = ' '.join('key%d=%d' % kv for kv in sorted(self.keys.items()))
        return re.sub('[^0-9A-Za-z=]+', '-', self.name + ' ' + keys).strip('-')

    @property
    def files(self):
        return sum(batch for _, batch, _ in self.spec)

    def __str__(self):
        return '%s F=%d K=%d %s ld=%d keys %s' % (self.name, self.F, self.K, ' + '.join('%d x N=%d' % (b, N) for N, b, _ in self.spec), self.ld, self.keys)

    def problem(self):
        """the logical state before `begin` (colsumW, hscale, num, den, R, U, rowsum: not yet anyone's) and the lazy scale to poke after it"""
        shards = []
        _, Ws, _, ss = S.problem(self.F, 64, self.K, 1, lines=False)   # (a rank without columns still holds the dictionary)
        W, s = (Ws[0], ss[0]) if not self.spec else (None, None)
        for N, batch, _ in self.spec:
            V, Ws, H, ss = S.problem(self.F, N, self.K, batch, lines=self.iterations == 1 or self.files > 1, frames=False)
            if W is None:
                W, s = Ws[0], ss[0]
            shards.append(dict(V=list(V), H=list(H)))
        return dict(W=W, shards=shards), s


def _four(F, N, K, B, keys=None, **claims):
    return Case('four calls (%d, %d, %d) x %d' % (F, N, K, B), F, K, [(N, B, 0)], 0, keys, claims, 1)


# ---- (a) the four calls, plain layout: the smallest shapes at which the kernels change form (S.DIRECT_SHAPES / S.THROUGHPUT_SHAPES) ------------
FOUR_CALL_CASES = (
    # defaults, one file: the direct kernels, Wt re-transposed every step A, the transposed copies behind the split scratch
    [_four(F, N, K, 1, direct=True) for F, N, K in [(513, 70, 65), (17, 64, 64), (40, 65, 17)]]
    # defaults, three files: the small-batch tile with a stride-0 W
    + [_four(F, N, K, 3, direct=False) for F, N, K in [(513, 96, 65), (200, 130, 130), (145, 1, 1)]]
    # key 2 = 1: the throughput tile, LDS-DMA (key 3 = 1) and register-staged (0); 9 files: the XCD-affine block map with ONE shared W
    + [_four(F, N, K, B, {2: 1, 3: dma}, direct=False) for dma in (1, 0) for B in (2, 9) for F, N, K in [(513, 96, 65), (513, 97, 65), (200, 130, 130)]]
    # F > 576: step B on nmf_update_w_kernel<16> instead of the one-pass kernel
    + [_four(641, 96, 70, 2, {2: 1}, direct=False)])

# ---- (b) the one-call run: the forms only gccnmf_klnmf_shared_run reaches --------------------------------------------------------------------------
COLUMN_BLOCKS = [(64, 3, 0), (37, 1, 192)]          # one [Fp][256] matrix of 229 columns: three blocks of 64 and the ragged remainder


def _column_blocks(keys=None):
    return Case('column blocks', 513, 65, COLUMN_BLOCKS, 256, keys, dict(direct=False, ld_batch=True, ragged_ld=True))


RUN_CASES = [
    _column_blocks(), _column_blocks({2: 1, 3: 1}), _column_blocks({2: 1, 3: 0}),
    Case('one column block of pitch Np', 513, 65, [(70, 1, 0)], 128, None, dict(direct=True)),
    Case('two plain shards', 200, 130, [(70, 2, 0), (130, 3, 0)], 0, None, dict(direct=False, two_widths=True)),
    Case('two file groups', 145, 20, [(512, 16, 0)], 0, None, dict(groups=2)),
    Case('three file groups', 145, 20, [(1024, 12, 0)], 0, None, dict(groups=3)),
    Case('one group by key 8', 145, 20, [(1024, 12, 0)], 0, {8: 1}, dict(groups=1)),
]
NO_COLUMNS = Case('a rank without columns', 513, 65, [])
CROSS_CHECK = Case('run against four calls (513, 96, 65) x 3', 513, 65, [(96, 3, 0)], 0, None, dict(direct=False))    # the hook's states in a plain-layout run are bit for bit the four calls'
ALL_CASES = FOUR_CALL_CASES + RUN_CASES


# ---- the checks ------------------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


class Report(object):
    """prints every check's worst share of its bar (or its count of differing words) before it asserts; keeps the worst per output"""

    def __init__(self, label):
        self.label, self.shares = label, {}

    def within(self, what, gots, refs, bar):
        worst, misses = 0.0, []
        for b, (g, ref) in enumerate(zip(gots, refs)):
            assert np.shape(g) == np.shape(ref), '%s: %s: shapes %s / %s' % (self.label, what, np.shape(g), np.shape(ref))
            w, miss = S.share(g, ref, bar)
            worst = max(worst, w)
            if miss is not None:
                misses.append('file %d element %s: %r, reference %r' % (b, miss, np.asarray(g)[miss], np.asarray(ref)[miss]))
        key = what.split(' [')[0]
        self.shares[key] = max(self.shares.get(key, 0.0), worst)
        print('%s: %s: worst share of the bar (%.1f * 2^-24) %.3f' % (self.label, what, bar / S.U24, worst))
        assert not misses, '%s: %s misses its bar of %.1f * 2^-24 relative: %s' % (self.label, what, bar / S.U24, '; '.join(misses[:4]))

    def same(self, what, gots, wants):
        differ, first = 0, None
        for b, (g, w) in enumerate(zip(gots, wants)):
            assert np.shape(g) == np.shape(w), '%s: %s: shapes %s / %s' % (self.label, what, np.shape(g), np.shape(w))
            d = _bits(g) != _bits(w)
            differ += int(d.sum())
            if d.any() and first is None:
                i = tuple(int(j) for j in np.argwhere(d)[0])
                first = 'file %d element %s: %r, wanted %r' % (b, i, np.asarray(g)[i], np.asarray(w)[i])
        print('%s: %s: %d words differ (bit for bit)' % (self.label, what, differ))
        assert not differ, '%s: %s is not bit for bit what it must be: %d words differ, first %s' % (self.label, what, differ, first)

    def summary(self, form):
        print('SHARES | %s | %s | %s' % (form, self.label, ' | '.join('%s %.3f' % kv for kv in sorted(self.shares.items()))))


def check_begin(rep, before, after, R=True):
    """R=False: `after` was taken later than begin's return (the run's first hook), when R is step A's"""
    F = before['W'].shape[0]
    rep.within('begin colsumW', [after['colsumW']], [S.stage0(before['W'])[0]], S.bar_colsum0(F))
    rep.same('begin hscale = 1', [after['hscale']], [np.ones_like(after['hscale'])])
    for i, sh in enumerate(after['shards'] if R else []):
        rep.same('begin R = 0 [shard %d]' % i, sh['R'], [np.zeros_like(R) for R in sh['R']])


def file_order_sum(parts, prior=None):
    """the float32 sum nmf_reduce_files_kernel states: s = 0; s += parts[b] in ascending order; prior + s for a second, third ... shard"""
    s = np.zeros(np.shape(parts[0]), f32)
    for p in parts:
        s = s + np.asarray(p, f32)
    return s if prior is None else np.asarray(prior, f32) + s


def check_step_a(rep, before, after, tag='step A'):
    W, s, cs = before['W'], before['hscale'], before['colsumW']
    F, K = W.shape
    num = den = None
    for i, (was, now) in enumerate(zip(before['shards'], after['shards'])):
        N, at = was['V'][0].shape[1], ' [shard %d]' % i
        rep.within(tag + ' H' + at, now['H'], [S.fused12(V, W, H, s, cs) for V, H in zip(was['V'], was['H'])], S.bar_H(F, K))
        rep.within(tag + ' R' + at, now['R'], [S.stage3(V, W, H) for V, H in zip(was['V'], now['H'])], S.bar_R(K))
        refs = [S.stage4(R, H) for R, H in zip(now['R'], now['H'])]
        rep.within(tag + ' Upart' + at, now['U'], [r[0] for r in refs], S.bar_U(N))
        rep.within(tag + ' rowsum_part' + at, now['rowsum'], [r[1] for r in refs], S.bar_rowsumH(N))
        num, den = file_order_sum(now['U'], num), file_order_sum(now['rowsum'], den)
    if num is None:                                                   # a rank without columns contributes exact zeros
        num, den = np.zeros((F, K), f32), np.zeros(K, f32)
    rep.same(tag + ' partial num', [after['num']], [num])
    rep.same(tag + ' partial den', [after['den']], [den])


def check_step_b(rep, before, after, tag='step B'):
    F = before['W'].shape[0]
    Wr, sr, cr = S.stage5(before['W'], before['num'], before['den'])
    rep.within(tag + ' W', [after['W']], [Wr], S.bar_W(F))
    rep.within(tag + ' hscale', [after['hscale']], [sr], S.bar_s(F))
    rep.within(tag + ' colsumW', [after['colsumW']], [cr], S.bar_colsumW(F))


def check_finish(rep, before, after):
    for i, (was, now) in enumerate(zip(before['shards'], after['shards'])):
        rep.same('finish H = H * hscale [shard %d]' % i, now['H'], [S.stage6(H, before['hscale']) for H in was['H']])
    rep.same('finish hscale = 1', [after['hscale']], [np.ones_like(after['hscale'])])


def lazy_scale_of(rep, what, H_before, H_after, s_ref, bar):
    """gccnmf_klnmf_shared_run's last step B leaves its hscale nowhere (finish resets it).  It is still pinned: for every atom there must be ONE
    float32 s within `bar` of the reference such that H after = float32(H before * s) bit for bit in every file, every column.  -> that s."""
    K = len(s_ref)
    k0 = [int(np.argmax(H_before[0][k])) for k in range(K)]
    guess = np.array([np.float64(H_after[0][k, j]) / np.float64(H_before[0][k, j]) for k, j in enumerate(k0)]).astype(f32)
    found = np.zeros(K, bool)
    s = guess.copy()
    for d in range(-4, 5):
        cand = (guess.view(np.int32) + d).view(f32)                   # positive floats: the neighbours are the neighbouring bit patterns
        ok = np.ones(K, bool)
        for was, now in zip(H_before, H_after):
            ok &= (_bits(S.stage6(was, cand)) == _bits(now)).all(1)
        s[ok & ~found] = cand[ok & ~found]
        found |= ok
    print('%s: %d of %d atoms have one float32 scale that reproduces H bit for bit in every file' % (rep.label, int(found.sum()), K))
    assert found.all(), '%s: %s: no single float32 scale gives H of atom %d in every file' % (rep.label, what, int(np.argmin(found)))
    rep.within(what, [s], [s_ref], bar)
    return s
