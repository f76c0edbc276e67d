"""Every call of the shared-dictionary KL-NMF protocol through the C ABI -- gccnmf_klnmf_shared_begin / _step_a / _step_b / _finish one at a
time, and gccnmf_klnmf_shared_run observed through its all-reduce hook -- each element of each output against the float64 restatement of
that call (tests/shared_protocol_restatement.py: the references, the bars, the workspace layout, the case table) evaluated on the state the
device held BEFORE the call: one wrong bin, frame, atom or file cannot hide in a norm, and two ways of running the same wrong kernels
cannot agree their way past it.  tests/test_shared_protocol_host.py shows that float32 NumPy passes the same checks and six wrong variants do
not.

(a) _four_calls: the workspace holds arbitrary bits before begin, the padding of V, W and H is zero.  After begin hscale == 1 is asserted
and then replaced by values in [0.5, 2), so step A meets s != 1.  A synchronisation and a download after every call; besides the element
checks, everything a call does not own is bit for bit what it was -- V always, W in begin / step A / finish, H in begin / step B, partial
in step B, every workspace block the call is not listed for (the split scratch of a single-file shard among them) -- and the padding of
W, H and R (and Rt) is exactly zero.  On a direct shard R is observed through Rt; R itself holds K1's quotient (checked against stage 1:
there it IS observable) but for bin F - 1, which K3 rewrites; Wt and Ht are the transposes of W and of the new H bit for bit.

(b) _run: the library calls the hook on the host between step A and step B of every iteration; the hook synchronises, downloads everything
and records -- it asserts nothing (ctypes would swallow it), catches every exception and returns non-zero for it, and the test re-raises.
Two iterations: hook 1 is begin + step A on the initial state, hook 2 step B and step A on hook 1's state with the real hscale != 1, the
return step B and finish on hook 2's.  The last hscale is reset by finish before anyone can read it: it is pinned through H
(restatement.lazy_scale_of).  Every file of every multi-file case has its silent bin, in both iterations (the files' bins are different rows,
so the shared W keeps them): the column blocks, the ragged remainder, the shard-order sums and the file groups all meet exactly-zero rows
of V, R and Upart, where the reference demands exactly 0.

Every check prints its worst share of the bar before it asserts; DESIGN section 2b records the figures."""
import contextlib

import numpy as np
import pytest
import torch

import klnmf_stages_restatement as S
import shared_protocol_restatement as P

pytestmark = pytest.mark.gpu

ALPHA, EPS = float(S.ALPHA), float(S.EPS)


def _hip():
    from gcc_nmf_amd import _hip
    return _hip


@contextlib.contextmanager
def _tuning(keys):
    lib = _hip().lib()
    try:
        for k, v in keys.items():
            assert lib.gccnmf_set_tuning(k, v) == 0, 'gccnmf_set_tuning(%d, %d) was refused: a product key, which every build accepts' % (k, v)
        yield lib
    finally:
        for k in keys:
            lib.gccnmf_set_tuning(k, P.DEFAULT_KEYS[k])


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _arbitrary(n, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(1, 1 << 30, n).astype(np.int32)).cuda().view(torch.float32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Device(object):
    """A case on the device: V, H, W with zero padding, every workspace, partial (and the run's vec) holding arbitrary bits."""

    def __init__(self, lib, case, four):
        self.lib, self.case, self.four, self.keys = lib, case, four, case.keys
        self.shards = case.shards(vectors=four)
        self.st0, self.s0 = case.problem()
        F, K = case.F, case.K
        self.Fp, self.Kp = P._up(F, 16), P._up(K, 64)
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device='cuda')
        up = lambda a: torch.from_numpy(np.array(a)).cuda()
        self.t = {'W': z(self.Fp, self.Kp)}
        self.t['W'][:F, :K] = up(self.st0['W'])
        if case.ld:
            self.t['V'], self.t['H'] = z(self.Fp, case.ld), z(self.Kp, case.ld)
        for i, (sh, files) in enumerate(zip(self.shards, self.st0['shards'])):
            if not case.ld:
                self.t['V%d' % i], self.t['H%d' % i] = z(sh.batch, self.Fp, sh.Np), z(sh.batch, self.Kp, sh.Np)
            for b in range(sh.batch):
                sh.file_of(self.t[self.Vn(i)], b)[:F] = up(files['V'][b])
                sh.file_of(self.t[self.Hn(i)], b)[:K] = up(files['H'][b])
            want = (lib.gccnmf_klnmf_shared_workspace_floats(F, sh.N, K, sh.batch) if four else
                    lib.gccnmf_klnmf_shared_shard_workspace_floats(F, sh.N, K, sh.batch, sh.ld))
            assert want == sh.floats, 'the layout of shard %d adds up to %d floats, the library says %d' % (i, sh.floats, want)
            self.t['ws%d' % i] = _arbitrary(sh.floats, 1 + i)
        assert lib.gccnmf_klnmf_shared_partial_floats(F, K) == P.partial_floats(F, K)
        self.t['partial'] = _arbitrary(P.partial_floats(F, K), 11)
        if not four:
            self.t['vec'] = _arbitrary(2 * self.Kp, 12)
        self.inputs = [n for n in self.t if n[0] in 'VH']

    def Vn(self, i):
        return 'V' if self.case.ld else 'V%d' % i

    def Hn(self, i):
        return 'H' if self.case.ld else 'H%d' % i

    def ptr(self, name, i=None):
        """the address a shard's V / H starts at (column col0 of the one matrix, or the shard's own tensor), or a tensor's"""
        if i is None:
            return self.t[name].data_ptr()
        return self.t[(self.Vn if name == 'V' else self.Hn)(i)].data_ptr() + 4 * self.shards[i].col0

    def snapshot(self):
        """name -> array of everything on the device: W, partial, colsumW, hscale, V / H (one matrix or per shard), every workspace block per shard"""
        torch.cuda.synchronize()
        raw = {n: self.t[n].cpu().numpy() for n in ['W', 'partial'] + self.inputs}
        for i, sh in enumerate(self.shards):
            ws = self.t['ws%d' % i].cpu().numpy()
            for name in sh.blocks:
                raw[name if name in ('colsumW', 'hscale') else '%s%d' % (name, i)] = sh.view(ws, name)
        if not self.four:
            vec = self.t['vec'].cpu().numpy()
            raw['colsumW'], raw['hscale'] = vec[:self.Kp], vec[self.Kp:]
        return raw

    def logical(self, raw):
        """the valid corners, per file (restatement: the state the checks take); a direct shard's R is what Rt holds"""
        F, K, Fp, Kp = self.case.F, self.case.K, self.Fp, self.Kp
        st = dict(W=raw['W'][:F, :K], colsumW=raw['colsumW'][:K], hscale=raw['hscale'][:K],
                  num=raw['partial'][:Fp * Kp].reshape(Fp, Kp)[:F, :K], den=raw['partial'][Fp * Kp:][:K], shards=[])
        for i, sh in enumerate(self.shards):
            files = range(sh.batch)
            if sh.direct(self.keys):
                R = [raw['Rt%d' % i].T[:F, :sh.N]]
            else:
                R = [sh.file_of(raw['R%d' % i], b, of_R=True)[:F] for b in files]
            st['shards'].append(dict(V=[sh.file_of(raw[self.Vn(i)], b)[:F] for b in files], H=[sh.file_of(raw[self.Hn(i)], b)[:K] for b in files],
                                     R=R, U=[raw['Upart%d' % i][b, :F, :K] for b in files], rowsum=[raw['rowsum_part%d' % i][b, :K] for b in files]))
        return st

    # ---- what each call owns (everything else must keep its bits) ----
    def owned(self, call):
        own = set()
        for i, sh in enumerate(self.shards):
            copies = {'Wt%d' % i, 'Ht%d' % i, 'Rt%d' % i}
            if call == 'begin':
                own |= {'R%d' % i} | (copies if sh.single else set())
            elif call == 'step A':
                own |= {self.Hn(i), 'R%d' % i, 'Upart%d' % i, 'rowsum_part%d' % i} | (copies if sh.direct(self.keys) else set())
            elif call == 'finish':
                own |= {self.Hn(i)}
        return own | {'begin': {'colsumW', 'hscale'}, 'step A': {'partial'}, 'step B': {'W', 'colsumW', 'hscale'}, 'finish': {'hscale'}}[call]

    def kept(self, label, what, was, now, calls):
        """everything none of `calls` owns is bit for bit what it was; the padding of W, H, R (and Rt) is exactly zero"""
        own = set().union(*[self.owned(c) for c in calls])
        assert not own & {n for n in now if n[0] == 'V'}
        for name in now:
            if name not in own:
                same = _bits(now[name]) == _bits(was[name])
                assert same.all(), '%s: %s changed %s at %s (it does not own it)' % (label, what, name, tuple(np.argwhere(~same)[0]))
        F, K = self.case.F, self.case.K
        pads = [('W', np.pad(np.ones((F, K), bool), ((0, self.Fp - F), (0, self.Kp - K))))]
        for i, sh in enumerate(self.shards):
            pads.append(('R%d' % i, sh.valid(now['R%d' % i].shape, F, of_R=True)))
            if sh.direct(self.keys):
                pads.append(('Rt%d' % i, np.pad(np.ones((sh.N, F), bool), ((0, sh.Np - sh.N), (0, self.Fp - F)))))
            if not self.case.ld:
                pads.append((self.Hn(i), sh.valid(now[self.Hn(i)].shape, K)))
        if self.case.ld and self.shards:                     # one matrix: what belongs to no shard's files -- the columns >= 229 of the case -- is padding
            pads.append(('H', np.any([sh.valid(now['H'].shape, K) for sh in self.shards], axis=0)))
        for name, valid in pads:
            stray = _bits(now[name]).astype(bool) & ~valid
            assert not stray.any(), '%s: %s left non-zero padding in %s at %s' % (label, what, name, tuple(np.argwhere(stray)[0]))

    def direct_copies(self, rep, what, was, now):
        """a direct shard after step A: Wt = W^T and Ht = (the new H)^T bit for bit; R = K1's quotient but for bin F - 1, which is K3's (= Rt's)"""
        F, K = self.case.F, self.case.K
        for i, sh in enumerate(self.shards):
            if not sh.direct(self.keys):
                continue
            H = now[self.Hn(i)] if self.case.ld else now[self.Hn(i)][0]
            rep.same(what + ' Wt = W^T', [now['Wt%d' % i]], [now['W'].T])
            rep.same(what + ' Ht = H^T', [now['Ht%d' % i]], [H.T])
            lw, ln = self.logical(was), self.logical(now)
            R = sh.file_of(now['R%d' % i], 0, of_R=True)[:F]
            k1 = S.stage1(lw['shards'][i]['V'][0], lw['W'], lw['shards'][i]['H'][0], lw['hscale'])
            rows = np.arange(F) != (F - 1 if sh.direct_tail(self.keys) else -1)
            rep.within(what + ' R of K1 (direct)', [R[rows]], [k1[rows]], S.bar_R(K))
            if sh.direct_tail(self.keys):
                rep.same(what + ' R bin F - 1 = Rt', [R[F - 1]], [ln['shards'][i]['R'][0][F - 1]])

    def form(self):
        return ', '.join('direct' if sh.direct(self.keys) else '%d file group%s%s' % (sh.groups(self.keys), 's'[:sh.groups(self.keys) > 1],
                                                                                 ' of column blocks' if sh.ld else '') for sh in self.shards) or 'no shard'


# ---- (a) the four calls, one at a time --------------------------------------------------------------------------------------------------------------
def _four_calls(case, poke=True, iterations=1):
    """-> (the states after each step A, the final state) for the cross-check; every check of the module docstring on the way when `poke`"""
    (N, B, _), F, K = case.spec[0], case.F, case.K
    seen = []
    with _tuning(case.keys) as lib:
        dev = Device(lib, case, four=True)
        label, sh = str(case), dev.shards[0]
        rep = P.Report(label)
        W, ws, partial, V, H = dev.ptr('W'), dev.ptr('ws0'), dev.ptr('partial'), dev.ptr('V', 0), dev.ptr('H', 0)

        def call(name, rc, was):
            assert rc == 0, '%s: %s returned %d' % (label, name, rc)
            now = dev.snapshot()
            dev.kept(label, name, was, now, [name])
            return now

        raw = dev.snapshot()
        now = call('begin', lib.gccnmf_klnmf_shared_begin(W, ws, F, N, K, B, _stream()), raw)
        P.check_begin(rep, dev.logical(raw), dev.logical(now))
        assert (now['hscale'] == 1).all() and not _bits(now['R0']).any(), '%s: begin: hscale is not 1 on all Kp entries or R is not zero' % label
        if sh.single:
            assert not any(_bits(now[n + '0']).any() for n in ('Wt', 'Ht', 'Rt')), '%s: begin left Wt, Ht or Rt non-zero' % label
        if poke:
            sh.view(dev.t['ws0'], 'hscale')[:K] = torch.from_numpy(np.array(dev.s0)).cuda()
            now = dev.snapshot()
        for it in range(iterations):
            raw, now = now, call('step A', lib.gccnmf_klnmf_shared_step_a(V, W, H, ws, partial, F, N, K, B, ALPHA, EPS, _stream()), now)
            P.check_step_a(rep, dev.logical(raw), dev.logical(now))
            dev.direct_copies(rep, 'step A', raw, now)
            seen.append(now)
            raw, now = now, call('step B', lib.gccnmf_klnmf_shared_step_b(W, ws, partial, F, N, K, B, _stream()), now)
            P.check_step_b(rep, dev.logical(raw), dev.logical(now))
        raw, now = now, call('finish', lib.gccnmf_klnmf_shared_finish(H, ws, F, N, K, B, _stream()), now)
        P.check_finish(rep, dev.logical(raw), dev.logical(now))
        assert (now['hscale'] == 1).all(), '%s: finish: hscale is not 1 on all Kp entries' % label
        rep.summary(dev.form())
    return seen, now


@pytest.mark.parametrize('case', P.FOUR_CALL_CASES, ids=[c.id for c in P.FOUR_CALL_CASES])
def test_four_calls(case):
    _four_calls(case)


# ---- (b) the one-call run through its all-reduce hook --------------------------------------------------------------------------------------------------
def _run(case, iterations=2, write=None):
    """gccnmf_klnmf_shared_run with a recording hook -> (dev, the state before, the states at each hook's entry, the state after).
    write: per hook, the partial the hook leaves in place of the one it found (the other ranks' contribution of a rank without columns)."""
    with _tuning(case.keys) as lib:
        dev = Device(lib, case, four=False)
        before, records, errors = dev.snapshot(), [], []

        def hook(ctx, buf, count, stream):
            try:
                records.append(dict(dev.snapshot(), _args=(buf, count, stream)))
                if write is not None:
                    dev.t['partial'].copy_(torch.from_numpy(write[len(records) - 1]))
                    torch.cuda.synchronize()
                return 0
            except BaseException as e:                              # noqa: an exception must not cross the C frames
                errors.append(e)
                return 1

        arr = (_hip().SharedShard * max(len(dev.shards), 1))()
        for i, (d, sh) in enumerate(zip(arr, dev.shards)):
            d.V, d.H, d.workspace, d.N, d.batch, d.ld = dev.ptr('V', i), dev.ptr('H', i), dev.ptr('ws%d' % i), sh.N, sh.batch, sh.ld
        fn = _hip().ALLREDUCE_FN(hook)
        rc = lib.gccnmf_klnmf_shared_run(arr, len(dev.shards), dev.ptr('W'), dev.ptr('partial'), dev.ptr('vec'), case.F, case.K, iterations,
                                         ALPHA, EPS, fn, None, _stream())
        if errors:
            raise errors[0]
        assert rc == 0, '%s: gccnmf_klnmf_shared_run returned %d' % (case, rc)
        after = dev.snapshot()
    assert len(records) == iterations, '%s: the hook was called %d times in %d iterations' % (case, len(records), iterations)
    for r in records:
        buf, count, stream = r.pop('_args')
        assert buf == dev.ptr('partial') and count == P.partial_floats(case.F, case.K) and (stream or 0) == _stream()
    return dev, before, records, after


def _check_run(dev, before, records, after):
    """two iterations, every call on exact inputs (module docstring, (b))"""
    case, L = dev.case, dev.logical
    label, F = str(case), case.F
    rep = P.Report(label)
    h1, h2 = records
    s0, s1, s2, s3 = L(before), L(h1), L(h2), L(after)
    dev.kept(label, 'begin + step A', before, h1, ['begin', 'step A'])
    P.check_begin(rep, s0, s1, R=False)
    assert (h1['hscale'] == 1).all(), '%s: begin: hscale is not 1 on all Kp entries' % label
    P.check_step_a(rep, dict(s1, shards=s0['shards']), s1, 'step A (1)')
    dev.direct_copies(rep, 'step A (1)', dict(h1, **{n: before[n] for n in dev.inputs}), h1)
    dev.kept(label, 'step B + step A', h1, h2, ['step B', 'step A'])
    P.check_step_b(rep, s1, s2, 'step B (1)')
    P.check_step_a(rep, dict(s2, shards=s1['shards']), s2, 'step A (2)')
    dev.direct_copies(rep, 'step A (2)', dict(h2, **{n: h1[n] for n in dev.inputs}), h2)
    dev.kept(label, 'step B + finish', h2, after, ['step B', 'finish'])
    Wr, sr, cr = S.stage5(s2['W'], s2['num'], s2['den'])
    rep.within('step B (2) W', [s3['W']], [Wr], S.bar_W(F))
    rep.within('step B (2) colsumW', [s3['colsumW']], [cr], S.bar_colsumW(F))
    files = lambda st: sum((sh['H'] for sh in st['shards']), [])
    P.lazy_scale_of(rep, 'step B (2) hscale, through finish H = H * hscale', files(s2), files(s3), sr, S.bar_s(F))
    assert (after['hscale'] == 1).all(), '%s: finish: hscale is not 1 on all Kp entries' % label
    rep.summary(dev.form())
    return rep


@pytest.mark.parametrize('case', P.RUN_CASES, ids=[c.id for c in P.RUN_CASES])
def test_run_through_the_hook(case):
    """column blocks of one matrix plus the ragged remainder (defaults and the throughput tile, LDS-DMA and register-staged): the generic
    padding and ownership checks are, there, `the columns >= 229 of H stay exactly zero` and `V is untouched`; one column block with
    ld == Np: the direct kernels inside the run; two plain shards of different widths: shard-order accumulation; 2 and 3 side-stream file
    groups (and one, by key 8): every file is checked, so a group that ran on the wrong base pointer cannot pass."""
    dev, before, records, after = _run(case)
    _check_run(dev, before, records, after)
    if case.ld == 256:
        assert not _bits(after['H'][:, 229:]).any() and not _bits(records[1]['H'][:, 229:]).any()


def test_run_of_a_rank_without_columns():
    """nshards == 0: at each hook's entry partial is exactly +0 in all its words; the hook then leaves there what the other ranks would --
    the partials recorded from the column-block case -- and W, colsumW, hscale follow stage 5 of exactly that."""
    _, _, donors, _ = _run(P.RUN_CASES[0])
    write = [r['partial'].copy() for r in donors]
    dev, before, (h1, h2), after = _run(P.NO_COLUMNS, write=write)
    label, F, L = str(P.NO_COLUMNS), P.NO_COLUMNS.F, dev.logical
    rep = P.Report(label)
    for i, h in enumerate((h1, h2)):
        assert h['partial'].size == P.partial_floats(F, P.NO_COLUMNS.K) and not _bits(h['partial']).any(), '%s: hook %d: partial is not all +0' % (label, i + 1)
    dev.kept(label, 'begin', before, h1, ['begin', 'step A'])
    P.check_begin(rep, L(before), L(h1))
    given = lambda raw, p: L(dict(raw, partial=p))
    dev.kept(label, 'step B', h1, h2, ['step B', 'step A'])
    P.check_step_b(rep, given(h1, write[0]), L(h2), 'step B (1)')
    dev.kept(label, 'step B + finish', dict(h2, partial=write[1]), after, ['step B', 'finish'])
    Wr, _, cr = S.stage5(*[given(h2, write[1])[n] for n in ('W', 'num', 'den')])
    rep.within('step B (2) W', [L(after)['W']], [Wr], S.bar_W(F))
    rep.within('step B (2) colsumW', [L(after)['colsumW']], [cr], S.bar_colsumW(F))
    assert (after['hscale'] == 1).all()
    rep.summary(dev.form())


def test_run_of_zero_iterations():
    """the hook is never called; W and H are bit for bit unchanged, colsumW = stage0(W), hscale == 1 (and R is zero: begin ran)"""
    case = P.RUN_CASES[4]
    assert case.name == 'two plain shards'
    dev, before, records, after = _run(case, iterations=0)
    assert records == []
    dev.kept(str(case), 'begin + finish', before, after, ['begin'])             # (finish's H *= 1 must change nothing: H is not owned here)
    rep = P.Report(str(case))
    P.check_begin(rep, dev.logical(before), dev.logical(after))
    assert (after['hscale'] == 1).all() and not any(_bits(after['R%d' % i]).any() for i in range(len(dev.shards)))


def test_hook_states_are_the_four_calls_bit_for_bit():
    """(513, 96, 65) x 3, plain layout: what the hook sees in the run is what the four calls leave (no poke), every buffer, every word"""
    case = P.CROSS_CHECK
    steps, final = _four_calls(case, poke=False, iterations=2)
    dev, _, records, after = _run(case)
    for i, (four, run) in enumerate(zip(steps + [final], records + [after])):
        for name in run:
            same = _bits(run[name]) == _bits(four[name])
            assert same.all(), '%s: %s at %s differs between the run and the four calls: %d words' % (
                case, name, 'hook %d' % (i + 1) if i < 2 else 'the end', int((~same).sum()))
