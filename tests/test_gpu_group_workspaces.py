"""-m gpu: KL-NMF on workspaces carved back to back out of ONE allocation -- what the engine's file groups get (group i works in
ws_nmf[i * size:]) -- at the shapes where the second carve used to start 8 bytes past a 16-byte boundary: an odd number of files per
group and an even number of 64-column tiles (the counter block at the workspace's end was batch * (2 * ceil(N / 64) + 2) + 32 words).
The size is now a multiple of 64 floats and the entry points reject a workspace that is not 16-byte aligned (tests/test_host.py); here
the second group's workspace is used for real, in every launch form gccnmf_klnmf has, and must give bit for bit what the first gives,
within the oracle's bar, without touching a word outside its own carve.

Bars: W, H against the float64 oracle as test_gpu_kernels.test_klnmf_vs_oracle (relative Frobenius error < 1e-4); the divergence as
test_gpu_kl_divergence.test_value_against_float64 (kl_divergence_restatement.value_bar)."""
import ctypes

import numpy as np
import pytest

import kl_divergence_restatement as R
from oracle import gccnmf_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
GUARD = 64                      # floats behind the second carve
PATTERN = 0x7fc0dead            # a NaN's bits: whoever reads a word outside its carve cannot stay finite, whoever writes one is seen


@pytest.fixture(scope='module')
def lib():
    from gcc_nmf_amd import _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300)


def tiles(N):
    return -(-N // 64)


def misaligned_before(per, N):
    """The carve this shape used to get: the old counter block made the workspace size = 2 (mod 4) floats."""
    return per % 2 == 1 and tiles(N) % 2 == 0 and (per * (2 * tiles(N) + 2) + 32) % 4 == 2


def two_carves(ws_per):
    """One allocation of two group workspaces and a guard, every word the pattern; (ws, int32 view)."""
    ws = torch.full((2 * ws_per + GUARD,), PATTERN, dtype=torch.int32, device='cuda')
    return ws.view(torch.float32), ws


def outside_untouched(bits, ws_per, carve):
    """Every word of the allocation outside carve `carve` still holds the pattern."""
    lo, hi = carve * ws_per, (carve + 1) * ws_per
    return bool((bits[:lo] == PATTERN).all()) and bool((bits[hi:] == PATTERN).all())


def chain_status(lib, ws, F, N, K, per):
    st = ctypes.c_int(-1)
    assert lib.gccnmf_klnmf_chain_status(ws.data_ptr(), F, N, K, per, ctypes.byref(st)) == 0
    return st.value


class tuning(object):
    """gccnmf_set_tuning(key, value) for the block, the library's defaults afterwards."""
    DEFAULTS = {2: 0, 16: 1, 17: 1}

    def __init__(self, lib, keys):
        self.lib, self.keys = lib, keys

    def __enter__(self):
        for k, v in self.keys.items():
            assert self.lib.gccnmf_set_tuning(k, v) == 0

    def __exit__(self, *exc):
        for k in self.keys:
            self.lib.gccnmf_set_tuning(k, self.DEFAULTS[k])


# name -> (F, N, K, files per group, iterations, tuning keys, plan bits 0-3 the form must show)
#   tuning key 2 = 1: the 512 x 64 throughput (LDS-DMA) tile at any launch size; keys 16 / 17 = 2: the fused short-dictionary launches
#   whenever the shape allows (by rule they want whole rounds of workgroups)
FORMS = {
    'one file alone': (513, 244, 128, 1, 5, {}, 1),
    'direct K=128': (513, 244, 128, 3, 5, {}, 1),
    'direct K=300': (513, 244, 300, 3, 5, {}, 1),
    'fused short dictionary': (513, 244, 128, 9, 5, {16: 2, 17: 2}, 6),
    'throughput tile by rule, 9 files K=256': (513, 1908, 256, 9, 4, {}, 0),
    'throughput tile by rule, 17 files K=1024': (513, 1012, 1024, 17, 3, {}, 0),
    'throughput tile forced, 9 files K=256': (513, 244, 256, 9, 4, {2: 1}, 0),
    'throughput tile forced, 17 files K=1024': (513, 244, 1024, 17, 3, {2: 1}, 0),
    'small-batch tile, 9 files K=256': (513, 244, 256, 9, 4, {}, 0),
    'off-path geometry': (200, 330, 100, 5, 5, {}, 0),
}


@pytest.mark.parametrize('form', sorted(FORMS))
def test_klnmf_on_the_second_carve_is_bitwise_the_first_and_within_the_oracle_bar(lib, form):
    """gccnmf_klnmf for `per` files on ws[0:] and on ws[ws_per:] of one allocation, same V, W0, H0: W and H bit for bit equal, the first and
    the last file within 1e-4 of the float64 oracle, no word outside the carve in use written, the status words clean.  Every shape has
    `per` odd and ceil(N / 64) even (the 8-byte carve of the old size formula), and gccnmf_klnmf_plan shows the form the case is named for:
    the direct latency kernels (one file: its workspace also holds the reserved block of a single file; three files), the fused short-dictionary launches
    (forced: keys 16 / 17), four launches with R materialised on the throughput tile, the small-batch tile, and a geometry without the
    bin-tail (F = 200).
    The throughput (LDS-DMA) tile by rule: at N = 244 neither 9 files at K = 256 nor 17 at K = 1024 reach it -- K1 and K3 take it from
    files * ceil(N / 64) >= 256 tall tiles on (nmf.hip: small_batch_tile) and have 36 and 68 -- so N is raised to the next values with an
    even tile count that do: N = 1908 (30 tiles, 270) for 9 files, N = 1012 (16 tiles, 272) for 17; N = 244 runs with the tile forced
    (tuning key 2 = 1), and once by rule on the small-batch tile, which is what the engine's groups of 9 run."""
    from gcc_nmf_amd.engine import Geometry, padded, klnmf_initial_factors
    F, N, K, per, iters, keys, want_plan = FORMS[form]
    assert misaligned_before(per, N)
    with tuning(lib, keys):
        plan = lib.gccnmf_klnmf_plan(F, N, K, per, 0)
        assert plan == want_plan, (form, plan)
        if 'by rule' in form:
            assert per * tiles(N) >= 256 and per * tiles(244) < 256
        ws_per = lib.gccnmf_klnmf_workspace_floats(F, N, K, per)
        assert ws_per > 0 and ws_per % 4 == 0
        g = Geometry(F, N // 2, K)
        assert g.Np == tiles(N) * 64
        rng = np.random.RandomState(F + N + K + per)
        V = (np.abs(rng.standard_normal((per, F, N))) + 0.01).astype(np.float32)
        W0, H0 = klnmf_initial_factors(F, N, K)
        dV = padded(V, (per, g.Fp, g.Np), 'cuda')
        ws, bits = two_carves(ws_per)
        res = []
        for carve in (0, 1, 0):
            mine = ws[carve * ws_per:]
            assert mine.data_ptr() % 16 == 0
            bits.fill_(PATTERN)
            mine[:ws_per].zero_()
            dW = padded(np.repeat(W0[None], per, 0), (per, g.Fp, g.Kp), 'cuda')
            dH = padded(np.repeat(H0[None], per, 0), (per, g.Kp, g.Np), 'cuda')
            assert lib.gccnmf_klnmf(dV.data_ptr(), dW.data_ptr(), dH.data_ptr(), mine.data_ptr(), F, N, K, per, iters, 0.0, 1e-16, 0, stream()) == 0
            torch.cuda.synchronize()
            assert outside_untouched(bits, ws_per, carve), (form, carve)
            assert chain_status(lib, mine, F, N, K, per) == 0
            res.append((dW, dH))
    for W, H in res[1:]:
        assert torch.equal(W, res[0][0]) and torch.equal(H, res[0][1]), form
    W, H = res[1][0].cpu().numpy(), res[1][1].cpu().numpy()
    assert np.isfinite(W).all() and np.isfinite(H).all()
    assert not W[:, F:].any() and not W[:, :, K:].any() and not H[:, K:].any() and not H[:, :, N:].any()         # the padding stays zero
    for b in sorted({0, per - 1}):
        Wr, Hr = O.performKLNMF(V[b], K, iters, 0)
        print('%s, file %d: rel W %.3g, rel H %.3g (bar 1e-4)' % (form, b, rel(W[b, :F, :K], Wr), rel(H[b, :K, :N], Hr)))
        assert rel(W[b, :F, :K], Wr) < 1e-4 and rel(H[b, :K, :N], Hr) < 1e-4, (form, b, rel(W[b, :F, :K], Wr), rel(H[b, :K, :N], Hr))


@pytest.mark.parametrize('F,N,K,per', [(130, 200, 160, 3), (513, 244, 128, 3)])
def test_divergence_on_the_second_carve(lib, F, N, K, per):
    """Stage 7 (float64 tile partials and results inside the workspace) in the second group's workspace: against the float64 divergence
    of the same factors at value_bar, bit for bit the first carve's, nothing outside the carve written."""
    assert misaligned_before(per, N)
    Fp, Kp, Np = -(-F // 16) * 16, -(-K // 64) * 64, -(-N // 64) * 64
    rng = np.random.RandomState(F * 7 + N * 3 + K)
    V = np.stack([R.low_rank_plus_noise(F, N, 5, 0.3, F + N + 17 * b) for b in range(per)])
    W = (rng.rand(per, F, K) + 0.01).astype(np.float32)
    H = (rng.rand(per, K, N) + 0.01).astype(np.float32)
    from gcc_nmf_amd.engine import padded
    dV, dW, dH = padded(V, (per, Fp, Np), 'cuda'), padded(W, (per, Fp, Kp), 'cuda'), padded(H, (per, Kp, Np), 'cuda')
    ws_per = lib.gccnmf_klnmf_workspace_floats(F, N, K, per)
    ws, bits = two_carves(ws_per)
    out = []
    for carve in (0, 1):
        mine = ws[carve * ws_per:]
        bits.fill_(PATTERN)
        assert lib.gccnmf_klnmf_stage(dV.data_ptr(), dW.data_ptr(), dH.data_ptr(), mine.data_ptr(), F, N, K, per, 0.0, 1e-16, 0, 7, stream()) == 0
        torch.cuda.synchronize()
        assert outside_untouched(bits, ws_per, carve)
        at = per * Fp * Np
        out.append(mine[at:at + 2 * per].view(torch.float64).cpu().numpy().copy())
    assert out[0].tobytes() == out[1].tobytes()
    for b in range(per):
        want, bar = R.kl_divergence(V[b], W[b], H[b]), R.value_bar(V[b], W[b], H[b])
        print('stage 7 (%d, %d, %d) second carve, file %d: D = %.17g, reference %.17g, |error| = %.3g of the bar' % (F, N, K, b, out[1][b], want, abs(out[1][b] - want) / bar))
        assert np.isfinite(out[1][b]) and abs(out[1][b] - want) <= bar


def test_divergence_of_bins_far_below_the_model(lib):
    """0 < V < R * 2^-24: V - R rounds to -R, and the term's general form (1 + x) log1p(x) - x at x = -1 is 0 * -inf.  The out-of-band bins
    of a quiet mixture under the random initial factors are such elements (the engine's divergence at iteration 0 was NaN for them).  Against
    the float64 divergence at value_bar, with elements at 1e-9, 1e-30 and (subnormal) 1e-42 of a model of order 10."""
    from gcc_nmf_amd.engine import padded
    F, N, K = 70, 150, 24
    Fp, Kp, Np = -(-F // 16) * 16, -(-K // 64) * 64, -(-N // 64) * 64
    rng = np.random.RandomState(5)
    V = R.low_rank_plus_noise(F, N, 5, 0.3, 3)[None].copy()
    V[0, 40:, :] = 1e-9
    V[0, :10, 100:] = 1e-30
    V[0, 10:20, 100:] = 1e-42
    assert (V[0, 10:20, 100:] > 0).all()
    W = (rng.rand(1, F, K) + 0.5).astype(np.float32)
    H = (rng.rand(1, K, N) + 0.5).astype(np.float32)
    dV, dW, dH = padded(V, (1, Fp, Np), 'cuda'), padded(W, (1, Fp, Kp), 'cuda'), padded(H, (1, Kp, Np), 'cuda')
    ws = torch.zeros(lib.gccnmf_klnmf_workspace_floats(F, N, K, 1), dtype=torch.float32, device='cuda')
    assert lib.gccnmf_klnmf_stage(dV.data_ptr(), dW.data_ptr(), dH.data_ptr(), ws.data_ptr(), F, N, K, 1, 0.0, 1e-16, 0, 7, stream()) == 0
    torch.cuda.synchronize()
    D = float(ws[Fp * Np:Fp * Np + 2].view(torch.float64).cpu().numpy()[0])
    want, bar = R.kl_divergence(V[0], W[0], H[0]), R.value_bar(V[0], W[0], H[0])
    print('stage 7, bins far below the model: D = %.17g, reference %.17g, |error| = %.3g of the bar' % (D, want, abs(D - want) / bar))
    assert np.isfinite(D) and abs(D - want) <= bar


def test_ragged_call_on_the_second_carve_is_bitwise_the_equal_length_batches(lib):
    """gccnmf_klnmf_ragged, 11 files of two lengths (5 x 244 and 6 x 120 columns; ceil(244 / 64) = 4), in the second of two ragged
    workspaces: its list tables sit behind the counters at the workspace's end.  Every file bit for bit what gccnmf_klnmf gives a batch of
    the files of its length (all on the throughput tile, tuning key 2 = 1: the only tile the ragged launch has), and what the first carve gives."""
    from gcc_nmf_amd.engine import Geometry, padded, klnmf_initial_factors
    F, K, Nmax, iters = 513, 256, 244, 4
    lengths = [244, 120] * 5 + [120]
    batch = len(lengths)
    assert misaligned_before(batch, Nmax)
    g = Geometry(F, Nmax // 2, K)
    rng = np.random.RandomState(11)
    V = [(np.abs(rng.standard_normal((F, n))) + 0.01).astype(np.float32) for n in lengths]
    start = dict((n, klnmf_initial_factors(F, n, K)) for n in set(lengths))

    def blocks(files, Np, what):
        t = torch.zeros((len(files), g.Fp if what != 'H' else g.Kp, Np if what != 'W' else g.Kp), dtype=torch.float32, device='cuda')
        for k, f in enumerate(files):
            a = V[f] if what == 'V' else start[lengths[f]][0 if what == 'W' else 1]
            t[k, :a.shape[0], :a.shape[1]] = torch.from_numpy(a).cuda()
        return t
    everyone = list(range(batch))
    with tuning(lib, {2: 1}):
        n_ws = lib.gccnmf_klnmf_ragged_workspace_floats(F, Nmax, K, batch)
        assert n_ws > 0 and n_ws % 4 == 0
        ws, bits = two_carves(n_ws)
        host_n = (ctypes.c_int * batch)(*lengths)
        res = []
        for carve in (0, 1):
            mine = ws[carve * n_ws:]
            bits.fill_(PATTERN)
            mine[:n_ws].zero_()
            dV, dW, dH = blocks(everyone, g.Np, 'V'), blocks(everyone, g.Np, 'W'), blocks(everyone, g.Np, 'H')
            assert lib.gccnmf_klnmf_ragged(dV.data_ptr(), dW.data_ptr(), dH.data_ptr(), mine.data_ptr(), F, host_n, Nmax, K, batch, iters, 0.0,
                                           1e-16, 0, stream()) == 0
            torch.cuda.synchronize()
            assert outside_untouched(bits, n_ws, carve)
            assert chain_status(lib, mine, F, Nmax, K, batch) == 0
            res.append((dW, dH))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        W, H = res[1]
        assert torch.isfinite(W).all() and torch.isfinite(H).all()
        for n in sorted(set(lengths)):
            files = [f for f in everyone if lengths[f] == n]
            Np = tiles(n) * 64
            dV, dW, dH = blocks(files, Np, 'V'), blocks(files, Np, 'W'), blocks(files, Np, 'H')
            plain = torch.zeros(lib.gccnmf_klnmf_workspace_floats(F, n, K, len(files)), dtype=torch.float32, device='cuda')
            assert lib.gccnmf_klnmf(dV.data_ptr(), dW.data_ptr(), dH.data_ptr(), plain.data_ptr(), F, n, K, len(files), iters, 0.0, 1e-16, 0, stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(W[files], dW), n
            assert torch.equal(H[files][:, :, :Np], dH) and not H[files][:, :, n:].any(), n
    Wr, Hr = O.performKLNMF(V[1], K, iters, 0)
    assert rel(W[1, :F, :K].cpu().numpy(), Wr) < 1e-4 and rel(H[1, :K, :120].cpu().numpy(), Hr) < 1e-4


def engine(**kw):
    from gcc_nmf_amd.engine import GCCNMFEngine
    return GCCNMFEngine(32000, **kw)                 # T = 122 frames, N = 244 columns: 4 column tiles


@pytest.mark.parametrize('batch,K,iters', [(6, 128, 6), (18, 128, 6), (18, 256, 5), (34, 1024, 3)])
def test_engine_with_an_odd_number_of_files_per_group(lib, batch, K, iters):
    """GCCNMFEngine(nmf_groups=2) with 3, 9 and 17 files per group: the second group's workspace is the carve that used to be misaligned.
    separate(), W and H bit for bit those of one group -- the launch forms that follow the launch size are chosen for the files of both
    groups together (GCCNMF_FLAG_GROUPS), whatever the split -- a second separate() reproduces them, the chain status is clean."""
    from gcc_nmf_amd.synthetic import synthetic_batch
    xs = synthetic_batch(300, batch, numSamples=32000)
    kw = dict(dictionarySize=K, numIterations=iters, batch=batch)
    e1 = engine(nmf_groups=1, **kw)
    assert e1.g.T == 122 and e1.g.N == 244 and misaligned_before(batch // 2, e1.g.N)
    y1 = e1.separate(xs)
    assert e1.chain_failed() == 0
    e2 = engine(nmf_groups=2, **kw)
    assert e2.nmf_groups == 2 and (e2.ws_nmf.numel() // 2) % 4 == 0 and e2.ws_nmf[e2.ws_nmf.numel() // 2:].data_ptr() % 16 == 0
    y2 = e2.separate(xs)
    assert e2.chain_failed() == 0
    assert torch.isfinite(e2.W).all() and torch.isfinite(e2.H).all() and np.isfinite(y2).all() and np.abs(y2).max() > 0
    assert torch.equal(e2.W, e1.W) and torch.equal(e2.H, e1.H)
    assert np.array_equal(y2, y1)
    assert np.array_equal(e2.separate(xs), y1) and torch.equal(e2.W, e1.W) and torch.equal(e2.H, e1.H)
    assert e2.chain_failed() == 0


def test_engine_divergences_in_the_second_group_workspace(lib):
    """tolerance=: the per-file divergences (stage 7 on each group's own carve) and the iteration counts of two groups of 9 files equal
    those of one group of 18, and the final divergence is the float64 one of the factors within value_bar."""
    from gcc_nmf_amd.synthetic import synthetic_batch
    batch = 18
    xs = synthetic_batch(300, batch, numSamples=32000)
    kw = dict(dictionarySize=128, numIterations=12, batch=batch, tolerance=0.02, checkEvery=2)
    e1, e2 = engine(nmf_groups=1, **kw), engine(nmf_groups=2, **kw)
    assert e2.nmf_groups == 2 and misaligned_before(batch // 2, e2.g.N)
    y1, y2 = e1.separate(xs), e2.separate(xs)
    assert e1.chain_failed() == 0 and e2.chain_failed() == 0
    assert np.array_equal(e2.get_iterations(), e1.get_iterations())
    t1, t2 = e1.get_divergence_trace(), e2.get_divergence_trace()
    assert t2.shape == t1.shape and t2.shape[1] == batch and np.isfinite(t2).all() and (t2 > 0).all()
    assert t2.tobytes() == t1.tobytes()
    assert e2.get_divergence().tobytes() == e1.get_divergence().tobytes()
    assert torch.equal(e2.W, e1.W) and torch.equal(e2.H, e1.H) and np.array_equal(y2, y1)
    g = e2.g
    V, (W, H), D = e2.V.cpu().numpy(), e2.get_WH(), e2.get_divergence()
    for b in (0, 9, 17):                                       # the first group's first file, the second group's first and last
        Vb = V[b, :g.F, :g.N]
        want, bar = R.kl_divergence(Vb, W[b], H[b]), R.value_bar(Vb, W[b], H[b])
        print('engine, file %d: D = %.17g, reference %.17g, |error| = %.3g of the bar' % (b, D[b], want, abs(D[b] - want) / bar))
        assert abs(D[b] - want) <= bar
