"""The KL-divergence stage (gccnmf_klnmf_stage, stage 7: csrc/divergence.hip) through the C ABI, and the convergence-stopped KL-NMF built
on it (getKLDivergence, performKLNMFUntilConverged, GCCNMFEngine(tolerance=...), inferKLNMFCoefficients(tolerance=...)).

References: tests/kl_divergence_restatement.py (float64 divergence of the same float32 factors; the oracle's float32 loop with the
stopping rule).  The value bar is (8 + K) * 2^-24 * sum(V + R) absolute (restatement.value_bar states why).

Every value test prints |D - reference| and its share of the bar before it asserts; DESIGN section 2a is where the figures are recorded."""
import functools

import numpy as np
import pytest
import torch

import kl_divergence_restatement as R

pytestmark = pytest.mark.gpu

FIXED_W = 1 << 16
SHAPES = [(70, 150, 24), (130, 200, 160), (33, 64, 8)]
BIG = (513, 128, 128)                    # full 128-row MFMA tiles + a one-row tile (F = 4 * 128 + 1), the short-dictionary path of the iteration


def _lib():
    from gcc_nmf_amd import _hip
    return _hip.lib()


def _geom(F, N, K):
    return -(-F // 16) * 16, -(-K // 64) * 64, -(-N // 64) * 64


@functools.lru_cache(maxsize=None)
def _factors(F, N, K, files):
    """`files` independent problems: low-rank-plus-noise V with isolated zeros, positive W and H (read-only arrays, shared by the tests)."""
    rng = np.random.RandomState(F * 7 + N * 3 + K)
    V = np.stack([R.low_rank_plus_noise(F, N, 5, 0.3, F + N + 17 * b) for b in range(files)])
    W = (rng.rand(files, F, K) + 0.01).astype(np.float32)
    H = (rng.rand(files, K, N) + 0.01).astype(np.float32)
    for a in (V, W, H):
        a.flags.writeable = False
    return V, W, H


@functools.lru_cache(maxsize=None)
def _reference(F, N, K, files):
    V, W, H = _factors(F, N, K, files)
    return [(R.kl_divergence(V[b], W[b], H[b]), R.value_bar(V[b], W[b], H[b])) for b in range(files)]


def _pad(a, shape, fill):
    t = torch.full(shape, fill, dtype=torch.float32, device='cuda')
    t[tuple(slice(0, n) for n in a.shape)] = torch.from_numpy(np.array(a)).cuda()
    return t


def _stage7(V, W, H, pad=0.0, fixed=False, check_untouched=True):
    """V (B, F, N), W (B, F, K) -- or (F, K) with fixed --, H (B, K, N) -> (B,) float64 through the C ABI; `pad` fills the padding."""
    lib = _lib()
    B, F, N = V.shape
    K = H.shape[1]
    Fp, Kp, Np = _geom(F, N, K)
    Vd, Hd = _pad(V, (B, Fp, Np), pad), _pad(H, (B, Kp, Np), pad)
    Wd = _pad(W, (Fp, Kp) if fixed else (B, Fp, Kp), pad)
    n_ws = lib.gccnmf_klnmf_workspace_floats(F, N, K, B)
    ws = torch.from_numpy(np.random.RandomState(1).randint(1, 1 << 30, n_ws).astype(np.int32)).cuda().view(torch.float32)     # arbitrary bits
    before = [t.clone() for t in (Vd, Wd, Hd, ws)]
    rc = lib.gccnmf_klnmf_stage(Vd.data_ptr(), Wd.data_ptr(), Hd.data_ptr(), ws.data_ptr(), F, N, K, B, 0.0, 1e-16, FIXED_W if fixed else 0, 7,
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    at = B * Fp * Np
    assert (ws.data_ptr() + 4 * at) % 16 == 0
    D = ws[at:at + 2 * B].view(torch.float64).cpu().numpy().copy()
    if check_untouched:
        for name, t, b in zip('VWH', (Vd, Wd, Hd), before):
            assert torch.equal(t.view(torch.int32), b.view(torch.int32)), '%s changed' % name
        # the workspace: only the head of each file's R block (tile partials) and the result area may change -- the chain counters and
        # the status words at its end in particular stay as they were
        tiles = -(-F // 128) * -(-N // 64)
        changed = (ws.view(torch.int32) != before[3].view(torch.int32)).nonzero().flatten().cpu().numpy()
        allowed = np.zeros(n_ws, bool)
        for b in range(B):
            allowed[b * Fp * Np:b * Fp * Np + 2 * tiles] = True
        allowed[at:at + 2 * B] = True
        assert allowed[changed].all(), 'stage 7 wrote outside its two areas: %s' % changed[~allowed[changed]][:8]
        assert 2 * tiles <= Fp * Np and at + 2 * B <= n_ws - 32
        assert torch.equal(ws[-32:].view(torch.int32), before[3][-32:].view(torch.int32))
    return D


CASES = [(F, N, K, B) for F, N, K in SHAPES for B in (1, 3)] + [BIG + (2,)]


@pytest.mark.parametrize('F,N,K,B', CASES)
def test_value_against_float64(F, N, K, B):
    V, W, H = _factors(F, N, K, 3)
    D = _stage7(V[:B], W[:B], H[:B])
    for b in range(B):
        want, bar = _reference(F, N, K, 3)[b]
        print('stage 7 (%d, %d, %d) batch %d file %d: D = %.17g, reference %.17g, |error| = %.3g = %.3g of the bar %.3g'
              % (F, N, K, B, b, D[b], want, abs(D[b] - want), abs(D[b] - want) / bar, bar))
        assert np.isfinite(D[b]) and abs(D[b] - want) <= bar


@pytest.mark.parametrize('F,N,K', SHAPES + [BIG])
def test_bits_alone_in_any_batch_run_to_run_and_garbage_in_the_padding(F, N, K):
    V, W, H = _factors(F, N, K, 3)
    alone = _stage7(V[:1], W[:1], H[:1])[0]
    for order in ([0, 1, 2], [1, 0, 2], [1, 2, 0]):
        D = _stage7(V[order], W[order], H[order], check_untouched=False)
        assert D[order.index(0)].tobytes() == alone.tobytes(), (order, D, alone)
    again = _stage7(V[[1, 2, 0]], W[[1, 2, 0]], H[[1, 2, 0]], check_untouched=False)
    assert again.tobytes() == D.tobytes()
    # NaN in every padding row and column of V, W and H (stage 7 runs alone on these buffers: no other stage has to cope with them)
    nan = _stage7(V[[1, 2, 0]], W[[1, 2, 0]], H[[1, 2, 0]], pad=float('nan'))
    assert nan.tobytes() == D.tobytes()


def test_shared_dictionary_form_and_python_layer():
    import gcc_nmf_amd.gccNMFFunctions as G
    F, N, K = SHAPES[0]
    V, W, H = _factors(F, N, K, 3)
    own = _stage7(V, np.broadcast_to(W[1], W.shape).copy(), H)
    shared = _stage7(V, W[1], H, fixed=True, pad=float('nan'))
    assert shared.tobytes() == own.tobytes()
    d = G.getKLDivergence(V[0], W[0], H[0])
    assert isinstance(d, np.float64) and d.tobytes() == _stage7(V[:1], W[:1], H[:1])[0].tobytes()
    lib, P = _lib(), 4096
    assert lib.gccnmf_klnmf_stage(P, P, P, P, F, N, K, 1, 0.0, 0.0, 0, 8, None) == 1            # an unknown stage: what it returned before
    assert lib.gccnmf_klnmf_stage(P, P, P, P, F, N, K, 1, 0.0, 0.0, FIXED_W | 1, 7, None) == 1
    assert lib.gccnmf_klnmf_stage(P, P, P, P + 4, F, N, K, 1, 0.0, 0.0, 0, 7, None) == 1         # a workspace that is not 8-byte aligned


def test_resident_divergence_uses_the_device_dictionary():
    import gcc_nmf_amd.gccNMFFunctions as G
    F, N, K = SHAPES[2]
    V = _factors(F, N, K, 3)[0][0]
    try:
        G.set_resident(True)
        W, H = G.performKLNMF(V, K, 4, 0)
        d = G.getKLDivergence(V, W, H)
    finally:
        G.set_resident(False)
    assert d.tobytes() == G.getKLDivergence(V, np.array(W), np.array(H)).tobytes()
    assert abs(d - R.kl_divergence(V, W, H)) <= R.value_bar(V, W, H)


def test_descent():
    """alpha = 0: D never rises from check to check by more than the evaluation bar, and falls as far as the oracle's does."""
    import gcc_nmf_amd.gccNMFFunctions as G
    F, N, K = SHAPES[0]
    V = _factors(F, N, K, 3)[0][0]
    ref = R.klnmf_until_converged(V, K, 30, 0, 1e-9, 5)
    assert ref['iterations'] == 30
    W, H, info = G.performKLNMFUntilConverged(V, K, 30, 0, tolerance=1e-9, checkEvery=5)
    assert info['iterations'] == 30 and [it for it, _ in info['divergences']] == [0, 5, 10, 15, 20, 25, 30]
    D = [d for _, d in info['divergences']]
    print('descent:', D, 'oracle:', [d for _, d in ref['divergences']])
    for (a, b), bar in zip(zip(D, D[1:]), ref['bars'][1:]):
        assert b <= a + bar
    # the factors are within 1e-4 * max of the oracle's, which moves D by well under a percent
    assert D[-1] / D[0] <= ref['divergences'][-1][1] / ref['divergences'][0][1] * 1.01
    assert D[-1] == G.getKLDivergence(V, W, H) and abs(D[-1] - R.kl_divergence(V, W, H)) <= R.value_bar(V, W, H)


# (F, N, K) -> tolerance, checkEvery, maxIterations: the restatement stops strictly before maxIterations with its criterion a factor
# 1.5 clear of the tolerance at the stopping check and at the one before (asserted below, per file)
STOPPING = {(70, 150, 24): (0.25, 5, 30), (130, 200, 160): (0.2, 5, 20), (33, 64, 8): (0.3, 3, 18)}


def _assert_clear_stop(ref, tolerance, maxIterations):
    assert ref['iterations'] < maxIterations and len(ref['criteria']) >= 2
    assert ref['criteria'][-1] <= tolerance / 1.5, ref['criteria']
    assert all(c >= tolerance * 1.5 for c in ref['criteria'][:-1]), ref['criteria']


@functools.lru_cache(maxsize=None)
def _stopping_reference(F, N, K):
    tolerance, every, most = STOPPING[(F, N, K)]
    V = _factors(F, N, K, 3)[0]
    return [R.klnmf_until_converged(V[b], K, most, 0, tolerance, every) for b in range(3)]


def _engine(F, N, batch, **kw):
    from gcc_nmf_amd.engine import GCCNMFEngine
    windowSize, T = 2 * (F - 1), N // 2
    hop = windowSize // 2
    return GCCNMFEngine(windowSize + hop * (T - 1), windowSize=windowSize, hopSize=hop, batch=batch, numTargets=2, numTDOAs=16, **kw)


def _close(got, want):
    return np.abs(got - want).max() <= 1e-4 * np.abs(want).max()


@pytest.mark.parametrize('F,N,K', SHAPES)
def test_stopping_against_the_restatement(F, N, K):
    import gcc_nmf_amd.gccNMFFunctions as G
    tolerance, every, most = STOPPING[(F, N, K)]
    V = _factors(F, N, K, 3)[0]
    refs = _stopping_reference(F, N, K)
    for ref in refs:
        _assert_clear_stop(ref, tolerance, most)
    eng = _engine(F, N, 3, dictionarySize=K, numIterations=most, tolerance=tolerance, checkEvery=every)
    assert (eng.g.F, eng.g.N, eng.g.K) == (F, N, K)
    eng.V[:, :F, :N] = torch.from_numpy(np.array(V)).to(eng.device)
    eng.klnmf()
    assert not eng.chain_failed()
    counts, trace = eng.get_iterations(), eng.get_divergence_trace()
    We, He = eng.get_WH()
    Dend = eng.get_divergence()
    for b, ref in enumerate(refs):
        W, H, info = G.performKLNMFUntilConverged(V[b], K, most, 0, tolerance=tolerance, checkEvery=every)
        print('stopping (%d, %d, %d) file %d: restatement %d iterations, criteria %s; function %d, engine %d'
              % (F, N, K, b, ref['iterations'], ref['criteria'], info['iterations'], counts[b]))
        assert info['iterations'] == ref['iterations'] == counts[b]
        assert _close(W, ref['W']) and _close(H, ref['H']) and _close(We[b], ref['W']) and _close(He[b], ref['H'])
        checks = len(ref['divergences'])
        assert [it for it, _ in info['divergences']] == [it for it, _ in ref['divergences']]
        for c in range(checks):
            assert abs(info['divergences'][c][1] - ref['divergences'][c][1]) <= ref['bars'][c], (c, info['divergences'][c], ref['divergences'][c])
            assert abs(trace[c, b] - ref['divergences'][c][1]) <= ref['bars'][c], (c, trace[c, b], ref['divergences'][c])
        assert (trace[checks - 1:, b] == trace[checks - 1, b]).all() and Dend[b] == trace[checks - 1, b]      # frozen where it stopped


def test_files_converge_independently_of_their_batch():
    """A near-exact low-rank file and two noisy ones stop at different checks; each gets, to the bit, what it gets beside a copy of itself."""
    F, N, K, tolerance, every, most = 70, 150, 8, 0.11, 5, 40
    V = np.stack([R.low_rank_plus_noise(F, N, 6, noise, seed) for noise, seed in ((0.0, 1), (0.3, 2), (1.0, 3))])
    kw = dict(dictionarySize=K, numIterations=most, tolerance=tolerance, checkEvery=every)
    eng = _engine(F, N, 3, **kw)
    eng.V[:, :F, :N] = torch.from_numpy(np.array(V)).to(eng.device)
    eng.klnmf()
    counts, (W, H), trace = eng.get_iterations(), eng.get_WH(), eng.get_divergence_trace()
    print('independence: iterations', counts, 'restatement', [R.klnmf_until_converged(v, K, most, 0, tolerance, every)['iterations'] for v in V])
    assert len(set(counts.tolist())) == 3 and counts.min() >= every and np.isfinite(W).all() and np.isfinite(H).all()
    pair = _engine(F, N, 2, **kw)
    for b in range(3):
        pair.V[:, :F, :N] = torch.from_numpy(np.array(V[b])).to(pair.device)
        pair.klnmf()
        Wp, Hp = pair.get_WH()
        assert pair.get_iterations().tolist() == [counts[b]] * 2
        assert np.array_equal(Wp[0], W[b]) and np.array_equal(Hp[0], H[b]) and np.array_equal(Wp[1], W[b]) and np.array_equal(Hp[1], H[b])
        tp = pair.get_divergence_trace()
        assert np.array_equal(tp[:, 0], trace[:len(tp), b]) and (trace[len(tp) - 1:, b] == tp[-1, 0]).all()


def test_tolerance_none_is_the_single_call_to_the_bit():
    F, N, K = SHAPES[0]
    V = _factors(F, N, K, 3)[0]
    eng = _engine(F, N, 3, dictionarySize=K, numIterations=12)
    eng.V[:, :F, :N] = torch.from_numpy(np.array(V)).to(eng.device)
    eng.klnmf()
    W, H = eng.get_WH()
    D = eng.get_divergence()
    with pytest.raises(ValueError):
        eng.get_iterations()
    with pytest.raises(ValueError):
        eng.get_divergence_trace()
    for b in range(3):
        assert abs(D[b] - R.kl_divergence(V[b], W[b], H[b])) <= R.value_bar(V[b], W[b], H[b])
    assert np.array_equal(eng.get_WH()[0], W) and np.array_equal(eng.get_WH()[1], H)          # get_divergence left them alone
    # the call klnmf() has always made: one gccnmf_klnmf over the batch from the broadcast initial factors
    lib = _lib()
    Wd, Hd = eng.W0.unsqueeze(0).repeat(3, 1, 1), eng.H0.unsqueeze(0).repeat(3, 1, 1)
    ws = torch.zeros(lib.gccnmf_klnmf_workspace_floats(F, N, K, 3), dtype=torch.float32, device=eng.device)
    assert lib.gccnmf_klnmf(eng.V.data_ptr(), Wd.data_ptr(), Hd.data_ptr(), ws.data_ptr(), F, N, K, 3, 12, 0.0, 1e-16, 0,
                            torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(Wd[:, :F, :K].cpu().numpy(), W) and np.array_equal(Hd[:, :K, :N].cpu().numpy(), H)


@functools.lru_cache(maxsize=None)
def _dictionary(F, K):
    """A plausible pre-trained dictionary: a few oracle iterations on another low-rank V."""
    from oracle import gccnmf_oracle as O
    return O.performKLNMF(R.low_rank_plus_noise(F, 90, 5, 0.3, 99), K, 8, 0)[0]


@pytest.mark.parametrize('initialH', ['random', 'ones'])
def test_fixed_dictionary(initialH):
    from gcc_nmf_amd.engine import inferKLNMFCoefficients
    F, N, K = SHAPES[0]
    tolerance, every, most = 0.1, 5, 30
    V = _factors(F, N, K, 3)[0]
    Wf = _dictionary(F, K)
    refs = [R.klnmf_until_converged(V[b], K, most, 0, tolerance, every, fixedW=Wf, initialH=initialH) for b in range(3)]
    for ref in refs:
        _assert_clear_stop(ref, tolerance, most)
    eng = _engine(F, N, 3, dictionaryW=Wf, initialH=initialH, numIterations=most, tolerance=tolerance, checkEvery=every)
    eng.V[:, :F, :N] = torch.from_numpy(np.array(V)).to(eng.device)
    eng.klnmf()
    counts, trace = eng.get_iterations(), eng.get_divergence_trace()
    We, He = eng.get_WH()
    Hi, info = inferKLNMFCoefficients(V, Wf, most, initialH=initialH, tolerance=tolerance, checkEvery=every)
    H1, info1 = inferKLNMFCoefficients(V[1], Wf, most, initialH=initialH, tolerance=tolerance, checkEvery=every)
    assert isinstance(info1['iterations'], int) and info1['iterations'] == refs[1]['iterations'] and np.array_equal(H1, Hi[1])
    for b, ref in enumerate(refs):
        print('fixed dictionary (%s) file %d: restatement %d iterations, criteria %s; engine %d' % (initialH, b, ref['iterations'], ref['criteria'], counts[b]))
        assert counts[b] == ref['iterations'] == info['iterations'][b]
        assert np.array_equal(We[b], Wf) and _close(He[b], ref['H']) and np.array_equal(Hi[b], He[b])
        for c in range(len(ref['divergences'])):
            assert abs(trace[c, b] - ref['divergences'][c][1]) <= ref['bars'][c]
            assert info['divergences'][c][0] == ref['divergences'][c][0] and info['divergences'][c][1][b] == trace[c, b]
    plain = inferKLNMFCoefficients(V, Wf, 7, initialH=initialH)                       # no tolerance: H alone, as before
    assert isinstance(plain, np.ndarray) and plain.shape == (3, K, N)


def _ragged_against_per_length_engines(lengths, tuned, **kw):
    """A ragged engine and one ordinary engine per length on the same mixtures, both after stft() and klnmf(): yields
    (ragged engine, length, the caller's indexes of that length, the per-length engine)."""
    from gcc_nmf_amd import _hip
    from gcc_nmf_amd.engine import GCCNMFEngine, RaggedGCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_mixture
    xs = [synthetic_mixture(300 + i, numSamples=n) for i, n in enumerate(lengths)]
    e = GCCNMFEngine(lengths=lengths, **kw)
    assert isinstance(e, RaggedGCCNMFEngine) and len(e.sub) == 2
    e.upload(xs)
    for sub in e.sub.values():
        sub.stft()
    e.klnmf()
    lib = _hip.lib()
    out = []
    for n in sorted(set(lengths)):
        idx = [i for i, m in enumerate(lengths) if m == n]
        ref = GCCNMFEngine(n, batch=len(idx), **kw)
        ref.upload(np.stack([xs[i] for i in idx]))
        ref.stft()
        try:
            # (an equal-length batch of a few files takes the small-batch tiles by itself; tuning key 2 = 1 puts it on the tiles of a
            # batch at scale, which the ragged launch runs: the same bits)
            assert not tuned or lib.gccnmf_set_tuning(2, 1) == 0
            ref.klnmf()
            torch.cuda.synchronize()
        finally:
            lib.gccnmf_set_tuning(2, 0)
        out.append((e, n, idx, ref))
    return out


def test_ragged_engine_divergence_after_one_ragged_launch():
    """tolerance=None and two lengths: one ragged chained launch, the factors copied back to the per-length engines; get_divergence()
    is each file's D in the caller's order -- the bits an engine of that length alone gives, and the float64 value of those factors."""
    K = 256
    rows = _ragged_against_per_length_engines([160000, 80000] * 8 + [160000], True, dictionarySize=K, numIterations=3)
    e = rows[0][0]
    assert e.ragged_klnmf_used is True and e.tolerance is None
    D = e.get_divergence()
    assert D.shape == (17,) and D.dtype == np.float64
    with pytest.raises(ValueError):
        e.get_iterations()
    with pytest.raises(ValueError):
        e.get_divergence_trace()
    for _, n, idx, ref in rows:
        sub = e.sub[n]
        assert torch.equal(sub.W, ref.W) and torch.equal(sub.H, ref.H)
        assert np.array_equal(D[idx], ref.get_divergence())
        g, k = sub.g, len(idx) - 1
        V, W, H = sub.V[k, :g.F, :g.N].cpu().numpy(), sub.W[k, :g.F, :K].cpu().numpy(), sub.H[k, :K, :g.N].cpu().numpy()
        want, bar = R.kl_divergence(V, W, H), R.value_bar(V, W, H)
        print('ragged, length %d, file %d: |error| = %.3g = %.3g of the bar' % (n, idx[k], abs(D[idx[k]] - want), abs(D[idx[k]] - want) / bar))
        assert abs(D[idx[k]] - want) <= bar


def test_ragged_engine_with_a_tolerance_runs_each_length_as_its_own_batch():
    """tolerance= and checkEvery= reach the per-length engines, which converge as batches of their own (no ragged launch); the three
    getters return every file's count, divergence and trace in the caller's order, equal to what an engine of that length alone gives."""
    kw = dict(dictionarySize=24, numIterations=30, numTargets=2, numTDOAs=16, tolerance=0.05, checkEvery=3)
    rows = _ragged_against_per_length_engines([9216, 5888, 9216], False, **kw)
    e = rows[0][0]
    assert e.ragged is None and e.ragged_klnmf_used is False
    assert all(sub.tolerance == 0.05 and sub.checkEvery == 3 and sub.iters == 30 for sub in e.sub.values())
    counts, D, traces = e.get_iterations(), e.get_divergence(), e.get_divergence_trace()
    assert counts.shape == (3,) and counts.dtype == np.int64 and D.shape == (3,) and len(traces) == 3
    print('ragged with a tolerance: iterations', counts, 'D', D)
    assert (counts >= 3).all() and (counts % 3 == 0).all()
    for _, n, idx, ref in rows:
        sub = e.sub[n]
        assert torch.equal(sub.W, ref.W) and torch.equal(sub.H, ref.H)
        assert counts[idx].tolist() == ref.get_iterations().tolist()
        assert np.array_equal(D[idx], ref.get_divergence())
        rt = ref.get_divergence_trace()
        for k, i in enumerate(idx):
            assert traces[i].shape == (rt.shape[0],) and np.array_equal(traces[i], rt[:, k]) and traces[i][-1] == D[i]
