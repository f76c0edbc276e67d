"""Host side of the KL-divergence stage and the convergence-stopped KL-NMF: the argument rules (decided before any device is looked
for) and the NumPy restatement the GPU tests are measured against."""
import math

import numpy as np
import pytest

import kl_divergence_restatement as R


def test_check_convergence_accepts():
    from gcc_nmf_amd import _hip
    assert _hip.check_convergence(None, 10, 100) == (None, 10, 100)
    assert _hip.check_convergence(1e-4, 1, 0) == (1e-4, 1, 0)
    tol, every, iters = _hip.check_convergence(np.float32(0.5), np.int64(3), np.int32(7))
    assert (tol, every, iters) == (0.5, 3, 7) and type(tol) is float and type(every) is int and type(iters) is int
    assert _hip.check_convergence(0.999999, 1000000, 5)[0] == 0.999999


@pytest.mark.parametrize('tolerance', [0, 0.0, 1, 1.0, -1e-4, 2.5, float('nan'), float('inf'), -float('inf'), '1e-4', True, [1e-4], 1e-4 + 0j])
def test_check_convergence_rejects_tolerance(tolerance):
    from gcc_nmf_amd import _hip
    with pytest.raises(ValueError):
        _hip.check_convergence(tolerance, 10, 100)


@pytest.mark.parametrize('checkEvery', [0, -1, 2.0, 2.5, None, '3', True, float('nan')])
def test_check_convergence_rejects_check_every(checkEvery):
    from gcc_nmf_amd import _hip
    with pytest.raises(ValueError):
        _hip.check_convergence(1e-4, checkEvery, 100)
    with pytest.raises(ValueError):            # checked whether or not a tolerance is given
        _hip.check_convergence(None, checkEvery, 100)


@pytest.mark.parametrize('numIterations', [-1, 1.5, None, True])
def test_check_convergence_rejects_iterations(numIterations):
    from gcc_nmf_amd import _hip
    with pytest.raises(ValueError):
        _hip.check_convergence(1e-4, 10, numIterations)


def test_new_names_and_keywords_raise_before_any_device(monkeypatch):
    import inspect
    import torch
    import gcc_nmf_amd.gccNMFFunctions as G
    from gcc_nmf_amd import engine
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    assert list(inspect.signature(G.performKLNMFUntilConverged).parameters) == \
        ['V', 'dictionarySize', 'maxIterations', 'sparsityAlpha', 'tolerance', 'checkEvery', 'epsilon', 'seedValue']
    defaults = dict((k, p.default) for k, p in inspect.signature(G.performKLNMFUntilConverged).parameters.items())
    assert (defaults['tolerance'], defaults['checkEvery'], defaults['epsilon'], defaults['seedValue']) == (1e-4, 10, 1e-16, 0)
    assert list(inspect.signature(G.getKLDivergence).parameters) == ['V', 'W', 'H']
    assert list(inspect.signature(G.performKLNMF).parameters) == ['V', 'dictionarySize', 'numIterations', 'sparsityAlpha', 'epsilon', 'seedValue']
    V = np.ones((4, 6), np.float32)
    with pytest.raises(ValueError):
        G.performKLNMFUntilConverged(V, 2, 10, 0, tolerance=2.0)
    with pytest.raises(ValueError):
        G.performKLNMFUntilConverged(V, 2, 10, 0, checkEvery=0)
    with pytest.raises(ValueError):
        G.performKLNMFUntilConverged(V, 2, 10, 0, tolerance=None)
    for cls in (engine.GCCNMFEngine, engine.RaggedGCCNMFEngine):
        p = inspect.signature(cls.__init__).parameters
        assert p['tolerance'].default is None and p['checkEvery'].default == 10
    p = inspect.signature(engine.inferKLNMFCoefficients).parameters
    assert p['tolerance'].default is None and p['checkEvery'].default == 10
    with pytest.raises(ValueError):
        engine.GCCNMFEngine(16000, tolerance=1.5)
    with pytest.raises(ValueError):
        engine.GCCNMFEngine(16000, checkEvery=0)
    with pytest.raises(ValueError):
        engine.GCCNMFEngine(lengths=[16000, 20000], tolerance=0.0)
    with pytest.raises(ValueError):
        engine.inferKLNMFCoefficients(V, np.ones((4, 2), np.float32), 10, tolerance=-1.0)


def test_restatement_closed_form_2x2_with_a_zero():
    W = np.array([[1.0, 2.0], [0.5, 1.0]])
    H = np.array([[1.0, 0.25], [0.5, 2.0]])
    # R = W.H = [[2, 4.25], [1, 2.125]]
    V = np.array([[3.0, 0.0], [1.0, 4.0]])
    want = (3 * math.log(3 / 2.0) - 3 + 2) + 4.25 + (1 * math.log(1 / 1.0) - 1 + 1) + (4 * math.log(4 / 2.125) - 4 + 2.125)
    assert R.kl_divergence(V, W, H) == pytest.approx(want, rel=1e-15)
    assert R.kl_divergence(V.astype(np.float32), W.astype(np.float32), H.astype(np.float32)) == pytest.approx(want, rel=1e-15)   # (all exact in float32)


def test_restatement_is_exactly_zero_for_v_equal_wh():
    rng = np.random.RandomState(3)
    W = np.round(rng.rand(9, 4) * 16) / 16 + 0.25          # short binary fractions: W.H is exact in float64
    H = np.round(rng.rand(4, 11) * 16) / 16 + 0.25
    assert R.kl_divergence(W @ H, W, H) == 0.0


def test_restatement_honours_max_iterations_and_the_rule():
    V = R.low_rank_plus_noise(20, 30, 3, 0.3, 1)
    assert (V == 0).sum() == 5 and (V.sum(0) > 0).all() and (V.sum(1) > 0).all()
    r = R.klnmf_until_converged(V, 4, 7, 0, 1e-12, 3)                       # never converges: 3 + 3 + 1 iterations
    assert r['iterations'] == 7 and [it for it, _ in r['divergences']] == [0, 3, 6, 7] and len(r['criteria']) == 3
    assert len(r['bars']) == 4 and all(b > 0 for b in r['bars'])
    assert R.klnmf_until_converged(V, 4, 0, 0, 0.5, 3)['iterations'] == 0
    r = R.klnmf_until_converged(V, 4, 30, 0, 0.5, 2)                        # a loose tolerance stops at the first check below it
    stop = next(i for i, c in enumerate(r['criteria']) if c < 0.5)
    assert r['iterations'] == 2 * (stop + 1) < 30 and len(r['criteria']) == stop + 1
    from oracle import gccnmf_oracle as O
    Wo, Ho = O.performKLNMF(V, 4, r['iterations'], 0)
    assert np.array_equal(r['W'], Wo) and np.array_equal(r['H'], Ho)        # the same loop as the oracle's, to the bit
    D = [d for _, d in r['divergences']]
    assert D[-1] == R.kl_divergence(V, r['W'], r['H']) and all(a > b for a, b in zip(D, D[1:]))
    Wf = Wo.copy()
    f = R.klnmf_until_converged(V, 4, 5, 0, 1e-12, 5, fixedW=Wf, initialH='ones')
    assert np.array_equal(f['W'], Wf) and f['iterations'] == 5 and f['divergences'][0][1] == R.kl_divergence(V, Wf, np.ones((4, 30)))


def test_converge_klnmf_plumbing_against_the_restatement():
    """engine.converge_klnmf (chunks, per-file rule, snapshots put back, trace) with the oracle's float32 loop standing in for the
    library: files that stop at different checks get exactly what the restatement gives each of them alone."""
    import torch
    from gcc_nmf_amd.engine import check_iterations, converge_klnmf
    from oracle import gccnmf_oracle as O
    F, N, K, tolerance, every, most = 70, 150, 8, 0.11, 5, 40
    V = np.stack([R.low_rank_plus_noise(F, N, 6, noise, seed) for noise, seed in ((0.0, 1), (0.3, 2), (1.0, 3))])
    refs = [R.klnmf_until_converged(v, K, most, 0, tolerance, every) for v in V]
    assert len(set(r['iterations'] for r in refs)) == 3
    W0, H0 = O.initKLNMF(F, N, K, 1e-16, 0)
    W, H = torch.from_numpy(np.stack([W0] * 3)), torch.from_numpy(np.stack([H0] * 3))
    calls = []

    def launch(n, first):
        calls.append((n, first))
        for b in range(3):
            w, h = W[b].numpy(), H[b].numpy()
            for _ in range(n):
                h *= np.dot(w.T, V[b] / np.dot(w, h)) / (np.sum(w, axis=0)[:, np.newaxis] + np.float32(0) + np.float32(1e-16))
                w *= np.dot(V[b] / np.dot(w, h), h.T) / np.sum(h, axis=1)
                norms = np.sqrt(np.sum(w ** 2, 0))
                w /= norms
                h *= norms[:, np.newaxis]

    iterations, trace = converge_klnmf(launch, lambda: np.array([R.kl_divergence(V[b], W[b].numpy(), H[b].numpy()) for b in range(3)]),
                                       [W, H], most, tolerance, every)
    assert iterations.tolist() == [r['iterations'] for r in refs]
    assert calls == [(every, i == 0) for i in range(max(iterations) // every)]
    assert check_iterations(trace, every, most) == [every * c for c in range(len(trace))] and check_iterations(range(4), 3, 7) == [0, 3, 6, 7]
    for b, r in enumerate(refs):
        assert np.array_equal(W[b].numpy(), r['W']) and np.array_equal(H[b].numpy(), r['H'])
        D = [d for _, d in r['divergences']]
        assert trace[:len(D), b].tolist() == D and (trace[len(D) - 1:, b] == D[-1]).all()
    # the maximum cuts the last chunk short and stops everything; a NaN divergence stops nothing
    W2, H2 = torch.from_numpy(np.stack([W0] * 3)), torch.from_numpy(np.stack([H0] * 3))
    calls.clear()
    W, H = W2, H2
    iterations, trace = converge_klnmf(launch, lambda: np.array([R.kl_divergence(V[b], W[b].numpy(), H[b].numpy()) for b in range(3)]),
                                       [W, H], 7, 1e-9, every)
    assert iterations.tolist() == [7, 7, 7] and calls == [(5, True), (2, False)] and trace.shape == (3, 3)
    iterations, trace = converge_klnmf(lambda n, first: None, lambda: np.array([np.nan, 1.0]), [torch.zeros(2, 1)], 20, 0.5, every)
    assert iterations.tolist() == [20, 5] and np.isnan(trace[:, 0]).all()
