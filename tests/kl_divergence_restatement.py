"""NumPy restatement of what the KL-divergence stage and the convergence-stopped KL-NMF compute (no GPU, no project code but the
oracle's initial factors): the reference for tests/test_kl_divergence_host.py and tests/test_gpu_kl_divergence.py.

    D(V || W.H) = sum_{f, n} V log(V / R) - V + R,   R = W.H,   an element with V = 0 contributing R alone

is the objective of performKLNMF (gccNMF/gccNMFFunctions.py:69-83); the reference never evaluates it."""
import numpy as np

from oracle import gccnmf_oracle as O


def kl_divergence(V, W, H):
    """float64 D(V || W.H) of the given factors (whatever their dtype: they are widened first, R is a float64 product)."""
    V, W, H = np.asarray(V, np.float64), np.asarray(W, np.float64), np.asarray(H, np.float64)
    R = W @ H
    pos = V > 0
    logs = np.zeros_like(V)
    logs[pos] = V[pos] * np.log(V[pos] / R[pos])
    return float((logs - V + R).sum())


def value_bar(V, W, H):
    """The absolute bar on a float32-GEMM evaluation of D against kl_divergence on the same float32 factors:
    (8 + K) * 2^-24 * sum(V + R) -- a handful of float32 roundings per element, each of magnitude <= max(V, R), plus the GEMM's worst
    case K * 2^-24 * R error in R weighted by |1 - V / R| <= (V + R) / R."""
    V, W, H = np.asarray(V, np.float64), np.asarray(W, np.float64), np.asarray(H, np.float64)
    return (8 + W.shape[1]) * 2.0 ** -24 * float((V + W @ H).sum())


def klnmf_until_converged(V, K, maxIterations, alpha, tolerance, checkEvery, eps=1e-16, seed=0, fixedW=None, initialH='random'):
    """oracle.gccnmf_oracle.performKLNMF's loop, float32 as the reference does it, in chunks of `checkEvery` iterations (the last one
    shorter where maxIterations cuts it).  After each chunk D = kl_divergence of the float32 factors; the run stops at the first check
    with D_prev - D < tolerance * D_prev or D <= 0, D_prev of the first check being the divergence of the initial factors.
    fixedW (F, K): only H is updated (performKLNMF's H update with W never touched), from the drawn H0 or from ones.
    Returns dict(W, H, iterations, divergences=[(iteration, D), ...] from (0, D0), criteria=[(D_prev - D) / D_prev of every check],
    bars=[value_bar of the factors behind every entry of divergences])."""
    V = np.asarray(V, np.float32)
    W, H = O.initKLNMF(V.shape[0], V.shape[1], K, eps, seed)
    if fixedW is not None:
        W = np.asarray(fixedW, np.float32).copy()
        if initialH == 'ones':
            H = np.ones_like(H)
    D_prev = kl_divergence(V, W, H)
    divergences, criteria, bars, done = [(0, D_prev)], [], [value_bar(V, W, H)], 0
    while done < maxIterations:
        for _ in range(min(checkEvery, maxIterations - done)):
            H *= np.dot(W.T, V / np.dot(W, H)) / (np.sum(W, axis=0)[:, np.newaxis] + np.float32(alpha) + np.float32(eps))
            if fixedW is None:
                W *= np.dot(V / np.dot(W, H), H.T) / np.sum(H, axis=1)
                norms = np.sqrt(np.sum(W ** 2, 0))
                W /= norms
                H *= norms[:, np.newaxis]
            done += 1
        D = kl_divergence(V, W, H)
        divergences.append((done, D))
        bars.append(value_bar(V, W, H))
        criteria.append((D_prev - D) / D_prev)
        stop = D_prev - D < tolerance * D_prev or D <= 0
        D_prev = D
        if stop:
            break
    return dict(W=W, H=H, iterations=done, divergences=divergences, criteria=criteria, bars=bars)


def low_rank_plus_noise(F, N, rank, noise, seed, zeros=5):
    """A non-negative (F, N) float32 V = (A.B) * (1 + noise * u) with `zeros` ISOLATED zero entries (never a whole zero row or column:
    the reference's own updates turn those into NaN)."""
    rng = np.random.RandomState(seed)
    A = rng.rand(F, rank) + 0.05
    B = rng.rand(rank, N) + 0.05
    V = (A @ B) * (1 + noise * rng.rand(F, N))
    for i in range(zeros):
        V[(7 + 13 * i) % F, (11 + 29 * i) % N] = 0
    return V.astype(np.float32)
