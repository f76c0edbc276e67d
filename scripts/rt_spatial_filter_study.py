"""What the online spatial (multichannel Wiener) filter of the real-time path buys over the per-channel mask, on the CPU in float64:
no device involved.

The real-time frame processor is restated causally in NumPy at the config-5 shape (window 512, hop 64, one frame per block, 64 TDOAs,
asymmetric analysis / synthesis windows with a 128-sample synthesis window, the config's coefficient inference): PHAT coherence, GCC-NMF
scores, arg-max over the TDOAs per atom and frame, the window-function mask (single target) or the one-hot arg-max over the targets
(multiple mode), the time-frequency mask -- oracle/rt_oracle.py's formulas, frame by frame -- and then tests/rt_spatial_restatement.py,
the contract of csrc/rt_spatial.hip, over the whole signal.  The dictionary is learned from the mixture's own magnitudes by KL-NMF (a
stand-in for a pre-trained one); the target TDOA indexes are the grid points nearest the true delays (the online localisation is not
what is studied).

Mixtures with known source images: two seeds of synthetic.reverberant_mixture and the same generator with reverbGain = 0 (anechoic).
Scores: stereo image SDR (both channels pooled).  Single-target enhancement: every talker in turn against the rest, filter off and
on for every tau; multiple mode, N = 3: per-source SDR under the best assignment.  The numbers are reported as they come out: the offline
figure (0.9 - 1.0 dB on reverberant mixtures, profiles/r12a_spatial_filter_study.json) is no prediction for a causal filter.
Prints one JSON record."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from oracle import rt_oracle as RO                                  # noqa: E402
from gcc_nmf_amd.synthetic import reverberant_mixture               # noqa: E402
import rt_spatial_restatement as RS                                 # noqa: E402
import spatial_restatement as SR                                    # noqa: E402

WS, HOP, SYNTH, D, RATE, SEPARATION_M = 512, 64, 128, 64, 16000, 1.0
DELAYS = (-20, 3, 27)
TAUS = (4, 8, 16, 32, 64, 128)


def frames_of(x):
    T = (x.shape[-1] - WS) // HOP + 1
    idx = np.arange(T)[:, None] * HOP + np.arange(WS)[None, :]
    return x[..., idx]                                              # (..., T, WS)


def klnmf(V, K, iterations, seed=0):
    rng = np.random.RandomState(seed)
    W, H = rng.rand(V.shape[0], K) + 0.02, rng.rand(K, V.shape[1]) + 0.02
    for _ in range(iterations):
        H *= (W.T @ (V / (W @ H + 1e-16))) / W.sum(axis=0)[:, None]
        W *= ((V / (W @ H + 1e-16)) @ H.T) / H.sum(axis=1)[None, :]
        W /= np.linalg.norm(W, axis=0)
    return W.astype(np.float32)


def front(x, W, nH):
    """The frame processor in front of the masks: X (2, F, T) complex64, the atoms' arg-max TDOA (K, T) and the target scores, the
    inferred coefficients h (2, K, T) (ones without inference)."""
    an, sy = RO.asymmetric_windows(WS, SYNTH)
    X = np.fft.rfft(frames_of(x.astype(np.float64)) * an, axis=-1).transpose(0, 2, 1).astype(np.complex64)
    with np.errstate(invalid='ignore', divide='ignore'):
        C = X[0] * X[1].conj() / np.abs(X[0]) / np.abs(X[1])
    C = np.where(np.isfinite(C), C, 0)
    F = WS // 2 + 1
    freqs = np.linspace(0, RATE / 2, F)
    maxTDOA = SEPARATION_M / 340.29
    taus = np.linspace(-maxTDOA, maxTDOA, D)
    E = np.exp(np.outer(freqs, -(2j * np.pi) * taus))              # (F, D)
    W64 = W.astype(np.float64)
    realGCC = C.real[:, :, None] * E.real[:, None, :] - C.imag[:, :, None] * E.imag[:, None, :]      # Re(C e), (F, T, D)
    G = (W64.T @ realGCC.reshape(F, -1)).reshape(W.shape[1], X.shape[2], D).transpose(2, 0, 1)         # (D, K, T)
    h = np.ones((2, W.shape[1], X.shape[2]))
    for c in range(2):
        v = np.abs(X[c]).astype(np.float64)
        for _ in range(nH):
            h[c] *= (W64.T @ RO.ratio0(v, W64 @ h[c])) / W64.sum(axis=0)[:, None]
    targets = [int(np.argmin(np.abs(taus * RATE - d))) for d in DELAYS]
    return X, G, h, targets, sy


def tf_masks(W, h, HMask):
    W64 = W.astype(np.float64)
    return np.stack([RO.ratio0(W64 @ (h[c] * HMask), W64 @ h[c]) for c in range(2)]).astype(np.float32)      # (2, F, T)


def synthesise(Y, sy, n):
    fr = np.fft.irfft(np.asarray(Y).transpose(0, 2, 1), n=WS, axis=-1) * sy      # (2, T, WS)
    y = np.zeros((2, n))
    for t in range(fr.shape[1]):
        y[:, t * HOP:t * HOP + WS] += fr[:, t]
    return y


def sdr_of(y, image):
    return float(SR.best_assignment_sdr(y[None], image[None], 0)[0][0])


def study(x, images, K, iterations, nH):
    n = x.shape[-1]
    V = np.concatenate([np.abs(np.fft.rfft(frames_of(x[c].astype(np.float64)) * np.hanning(WS), axis=-1)).T for c in range(2)], axis=1)
    W = klnmf(V, K, iterations)
    X, G, h, targets, sy = front(x, W, nH)
    F, T = X.shape[1:]
    am = np.argmax(G, axis=0)                                       # (K, T)
    out = dict(target_indexes=targets, frames=T)
    zero = lambda NC: np.zeros((NC, F, 4), np.float32)
    masked = lambda tf: (tf * X.real + 1j * (tf * X.imag)).astype(np.complex64)
    single = {'off': []}
    for j, tgt in enumerate(targets):                               # every talker in turn against the rest
        HMask = np.exp(-(np.abs(am - tgt) / 5.0) ** 2.0)            # epsilon 5, beta 2, noise floor 0 (the reference's defaults)
        Y = masked(tf_masks(W, h, HMask))
        single['off'].append(sdr_of(synthesise(Y, sy, n), images[j]))
        for tau in TAUS:
            Yf = RS.rt_spatial(Y[None], X, zero(2), tau, False)[0][0]
            single.setdefault('tau_%d' % tau, []).append(sdr_of(synthesise(Yf, sy, n), images[j]))
    out['single_target_talker_sdr_db'] = {k: dict(per_talker=[round(v, 3) for v in vs], mean=round(float(np.mean(vs)), 3)) for k, vs in single.items()}
    pick = np.argmax(G[targets], axis=0)                            # multiple mode: one-hot arg-max over the targets
    Ym = np.stack([masked(tf_masks(W, h, (pick == i).astype(np.float64))) for i in range(len(targets))])
    multi = {}
    for key, spec in [('off', Ym)] + [('tau_%d' % tau, RS.rt_spatial(Ym, X, zero(len(targets)), tau, True)[0]) for tau in TAUS]:
        y = np.stack([synthesise(spec[i], sy, n) for i in range(len(targets))])
        sdr, perm = SR.best_assignment_sdr(y, images, 0)
        multi[key] = dict(per_source=[round(float(v), 3) for v in sdr], mean=round(float(sdr.mean()), 3), outputs=list(perm))
    out['multiple_mode_sdr_db'] = multi
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=128)
    ap.add_argument('--iterations', type=int, default=60)
    ap.add_argument('--numHUpdates', type=int, default=2, help="config 5's own value")
    ap.add_argument('--samples', type=int, default=96000)
    args = ap.parse_args()
    rec = dict(K=args.K, iterations=args.iterations, numHUpdates=args.numHUpdates, windowSize=WS, hopSize=HOP, synthesisSize=SYNTH, numTDOAs=D,
               taus=list(TAUS), loading=RS.LOADING, mixtures={})
    for name, kw in (('reverberant_seed0', dict(seed=0)), ('reverberant_seed1', dict(seed=1)), ('anechoic_seed0', dict(seed=0, reverbGain=0.0))):
        x, images = reverberant_mixture(returnSources=True, numSamples=args.samples, **kw)
        rec['mixtures'][name] = study(x, images, args.K, args.iterations, args.numHUpdates)
        print(name, json.dumps(rec['mixtures'][name]), file=sys.stderr, flush=True)
    keys = ['off'] + ['tau_%d' % t for t in TAUS]
    mean = lambda what, k: round(float(np.mean([m[what][k]['mean'] for m in rec['mixtures'].values()])), 3)
    rec['mean_over_mixtures'] = dict(single_target=dict((k, mean('single_target_talker_sdr_db', k)) for k in keys),
                                     multiple_mode=dict((k, mean('multiple_mode_sdr_db', k)) for k in keys))
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
