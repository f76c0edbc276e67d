"""What a microphone array buys a mask-based GCC-NMF separation: CPU, float64, through the restatement
tests/array_restatement.py -- no device, no timing.

Three far-field talkers (synthetic.array_mixture) at 40 / 90 / 130 degrees in front of a 4-microphone line (x = 0, 0.2, 0.5, 1.0 m),
--files seeded mixtures of --seconds each, n_fft 1024, hop 256, K = --K, --iterations KL-NMF iterations, 181 azimuths.  Each mixture is
separated twice: with all four microphones (M = 4, six pairs), and with the outer pair alone (M = 2, one pair, the same 1 m aperture).
The score is the mean image SDR of BSS Eval (tests/bss_eval_restatement.py, --taps filter taps), on the outer pair's channels for both
runs (the same true images) and on all four channels for M = 4; ISR / SIR / SAR and the chosen azimuths are recorded beside it.

The ratio mask is applied per channel, so the array enters only through the localisation and the atom assignment; the array gain proper
needs an M x M spatial filter.  Writes one JSON record (default profiles/r23a_array_study.json) and prints it."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import array_restatement as A          # noqa: E402
import bss_eval_restatement as E       # noqa: E402
import fft_checks as K                 # noqa: E402

LINE = np.array([[0.0, 0, 0], [0.2, 0, 0], [0.5, 0, 0], [1.0, 0, 0]])
SOUND = 340.29
AZIMUTHS = [40, 90, 130]


def klnmf64(V, Kk, iterations, epsilon=1e-16, seed=0):
    """performKLNMF (gccNMF/gccNMFFunctions.py:69-83) in float64 from the float32 draws of klnmf_initial_factors."""
    rs = np.random.RandomState(seed)
    W = rs.random_sample((V.shape[0], Kk)).astype(np.float32).astype(np.float64) + epsilon
    H = rs.random_sample((Kk, V.shape[1])).astype(np.float32).astype(np.float64) + epsilon
    for _ in range(iterations):
        H *= W.T.dot(V / W.dot(H)) / (W.sum(axis=0)[:, None] + epsilon)
        W *= (V / W.dot(H)).dot(H.T) / H.sum(axis=1)
        norms = np.sqrt((W ** 2).sum(axis=0))
        W /= norms
        H *= norms[:, None]
    return W, H


def separate(x, positions, n_fft, hop, Kk, iterations, S, D):
    """x (M, n) float32 -> (waveforms (S, M, L) float64, chosen direction indexes, status)."""
    M, n = x.shape
    T = 1 + (n - n_fft) // hop
    w = np.hanning(n_fft).astype(np.float32)
    xx = np.concatenate([x, np.zeros((M % 2, n), np.float32)])
    X = np.concatenate([K.stft64(xx[c:c + 2], w, n_fft, hop, T)[0] for c in range(0, M, 2)])[:M]
    V, Cs = A.features(X)
    W, H = klnmf64(V, Kk, iterations)
    freqs = np.linspace(0, 8000.0, n_fft // 2 + 1)
    tau = A.pair_tdoas_from_geometry(positions, A.azimuth_directions(D), SOUND)
    ang, _ = A.angular(Cs, freqs, tau)
    idx, status = A.peaks(ang.mean(axis=1), S)
    if status:
        return None, idx, status
    G, _ = A.scores(Cs, W, freqs, tau, idx)
    spec = A.ratio_one_hot(W, H, A.argmax(G), S, X)
    flat = spec.reshape(S * M, spec.shape[2], T)
    if (S * M) % 2:
        flat = np.concatenate([flat, np.zeros_like(flat[:1])])
    y, _ = A.istft(flat.astype(np.complex64), w, n_fft, hop, hop / float(n_fft) * 2)
    return y[:S * M].reshape(S, M, -1), idx, status


def score(images, y, channels, n_fft, taps):
    """Mean image criteria over the sources on ``channels``: waveform sample y[n] belongs to image sample n + n_fft // 2."""
    L = y.shape[-1]
    s = images[:, channels, n_fft // 2:n_fft // 2 + L]
    sdr, isr, sir, sar, perm = E.bss_eval_images(s, y[:, channels], taps)
    return dict(sdr=float(np.mean(sdr)), isr=float(np.mean(isr)), sir=float(np.mean(sir)), sar=float(np.mean(sar)),
                sdr_per_source=[float(v) for v in sdr], perm=[int(p) for p in perm])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=4)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--K', type=int, default=128)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--taps', type=int, default=64)
    ap.add_argument('--directions', type=int, default=181)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r23a_array_study.json'))
    args = ap.parse_args()
    from gcc_nmf_amd.synthetic import array_mixture
    n, n_fft, hop, S = int(round(args.seconds * 16000)), 1024, 256, 3
    rec = dict(files=args.files, seconds=args.seconds, K=args.K, iterations=args.iterations, taps=args.taps, directions=args.directions,
               n_fft=n_fft, hop=hop, microphones_x=LINE[:, 0].tolist(), azimuths=AZIMUTHS, runs=[])
    for seed in range(args.files):
        x, images = array_mixture(seed, LINE, AZIMUTHS, n, 16000, returnImages=True)
        run = dict(seed=seed)
        y4, idx4, st4 = separate(x, LINE, n_fft, hop, args.K, args.iterations, S, args.directions)
        y2, idx2, st2 = separate(x[[0, 3]], LINE[[0, 3]], n_fft, hop, args.K, args.iterations, S, args.directions)
        run['M4_indexes'], run['M2_indexes'] = [int(i) for i in idx4], [int(i) for i in idx2]
        if st4 == 0:
            run['M4_outer_pair'] = score(images, y4, [0, 3], n_fft, args.taps)
            run['M4_all_channels'] = score(images, y4, [0, 1, 2, 3], n_fft, args.taps)
        if st2 == 0:
            run['M2_outer_pair'] = score(images[:, [0, 3]], y2, [0, 1], n_fft, args.taps)
        rec['runs'].append(run)
        print(json.dumps(run), file=sys.stderr, flush=True)
    summary = {}
    for key in ('M4_outer_pair', 'M4_all_channels', 'M2_outer_pair'):
        got = [r[key] for r in rec['runs'] if key in r]
        summary[key] = dict(files_scored=len(got))
        for crit in ('sdr', 'isr', 'sir', 'sar'):
            summary[key]['mean_' + crit] = float(np.mean([g[crit] for g in got])) if got else None
    exact = lambda key: sum(1 for r in rec['runs'] if r[key] == AZIMUTHS)
    summary['M4_files_with_exact_azimuths'], summary['M2_files_with_exact_azimuths'] = exact('M4_indexes'), exact('M2_indexes')
    rec['summary'] = summary
    text = json.dumps(rec)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
