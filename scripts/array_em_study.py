"""What the EM refinement of the M x M spatial filter buys the microphone-array separation: CPU, float64, through the
restatements tests/array_restatement.py, tests/array_spatial_restatement.py and tests/array_em_restatement.py -- no device, no timing.

The mixtures, the line, the separation up to the ratio-mode estimates and the scoring are those of scripts/array_spatial_study.py (three
far-field talkers in front of the 4-microphone line; --files seeded mixtures of --seconds each, n_fft 1024, hop 256, K = --K, --iterations
KL-NMF iterations, 181 azimuths).  Each mixture is separated with all four microphones and with the outer pair alone, and each of the two
is reconstructed from the same masks with the spatial filter after n = 0, 5, 10 and 20 EM iterations (include/gccnmf_array_em.h; at M = 2
the stereo recursion).  The score is the mean image SDR / SIR / ISR / SAR of BSS Eval on the outer pair's channels.

Writes one JSON record (default profiles/r26a_array_em_study.json) and prints it."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.join(HERE, '..')
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, HERE)

import array_em_restatement as AE          # noqa: E402
import array_restatement as A              # noqa: E402
import array_spatial_restatement as AS     # noqa: E402
import array_spatial_study as spatial      # noqa: E402
import array_study as base                 # noqa: E402
import fft_checks as K                     # noqa: E402

ITERATIONS = (0, 5, 10, 20)


def separate(x, positions, n_fft, hop, Kk, iterations, S, D):
    """x (M, n) float32 -> ({n: waveforms (S, M, L) float64}, chosen direction indexes, status): the steps of array_spatial_study.separate,
    then the filter after every n of ITERATIONS, from the same arg-max image."""
    M, n = x.shape
    T = 1 + (n - n_fft) // hop
    w = np.hanning(n_fft).astype(np.float32)
    xx = np.concatenate([x, np.zeros((M % 2, n), np.float32)])
    X = np.concatenate([K.stft64(xx[c:c + 2], w, n_fft, hop, T)[0] for c in range(0, M, 2)])[:M]
    V, Cs = A.features(X)
    W, H = base.klnmf64(V, Kk, iterations)
    freqs = np.linspace(0, 8000.0, n_fft // 2 + 1)
    tau = A.pair_tdoas_from_geometry(positions, A.azimuth_directions(D), base.SOUND)
    ang, _ = A.angular(Cs, freqs, tau)
    idx, status = A.peaks(ang.mean(axis=1), S)
    if status:
        return None, idx, status
    G, _ = A.scores(Cs, W, freqs, tau, idx)
    E = A.ratio_one_hot(W, H, A.argmax(G), S, X)
    out, cache = {}, {}
    for m in ITERATIONS:
        if m == 0:
            filtered = AS.spatial_filter(E, X, np.float64)
        else:
            v, R = AE.refine(E, X, m, np.float64, cache=cache)
            filtered = AE.filter_with(v, R, X, np.float64)
        out[m] = spatial.waveforms(filtered, w, n_fft, hop)
    return out, idx, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=4)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--K', type=int, default=128)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--taps', type=int, default=64)
    ap.add_argument('--directions', type=int, default=181)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r26a_array_em_study.json'))
    args = ap.parse_args()
    from gcc_nmf_amd.synthetic import array_mixture
    LINE, AZIMUTHS = base.LINE, base.AZIMUTHS
    n, n_fft, hop, S = int(round(args.seconds * 16000)), 1024, 256, 3
    rec = dict(files=args.files, seconds=args.seconds, K=args.K, iterations=args.iterations, taps=args.taps, directions=args.directions,
               n_fft=n_fft, hop=hop, microphones_x=LINE[:, 0].tolist(), azimuths=AZIMUTHS, loading=AS.LOADING,
               spatial_iterations=list(ITERATIONS), runs=[])
    for seed in range(args.files):
        x, images = array_mixture(seed, LINE, AZIMUTHS, n, 16000, returnImages=True)
        run = dict(seed=seed)
        y4, idx4, st4 = separate(x, LINE, n_fft, hop, args.K, args.iterations, S, args.directions)
        y2, idx2, st2 = separate(x[[0, 3]], LINE[[0, 3]], n_fft, hop, args.K, args.iterations, S, args.directions)
        run['M4_indexes'], run['M2_indexes'] = [int(i) for i in idx4], [int(i) for i in idx2]
        for m in ITERATIONS:
            if st4 == 0:
                run['M4_n%d_outer_pair' % m] = base.score(images, y4[m], [0, 3], n_fft, args.taps)
            if st2 == 0:
                run['M2_n%d_outer_pair' % m] = base.score(images[:, [0, 3]], y2[m], [0, 1], n_fft, args.taps)
        rec['runs'].append(run)
        print(json.dumps(run), file=sys.stderr, flush=True)
    summary = {}
    for key in ['M%d_n%d_outer_pair' % (M, m) for M in (4, 2) for m in ITERATIONS]:
        got = [r[key] for r in rec['runs'] if key in r]
        summary[key] = dict(files_scored=len(got))
        for crit in ('sdr', 'isr', 'sir', 'sar'):
            summary[key]['mean_' + crit] = float(np.mean([g[crit] for g in got])) if got else None
    rec['summary'] = summary
    text = json.dumps(rec)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
