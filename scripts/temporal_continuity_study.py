"""What the temporal-continuity term of KL-NMF does to the separation, on the CPU in float64: no device involved.

The NumPy oracle (oracle/gccnmf_oracle.py) states the pipeline around the factorisation; the factorisation itself is
tests/temporal_continuity_restatement.py's float64 iteration from the reference's initial factors, with two column segments [L | R] as the
engine runs it.  Mixtures with known source images: the three of scripts/spatial_filter_study.py (two seeds of
synthetic.reverberant_mixture and its anechoic form).  For every dictionary size and weight: the mean stereo image SDR of the direct,
ratio-mask and spatial reconstructions under the best assignment of outputs to sources, the KL divergence and the continuity cost of the
factors.  The weight is ABSOLUTE, in units of V; the record also holds it relative to the mean of V.  Writes one JSON record."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from oracle import gccnmf_oracle as O                              # noqa: E402
from gcc_nmf_amd.synthetic import reverberant_mixture               # noqa: E402
import ratio_restatement as R                                       # noqa: E402
import spatial_restatement as SR                                    # noqa: E402
import temporal_continuity_restatement as C                         # noqa: E402


def study(x, images, K, iterations, weights, sampleRate=16000, ws=1024, hop=256, numTDOAs=128, d=1.0):
    S = len(images)
    X = O.computeComplexMixtureSpectrogram(x, ws, hop, np.hanning)
    F = X.shape[1]
    f = np.linspace(0, sampleRate / 2.0, F)
    V = O.magnitudeSpectrogramV(X)
    coh = O.spectralCoherence(X)
    idx = O.estimateTargetTDOAIndexesFromAngularSpectrum(np.mean(O.getAngularSpectrogram(coh, f, d, numTDOAs), axis=-1), d, numTDOAs, S)
    W0, H0 = O.initKLNMF(F, V.shape[1], K, 1e-16, 0)
    out = dict(tdoa_indexes=[int(i) for i in idx], mean_V=round(float(V.mean()), 5), weights={})
    for weight in weights:
        W, H = C.iterate(V, W0, H0, weight, 2, 0.0, 1e-16, iterations)
        W32, H32 = W.astype(np.float32), H.astype(np.float32)
        stereoH = np.array(np.hsplit(H32, 2))
        G = O.getTargetTDOAGCCNMFs(coh, d, numTDOAs, f, idx, W32, stereoH)
        direct = O.getTargetSpectrogramEstimates(O.getTargetCoefficientMasks(G, S), X, W32, stereoH)
        ratio = R.ratio_one_hot(W32, H32, np.nanargmax(G, axis=0), S, X)
        rec = dict(weight_over_mean_V=round(float(weight / V.mean()), 4), kl_divergence=round(C.kl(V, W, H), 3),
                   continuity_cost=round(C.cost(H, 2), 3))
        for name, spec in (('direct', direct), ('ratio', ratio), ('spatial', SR.spatial_filter(ratio, X))):
            y = O.getTargetSignalEstimates(spec.astype(np.complex64), ws, hop, np.hanning)
            sdr, perm = SR.best_assignment_sdr(y, images, ws)
            rec[name] = dict(image_sdr_db=[round(float(v), 3) for v in sdr], mean_db=round(float(sdr.mean()), 3), outputs=[int(p) for p in perm])
        out['weights']['%g' % weight] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', default='128,64')
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--weights', default='0,0.01,0.1,1,10')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r21a_temporal_continuity_study.json'))
    args = ap.parse_args()
    weights = [float(v) for v in args.weights.split(',')]
    rec = dict(iterations=args.iterations, n_fft=1024, hop=256, segments=2, weights=weights, K={})
    for K in (int(v) for v in args.K.split(',')):
        rec['K'][str(K)] = {}
        for name, kw in (('reverberant_seed0', dict(seed=0)), ('reverberant_seed1', dict(seed=1)), ('anechoic_seed0', dict(seed=0, reverbGain=0.0))):
            x, images = reverberant_mixture(returnSources=True, **kw)
            rec['K'][str(K)][name] = study(x, images, K, args.iterations, weights)
            print(K, name, json.dumps(rec['K'][str(K)][name]), file=sys.stderr, flush=True)
    # the summary the documents quote: mean image SDR over the three mixtures, per dictionary size, mode and weight
    rec['summary'] = dict((K, dict((mode, dict(('%g' % w, round(float(np.mean([m['weights']['%g' % w][mode]['mean_db'] for m in mix.values()])), 3))
                                               for w in weights)) for mode in ('direct', 'ratio', 'spatial'))) for K, mix in rec['K'].items())
    with open(args.out, 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')
    print(json.dumps(rec['summary']))


if __name__ == '__main__':
    main()
