"""What EM iterations behind the spatial reconstruction buy (``spatialIterations``), on the CPU in float64: no device
involved.

The pipeline and the mixtures are those of scripts/spatial_filter_study.py: the NumPy oracle up to the coefficient masks, the ratio
mask of tests/ratio_restatement.py, then tests/spatial_em_restatement.py for n EM iterations of the local Gaussian model and the
oracle's inverse STFT.  Scores: the mean stereo image SDR of the sources under the best assignment of outputs to sources.  n = 0 is the
spatial mode of profiles/r12a_spatial_filter_study.json.  Two variants that lost are kept on record beside the contract: 'r_first'
(the covariances are updated first, from C_i / v_i with the old powers, and the new powers are taken against the NEW covariances) and 'power' (a power-weighted covariance,
sum C_i / (1/2 sum tr C_i), instead of the mean of C_i / v'_i).  Writes one JSON record (default
profiles/r17a_spatial_em_study.json) and prints it."""
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
import spatial_em_restatement as EM                                 # noqa: E402

VARIANTS = {'em': {}, 'r_first': dict(order='r_first'), 'power': dict(weighting='power')}


def study(x, images, K, iterations, counts, sampleRate=16000, ws=1024, hop=256):
    S = len(images)
    r = O.runGCCNMF(x, sampleRate, ws, hop, 128, 1.0, S, dictionarySize=K, numIterations=iterations, return_intermediates=True)
    ratio = R.ratio_one_hot(r['W'], r['H'], np.nanargmax(r['G'], axis=0), S, r['X'])

    def score(spec):
        y = O.getTargetSignalEstimates(spec.astype(np.complex64), ws, hop, np.hanning)
        sdr, perm = SR.best_assignment_sdr(y, images, ws)
        return dict(image_sdr_db=[round(float(v), 3) for v in sdr], mean_db=round(float(sdr.mean()), 3), outputs=list(perm))

    out = dict(tdoa_indexes=r['idx'], shape=dict(S=S, F=int(r['X'].shape[1]), T=int(r['X'].shape[2])), ratio=score(ratio))
    for name, variant in VARIANTS.items():
        v, Rt = SR.powers(ratio), SR.covariances(ratio)
        rows, done = {}, 0
        for n in counts:
            for _ in range(n - done):
                v, Rt = EM.em_step(v, Rt, r['X'], **variant)
            done = n
            rows[str(n)] = score(SR.spatial_filter(ratio, r['X']) if n == 0 else EM.filter_with(v, Rt, r['X']))
            print(name, n, rows[str(n)]['mean_db'], file=sys.stderr, flush=True)
        out[name] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=128)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--counts', default='0,1,2,3,5,10,20,40')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r17a_spatial_em_study.json'))
    args = ap.parse_args()
    counts = sorted(int(v) for v in args.counts.split(','))
    rec = dict(K=args.K, iterations=args.iterations, n_fft=1024, hop=256, loading=SR.LOADING, counts=counts, variants=sorted(VARIANTS),
               mixtures={})
    for name, kw in (('reverberant_seed0', dict(seed=0)), ('reverberant_seed1', dict(seed=1)), ('anechoic_seed0', dict(seed=0, reverbGain=0.0))):
        x, images = reverberant_mixture(returnSources=True, **kw)
        rec['mixtures'][name] = study(x, images, args.K, args.iterations, counts)
    text = json.dumps(rec)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
