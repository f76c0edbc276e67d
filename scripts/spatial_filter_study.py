"""What the spatial (multichannel Wiener) reconstruction buys over the ratio mask, on the CPU in float64: no device involved.

The NumPy oracle (oracle/gccnmf_oracle.py) runs the pipeline up to the coefficient masks; tests/ratio_restatement.py and
tests/spatial_restatement.py then state the two reconstructions, and the oracle's inverse STFT gives waveforms.  Mixtures with known
source images: two seeds of synthetic.reverberant_mixture (each source convolved per channel with its own short impulse response) and
the same generator with reverbGain = 0 (anechoic: the right channel holds delayed copies, the shape of synthetic_mixture).  Scores: the
stereo image SDR of every source (both channels pooled) under the best assignment of outputs to sources, and its mean.  ``--loadings``
adds the spatial mode at other diagonal loadings than GCCNMF_SPATIAL_LOADING.  Prints one JSON record."""
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


def study(x, images, K, iterations, loadings, sampleRate=16000, ws=1024, hop=256):
    S = len(images)
    r = O.runGCCNMF(x, sampleRate, ws, hop, 128, 1.0, S, dictionarySize=K, numIterations=iterations, return_intermediates=True)
    am = np.nanargmax(r['G'], axis=0)
    ratio = R.ratio_one_hot(r['W'], r['H'], am, S, r['X'])
    out = dict(tdoa_indexes=r['idx'])
    modes = {'direct': r['S'], 'ratio': ratio}
    for lam in loadings:
        modes['spatial' if lam == loadings[0] else 'spatial_loading_%g' % lam] = SR.spatial_filter(ratio, r['X'], loading=lam)
    for name, spec in modes.items():
        y = O.getTargetSignalEstimates(spec.astype(np.complex64), ws, hop, np.hanning)
        sdr, perm = SR.best_assignment_sdr(y, images, ws)
        out[name] = dict(image_sdr_db=[round(float(v), 3) for v in sdr], mean_db=round(float(sdr.mean()), 3), outputs=list(perm))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=128)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--loadings', default='1e-3,1e-2,1e-1', help='the first is GCCNMF_SPATIAL_LOADING, the others are studied beside it')
    args = ap.parse_args()
    loadings = [float(v) for v in args.loadings.split(',')]
    rec = dict(K=args.K, iterations=args.iterations, n_fft=1024, hop=256, loadings=loadings, mixtures={})
    for name, kw in (('reverberant_seed0', dict(seed=0)), ('reverberant_seed1', dict(seed=1)), ('anechoic_seed0', dict(seed=0, reverbGain=0.0))):
        x, images = reverberant_mixture(returnSources=True, **kw)
        rec['mixtures'][name] = study(x, images, args.K, args.iterations, loadings)
        print(name, json.dumps(rec['mixtures'][name]), file=sys.stderr, flush=True)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
