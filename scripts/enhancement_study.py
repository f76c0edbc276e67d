"""Is offline speech enhancement by atom TDOA worth having?  On the CPU in float64: no device involved.

tests/atom_tdoa_restatement.py (float64_enhancement) runs the whole pipeline -- the NumPy oracle's STFT and KL-NMF, every atom's arg-max
TDOA over the whole grid, the talker / noise masks around the strongest direction, the ratio-mask reconstruction, the oracle's inverse
STFT -- on synthetic.speech_in_noise_mixture at three SNRs: 4 s at 16 kHz, K = 64, 100 iterations, 128 TDOAs, boxcar epsilon = 4 unless
told otherwise.  SDR is taken against the clean talker passed through the same STFT / iSTFT pair.  ``--epsilons`` adds other boxcar
widths, ``--window`` the window-function mask (epsilon 5, beta 2).  Prints one JSON record (profiles/r14a_enhancement_study.json)."""
import argparse
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from gcc_nmf_amd.synthetic import speech_in_noise_mixture           # noqa: E402
import atom_tdoa_restatement as A                                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--snrs', default='0,5,-5')
    ap.add_argument('--epsilons', default='4,2,8')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--samples', type=int, default=64000)
    ap.add_argument('--atoms', type=int, default=64)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--window', action='store_true')
    args = ap.parse_args()
    rec = dict(generator='synthetic.speech_in_noise_mixture', seed=args.seed, samples=args.samples, sampleRate=16000, K=args.atoms,
               iterations=args.iterations, numTDOAs=128, reconstruction='ratio', precision='float64 (CPU)', runs=[])
    for snr in [float(v) for v in args.snrs.split(',')]:
        x, clean = speech_in_noise_mixture(args.seed, snr, numSamples=args.samples)
        settings = [dict(window=0, eps=float(e)) for e in args.epsilons.split(',')]
        if args.window:
            settings.append(dict(window=1, eps=5.0, beta=2.0, nf=0.0))
        for kw in settings:
            sdr_in, sdr_out, target = A.float64_enhancement(x, clean, K=args.atoms, iterations=args.iterations, **kw)
            rec['runs'].append(dict(snr_db=snr, mask='window' if kw['window'] else 'boxcar', epsilon=kw['eps'], target_index=target,
                                    input_sdr_db=round(float(sdr_in), 2), output_sdr_db=round(float(sdr_out), 2),
                                    gain_db=round(float(sdr_out - sdr_in), 2)))
            print(json.dumps(rec['runs'][-1]), file=sys.stderr, flush=True)
    print(json.dumps(rec, indent=1))


if __name__ == '__main__':
    main()
