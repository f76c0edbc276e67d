"""The reconstruct() stage alone: the direct mode (masked copies of H + a GEMM with the phase epilogue, csrc/gcc.hip) against the ratio-mask
mode (one fused launch, csrc/ratio.hip), alternated in one process.

64 synthetic 10 s mixtures, n_fft 1024, hop 256, S = 3, K = 128 and K = 1024.  The factors, the arg-max image and X come from a short run
of the pipeline itself (--iterations KL-NMF iterations: the stage's time does not depend on their values); HIP events time each call after
warm-up; median of --repeats with the spread.  ``--modes direct`` times the direct mode alone, so that the same script measures a library
of an earlier revision (GCCNMF_HIP_LIB=<path>); the SHA-256 of the direct mode's spectrograms is in the record, to show that two
libraries computed the same bits.  Prints one JSON record."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gcc_nmf_amd.engine import GCCNMFEngine                        # noqa: E402
from gcc_nmf_amd.synthetic import synthetic_batch                  # noqa: E402

PEAK = 157.3e12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--targets', type=int, default=3)
    ap.add_argument('--iterations', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--K', default='128,1024')
    ap.add_argument('--modes', default='direct,ratio')
    args = ap.parse_args()
    modes = args.modes.split(',')
    B, S = args.files, args.targets
    x = synthetic_batch(0, B)
    rec = dict(files=B, targets=S, n_fft=1024, hop=256, repeats=args.repeats, modes=modes, K={})
    for K in [int(k) for k in args.K.split(',')]:
        eng = GCCNMFEngine(x.shape[-1], batch=B, dictionarySize=K, numIterations=args.iterations, numTargets=S)
        eng.upload(x)
        eng.run()
        g = eng.g

        def run(mode):
            eng.reconstruction = mode
            eng.reconstruct()

        for m in modes:
            run(m)
        torch.cuda.synchronize()
        t = dict((m, []) for m in modes)
        for _ in range(args.repeats):
            for m in modes:
                t[m].append(timed(lambda: run(m)))
        # the MFMA work both modes share: 2 S products W (F x K) . (K x T) per file
        flop = 2.0 * g.F * K * g.T * 2 * S * B
        r = dict(F=g.F, T=g.T)
        for m in modes:
            med = float(np.median(t[m]))
            r[m + '_ms'] = med
            r[m + '_spread'] = [min(t[m]), max(t[m])]
            r[m + '_fraction_of_f32_mfma_peak'] = flop / (med * 1e-3) / PEAK
        if 'direct' in modes:
            run('direct')
            torch.cuda.synchronize()
            r['direct_spec_sha256'] = hashlib.sha256(eng.spec.cpu().numpy().tobytes()).hexdigest()
        if 'direct' in modes and 'ratio' in modes:
            r['ratio_over_direct'] = r['ratio_ms'] / r['direct_ms']
            r['bar'] = 1.0 + 1.0 / S
        rec['K'][K] = r
        print(K, json.dumps(r), file=sys.stderr, flush=True)
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
