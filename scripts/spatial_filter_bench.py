"""The reconstruct() stage alone: the ratio-mask mode (one fused launch, csrc/ratio.hip) against the spatial mode (the same launch, then
the covariance reduction and the 2 x 2 filter of csrc/spatial.hip), alternated in one process; the direct mode beside them.

64 synthetic 10 s mixtures, n_fft 1024, hop 256, S = 3, K = 128 and K = 1024.  The factors, the arg-max image and X come from a short run
of the pipeline itself (--iterations KL-NMF iterations: the stage's time does not depend on their values); HIP events time each call after
warm-up; median of --repeats with the range.  The spatial stage's own time is the difference of the two medians; the bytes it must move
per file are (S 2 + 2) Fp Tp 8 B terms: spec read twice (once per launch) and written once, X read once.  ``--modes direct,ratio`` times
the modes an earlier revision has, so that the same script measures its library (GCCNMF_HIP_LIB=<path>); the SHA-256 of every mode's
spectrograms is in the record, to show that two libraries computed the same bits.  Prints one JSON record."""
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

HBM_MEASURED = 6.29e12        # bytes/s, float4 copy on an MI355X (8.0e12 is the data sheet's figure)


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
    ap.add_argument('--modes', default='direct,ratio,spatial')
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
        r = dict(F=g.F, T=g.T, Fp=g.Fp, Tp=g.Tp)
        for m in modes:
            r[m + '_ms'] = float(np.median(t[m]))
            r[m + '_range'] = [min(t[m]), max(t[m])]
            run(m)
            torch.cuda.synchronize()
            r[m + '_spec_sha256'] = hashlib.sha256(eng.spec.cpu().numpy().tobytes()).hexdigest()
        if 'ratio' in modes and 'spatial' in modes:
            stage = r['spatial_ms'] - r['ratio_ms']
            # spec read twice and written once, X read once
            moved = B * (3 * 2 * S + 2) * g.Fp * g.Tp * 8
            r['spatial_stage_ms'] = stage
            r['spatial_over_ratio'] = r['spatial_ms'] / r['ratio_ms']
            r['spatial_stage_bytes'] = moved
            r['spatial_stage_bytes_per_s'] = moved / (stage * 1e-3)
            r['spatial_stage_fraction_of_measured_hbm'] = moved / (stage * 1e-3) / HBM_MEASURED
        rec['K'][K] = r
        print(K, json.dumps(r), file=sys.stderr, flush=True)
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
