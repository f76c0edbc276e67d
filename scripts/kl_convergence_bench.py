"""What the KL-divergence stage costs, and what stopping KL-NMF on it saves.

  (1) one stage-7 launch (gccnmf_klnmf_stage: D(V || W.H), csrc/divergence.hip) against one stage-3 launch (R = V / (W.H)) at the headline
      shape: 64 synthetic 10 s mixtures, n_fft 1024, hop 256 (F = 513, N = 1244), K = 1024 -- and at K = 128;
  (2) the same 64-file batch through GCCNMFEngine.klnmf(): 100 fixed iterations against tolerance in {1e-3, 1e-4} with checkEvery = 10 and
      100 as the maximum: iterations used per file, ms per step (the STFT is outside the timed region), the divergences reached.
HIP events time each after warm-up.  Prints one JSON record."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gcc_nmf_amd import _hip                                       # noqa: E402
from gcc_nmf_amd.engine import GCCNMFEngine                        # noqa: E402
from gcc_nmf_amd.synthetic import synthetic_batch                  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--K', default='1024,128')
    ap.add_argument('--tolerances', default='1e-3,1e-4')
    ap.add_argument('--check-every', type=int, default=10)
    args = ap.parse_args()
    lib = _hip.lib()
    B, it = args.files, args.iterations
    x = synthetic_batch(0, B)
    s = torch.cuda.current_stream().cuda_stream
    med = lambda v: float(np.median(v))
    rec = dict(files=B, max_iterations=it, check_every=args.check_every, n_fft=1024, hop=256, K={})
    for K in [int(k) for k in args.K.split(',')]:
        eng = GCCNMFEngine(x.shape[-1], batch=B, dictionarySize=K, numIterations=it)
        eng.upload(x)
        eng.stft()
        g = eng.g
        eng.klnmf()
        fixed_D = eng.get_divergence()
        ws = torch.zeros(lib.gccnmf_klnmf_workspace_floats(g.F, g.N, K, B), device='cuda')

        def stage(n):
            return lambda: _hip.check(lib.gccnmf_klnmf_stage(eng.V.data_ptr(), eng.W.data_ptr(), eng.H.data_ptr(), ws.data_ptr(), g.F, g.N, K, B,
                                                             0.0, 1e-16, 0, n, s), 'stage %d' % n)
        # each stage in a loop of its own, stage 3 first: once stage 7 has written its partials into R, stage 0 has to run before any of
        # stages 1 - 6 does again
        stage(0)()
        stage(3)()
        torch.cuda.synchronize()
        t3 = timed(stage(3), 10)
        stage(7)()
        torch.cuda.synchronize()
        t7 = timed(stage(7), 10)
        stage(0)()
        r = dict(stage3_ms=med(t3), stage3_spread=[min(t3), max(t3)], stage7_ms=med(t7), stage7_spread=[min(t7), max(t7)],
                 stage7_over_stage3=med(t7) / med(t3), stage3_includes_k4a=bool(lib.gccnmf_klnmf_plan(g.F, g.N, K, B, 0) & 4))
        tf = timed(eng.klnmf, args.repeats)
        r['fixed'] = dict(iterations=it, ms_per_step=med(tf), spread=[min(tf), max(tf)], divergence_min_median_max=[float(fixed_D.min()), float(np.median(fixed_D)),
                                                                                                                    float(fixed_D.max())])
        for tol in [float(t) for t in args.tolerances.split(',')]:
            eng.tolerance, eng.checkEvery = tol, args.check_every
            eng.klnmf()
            tt = timed(eng.klnmf, args.repeats)
            n, D = eng.get_iterations(), eng.get_divergence()
            r['tolerance_%g' % tol] = dict(ms_per_step=med(tt), spread=[min(tt), max(tt)], over_fixed=med(tt) / med(tf), iterations=n.tolist(),
                                           iterations_min_median_max=[int(n.min()), float(np.median(n)), int(n.max())],
                                           divergence_over_fixed_min_median_max=[float((D / fixed_D).min()), float(np.median(D / fixed_D)),
                                                                                 float((D / fixed_D).max())])
            eng.tolerance = None
        rec['K'][K] = r
        print(K, json.dumps(r), file=sys.stderr, flush=True)
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
