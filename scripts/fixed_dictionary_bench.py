"""Fixed-dictionary KL-NMF (gccnmf_klnmf with GCCNMF_FLAG_FIXED_W) against the same inference with existing calls and the blind call.

64 synthetic 10 s mixtures, n_fft 1024, hop 256, 100 iterations, K in {64, 128, 256, 512, 1024}:
  (a) the fused fixed-dictionary call; (b) gccnmf_klnmf_shared_begin + 100 x gccnmf_klnmf_shared_step_a + _finish on the same V / W / H;
  (c) the blind gccnmf_klnmf at the same shape; (e) (a) for one file alone.
(a), (b) and (c) alternate in one process; HIP events time each after warm-up.  Prints one JSON record."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gcc_nmf_amd import _hip                                       # noqa: E402
from gcc_nmf_amd.engine import GCCNMFEngine, klnmf_initial_factors  # noqa: E402
from gcc_nmf_amd.synthetic import synthetic_batch                  # noqa: E402

PEAK = 157.3e12
FIXED_W = 1 << 16


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
    ap.add_argument('--K', default='64,128,256,512,1024')
    args = ap.parse_args()
    lib = _hip.lib()
    B, it = args.files, args.iterations
    x = synthetic_batch(0, B)
    s = torch.cuda.current_stream().cuda_stream
    rec = dict(files=B, iterations=it, n_fft=1024, hop=256, K={})
    for K in [int(k) for k in args.K.split(',')]:
        eng = GCCNMFEngine(x.shape[-1], batch=B, dictionarySize=K, numIterations=it)
        eng.upload(x)
        eng.stft()
        g = eng.g
        W = eng.W0.clone()
        H0 = eng.H0.unsqueeze(0).expand(B, -1, -1).contiguous()
        H = torch.empty_like(H0)
        ws = torch.zeros(lib.gccnmf_klnmf_workspace_floats(g.F, g.N, K, B), device='cuda')
        Wb = W.unsqueeze(0).expand(B, -1, -1).contiguous()
        sws = torch.zeros(lib.gccnmf_klnmf_shared_workspace_floats(g.F, g.N, K, B), device='cuda')
        part = torch.zeros(lib.gccnmf_klnmf_shared_partial_floats(g.F, K), device='cuda')

        def run_a(batch=B):
            H.copy_(H0)
            _hip.check(lib.gccnmf_klnmf(eng.V.data_ptr(), W.data_ptr(), H.data_ptr(), ws.data_ptr(), g.F, g.N, K, batch, it, 0.0, 1e-16,
                                        FIXED_W, s), 'fixed')

        def run_b():
            H.copy_(H0)
            _hip.check(lib.gccnmf_klnmf_shared_begin(W.data_ptr(), sws.data_ptr(), g.F, g.N, K, B, s), 'begin')
            for _ in range(it):
                _hip.check(lib.gccnmf_klnmf_shared_step_a(eng.V.data_ptr(), W.data_ptr(), H.data_ptr(), sws.data_ptr(), part.data_ptr(),
                                                          g.F, g.N, K, B, 0.0, 1e-16, s), 'step_a')
            _hip.check(lib.gccnmf_klnmf_shared_finish(H.data_ptr(), sws.data_ptr(), g.F, g.N, K, B, s), 'finish')

        def run_c():
            Wb.copy_(W.unsqueeze(0).expand_as(Wb))
            H.copy_(H0)
            _hip.check(lib.gccnmf_klnmf(eng.V.data_ptr(), Wb.data_ptr(), H.data_ptr(), ws.data_ptr(), g.F, g.N, K, B, it, 0.0, 1e-16, 0, s),
                       'blind')

        for f in (run_a, run_b, run_c):
            f()
        torch.cuda.synchronize()
        ta, tb, tc = [], [], []
        for _ in range(args.repeats):
            ta += timed(run_a, 1)
            tb += timed(run_b, 1)
            tc += timed(run_c, 1)
        te = timed(lambda: run_a(1), args.repeats)
        flop = 4.0 * g.F * K * g.N * B * it
        med = lambda v: float(np.median(v))
        rec['K'][K] = dict(a_ms=med(ta), a_spread=[min(ta), max(ta)], b_ms=med(tb), b_spread=[min(tb), max(tb)], c_ms=med(tc),
                           c_spread=[min(tc), max(tc)], e_one_file_ms=med(te), a_tflops=flop / med(ta) / 1e9,
                           a_fraction_of_peak=flop / (med(ta) * 1e-3) / PEAK, a_over_c=med(ta) / med(tc), a_over_b=med(ta) / med(tb))
        print(K, json.dumps(rec['K'][K]), file=sys.stderr, flush=True)
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
