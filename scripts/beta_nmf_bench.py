"""Itakura-Saito and Euclidean NMF (gccnmf_klnmf with GCCNMF_FLAG_DIVERGENCE_IS / _EUCLIDEAN, csrc/nmf_beta.hip) against KL-NMF.

64 synthetic 10 s mixtures, n_fft 1024, hop 256, at K = 128 and K = 1024.  Per K, the per-iteration time of
  (a) an IS iteration, (b) a Euclidean iteration -- five plain launches each, six GEMM-units;
  (c) a KL iteration on plain launches (tuning keys 21 = 16 = 17 = 0: four GEMM-units, the form the new path is to be compared with);
  (d) a KL iteration as the library launches it by default (chained / fused where it chains or fuses), for context;
and the per-stage times of the IS iteration (gccnmf_klnmf_stage, stages 1-5).
The calls alternate in one process; HIP events time each whole call after a warm-up, the median over the repeats is reported with the
spread.  Prints one JSON record (profiles/r19a_beta_nmf_bench.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
from gcc_nmf_amd import _hip                                       # noqa: E402
from gcc_nmf_amd.engine import GCCNMFEngine                        # noqa: E402
from gcc_nmf_amd.synthetic import synthetic_batch                  # noqa: E402

PLAIN_KEYS = {21: 0, 16: 0, 17: 0}          # GCCNMF_TUNE="21=0,16=0,17=0"
DEFAULT_KEYS = {21: 1, 16: 1, 17: 1}


def timed(fn, before=None):
    if before is not None:
        before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--iterations', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--atoms', default='128,1024')
    args = ap.parse_args()
    lib = _hip.lib()
    B, it = args.files, args.iterations
    x = synthetic_batch(0, B)
    s = torch.cuda.current_stream().cuda_stream
    med = lambda v: float(np.median(v))
    rec = dict(files=B, iterations=it, n_fft=1024, hop=256, repeats=args.repeats, K={})

    def tune(keys):
        for k, v in keys.items():
            _hip.check(lib.gccnmf_set_tuning(k, v), 'gccnmf_set_tuning')

    for K in (int(v) for v in args.atoms.split(',')):
        eng = GCCNMFEngine(x.shape[-1], batch=B, dictionarySize=K, numIterations=it)
        eng.upload(x)
        eng.stft()
        g, V = eng.g, eng.V
        W0 = eng.W0.unsqueeze(0).expand(B, -1, -1).contiguous()
        H0 = eng.H0.unsqueeze(0).expand(B, -1, -1).contiguous()
        W, H = torch.empty_like(W0), torch.empty_like(H0)
        ws = torch.zeros(_hip.klnmf_divergence_workspace_floats(g.F, g.N, K, B, 'is'), device='cuda')
        flags = dict(is_=_hip.GCCNMF_FLAG_DIVERGENCE_IS, euclidean=_hip.GCCNMF_FLAG_DIVERGENCE_EUCLIDEAN)
        assert lib.gccnmf_klnmf_plan(g.F, g.N, K, B, flags['is_']) == 64

        def reset():
            W.copy_(W0)
            H.copy_(H0)

        def call(f):
            _hip.check(lib.gccnmf_klnmf(V.data_ptr(), W.data_ptr(), H.data_ptr(), ws.data_ptr(), g.F, g.N, K, B, it, 0.0, 1e-16, f, s), 'klnmf')

        def stage(st, f):
            _hip.check(lib.gccnmf_klnmf_stage(V.data_ptr(), W.data_ptr(), H.data_ptr(), ws.data_ptr(), g.F, g.N, K, B, 0.0, 1e-16, f, st, s), 'stage')

        def kl_plain():
            tune(PLAIN_KEYS)
            try:
                call(0)
            finally:
                tune(DEFAULT_KEYS)

        tune(PLAIN_KEYS)
        plain_plan = lib.gccnmf_klnmf_plan(g.F, g.N, K, B, 0)
        tune(DEFAULT_KEYS)
        runs = dict(is_=lambda: call(flags['is_']), euclidean=lambda: call(flags['euclidean']), kl_plain=kl_plain, kl_default=lambda: call(0))
        t = {k: [] for k in runs}
        for f in runs.values():          # warm-up
            reset()
            f()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for k, f in runs.items():
                t[k].append(timed(f, before=reset))
        # the IS iteration stage by stage, in sequence on a live state (the first round is the warm-up)
        st = {n: [] for n in range(1, 6)}
        reset()
        stage(0, flags['is_'])
        for _ in range(args.repeats + 1):
            for n in range(1, 6):
                st[n].append(timed(lambda: stage(n, flags['is_'])))
        finite = bool(torch.isfinite(W).all()) and bool(torch.isfinite(H).all())
        per_it = {k: med(v) / it for k, v in t.items()}
        rec['K'][str(K)] = dict(
            F=g.F, N=g.N, kl_plain_plan=plain_plan, kl_default_plan=lib.gccnmf_klnmf_plan(g.F, g.N, K, B, 0),
            is_ms_per_iteration=per_it['is_'], euclidean_ms_per_iteration=per_it['euclidean'],
            kl_plain_ms_per_iteration=per_it['kl_plain'], kl_default_ms_per_iteration=per_it['kl_default'],
            is_over_kl_plain=per_it['is_'] / per_it['kl_plain'], euclidean_over_kl_plain=per_it['euclidean'] / per_it['kl_plain'],
            is_over_kl_default=per_it['is_'] / per_it['kl_default'],
            spread_ms_per_call={k: [min(v), max(v)] for k, v in t.items()},
            is_stage_us={str(n): 1e3 * med(v[1:]) for n, v in st.items()}, factors_finite_after_stage_rounds=finite)
        print(K, json.dumps(rec['K'][str(K)]), file=sys.stderr, flush=True)
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(rec, indent=1))


if __name__ == '__main__':
    main()
