"""Temporal-continuity KL-NMF (gccnmf_klnmf with GCCNMF_FLAG_CONTINUITY, csrc/nmf_smooth.hip) against KL-NMF on plain launches.

64 synthetic 10 s mixtures, n_fft 1024, hop 256, at K = 128 and K = 1024, two column segments [L | R] as the engine runs it.  Per K, the
per-iteration time of
  (a) a temporal-continuity iteration -- seven plain launches: the 128 x 64 register-staging tile for stages 1 - 4, the row launches, the
      two-pass W update;
  (b) a KL iteration on plain launches (tuning keys 21 = 16 = 17 = 0), the yardstick: the form the new path is to be compared with;
  (c) a KL iteration as the library launches it by default, for context;
the per-stage times of (a) and (b) (gccnmf_klnmf_stage, stages 1 - 5), stage 2 of the Euclidean iteration (the same tile with two products)
and the bytes stage 2's row launch has to move -- H read once, Gm and Gp written -- against the HBM copy rate the repository records
(6.29 TB/s, profiles/r12a_spatial_filter_bench.json); the row launch is not addressable on its own, so its time is bounded from above by
stage 2 as a whole (a kernel trace separates the two launches).
The calls alternate in one process; HIP events time each whole call after a warm-up, the median over the repeats is reported with the
spread.  Writes one JSON record (profiles/r21a_temporal_continuity_bench.json)."""
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
HBM_COPY_RATE = 6.29e12                     # bytes / s, as recorded with profiles/r12a_spatial_filter_bench.json


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
    ap.add_argument('--weight', type=float, default=1.0)
    ap.add_argument('--out', default=os.path.join(HERE, '..', 'profiles', 'r21a_temporal_continuity_bench.json'))
    args = ap.parse_args()
    lib = _hip.lib()
    B, it = args.files, args.iterations
    x = synthetic_batch(0, B)
    s = torch.cuda.current_stream().cuda_stream
    med = lambda v: float(np.median(v))
    rec = dict(files=B, iterations=it, n_fft=1024, hop=256, repeats=args.repeats, weight=args.weight, segments=2, hbm_copy_rate_bytes_per_s=HBM_COPY_RATE, K={})

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
        ws = torch.zeros(max(_hip.klnmf_continuity_workspace_floats(g.F, g.N, K, B), _hip.klnmf_divergence_workspace_floats(g.F, g.N, K, B, 'euclidean')),
                         device='cuda')
        cont = _hip.GCCNMF_FLAG_CONTINUITY | _hip.GCCNMF_FLAG_CONTINUITY_STEREO
        Kw, Bw = _hip.continuity_words(K, B, args.weight)
        assert lib.gccnmf_klnmf_plan(g.F, g.N, Kw, Bw, cont) == 128

        def reset():
            W.copy_(W0)
            H.copy_(H0)

        def call(f):
            k, b = (Kw, Bw) if f & cont else (K, B)
            _hip.check(lib.gccnmf_klnmf(V.data_ptr(), W.data_ptr(), H.data_ptr(), ws.data_ptr(), g.F, g.N, k, b, it, 0.0, 1e-16, f, s), 'klnmf')

        def stage(st, f):
            k, b = (Kw, Bw) if f & cont else (K, B)
            _hip.check(lib.gccnmf_klnmf_stage(V.data_ptr(), W.data_ptr(), H.data_ptr(), ws.data_ptr(), g.F, g.N, k, b, 0.0, 1e-16, f, st, s), 'stage')

        def kl_plain():
            tune(PLAIN_KEYS)
            try:
                call(0)
            finally:
                tune(DEFAULT_KEYS)

        tune(PLAIN_KEYS)
        plain_plan = lib.gccnmf_klnmf_plan(g.F, g.N, K, B, 0)
        tune(DEFAULT_KEYS)
        runs = dict(continuity=lambda: call(cont), kl_plain=kl_plain, kl_default=lambda: call(0))
        t = {k: [] for k in runs}
        for f in runs.values():          # warm-up
            reset()
            f()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for k, f in runs.items():
                t[k].append(timed(f, before=reset))

        # stage by stage, in sequence on a live state (the first round is the warm-up): the continuity iteration, the KL iteration on plain
        # launches, and stage 2 of the Euclidean iteration on the state its own stage 1 left
        def stage_rounds(f, stages, keys=None):
            st = {n: [] for n in stages}
            if keys:
                tune(keys)
            try:
                reset()
                stage(0, f)
                for _ in range(args.repeats + 1):
                    for n in range(1, 6):
                        ms = timed(lambda: stage(n, f))
                        if n in st:
                            st[n].append(ms)
            finally:
                if keys:
                    tune(DEFAULT_KEYS)
            return {str(n): 1e3 * med(v[1:]) for n, v in st.items()}
        cont_us = stage_rounds(cont, range(1, 6))
        finite = bool(torch.isfinite(W).all()) and bool(torch.isfinite(H[:, :K, :g.N]).all())
        kl_us = stage_rounds(0, range(1, 6), PLAIN_KEYS)
        eu_us = stage_rounds(_hip.GCCNMF_FLAG_DIVERGENCE_EUCLIDEAN, [2])
        per_it = {k: med(v) / it for k, v in t.items()}
        row_bytes = 3 * 4 * B * K * g.N             # H read once (the second read is an L2 hit by design), Gm and Gp written
        rec['K'][str(K)] = dict(
            F=g.F, N=g.N, kl_plain_plan=plain_plan, kl_default_plan=lib.gccnmf_klnmf_plan(g.F, g.N, K, B, 0),
            continuity_ms_per_iteration=per_it['continuity'], kl_plain_ms_per_iteration=per_it['kl_plain'],
            kl_default_ms_per_iteration=per_it['kl_default'], continuity_over_kl_plain=per_it['continuity'] / per_it['kl_plain'],
            continuity_over_kl_default=per_it['continuity'] / per_it['kl_default'],
            spread_ms_per_call={k: [min(v), max(v)] for k, v in t.items()},
            continuity_stage_us=cont_us, kl_plain_stage_us=kl_us, euclidean_stage_2_us=eu_us['2'],
            continuity_stage_2_over_euclidean_stage_2=cont_us['2'] / eu_us['2'],
            row_launch_bytes=row_bytes, row_launch_floor_us_at_hbm_copy_rate=1e6 * row_bytes / HBM_COPY_RATE,
            stage_2_extra_us_over_kl_plain=cont_us['2'] - kl_us['2'], factors_finite_after_stage_rounds=finite)
        print(K, json.dumps(rec['K'][str(K)]), file=sys.stderr, flush=True)
        del eng, ws
        torch.cuda.empty_cache()
    with open(args.out, 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')
    print(json.dumps(rec, indent=1))


if __name__ == '__main__':
    main()
