"""Semi-supervised KL-NMF (gccnmf_klnmf with GCCNMF_FLAG_FREE_ATOMS) against the blind call on plain launches and the fixed-dictionary call.

64 synthetic 10 s mixtures, n_fft 1024, hop 256.  Per (K_fixed, n), K = K_fixed + n:
  per-iteration time of (a) the semi-supervised call, (b) the blind call at the same K with plain launches (tuning key 21 = 0: the form the
  semi-supervised iteration shares three GEMMs with; the default, chained where the library chains, is reported beside it), (c) the
  fixed-dictionary call at the same K;
  per-stage time of stage 4 + stage 5 (gccnmf_klnmf_stage) with the bits -- nmf_semi.hip: R.H_free^T and the free columns' W update -- and
  without them (the blind R.H^T + W update over all K atoms), on the same R and H, and stage 4 alone with the bits as bytes of R per second
  against the HBM copy rate recorded in profiles/r12a_spatial_filter_bench.json.
The calls alternate in one process; HIP events time each after a warm-up.  K is capped at 1024 by the call, so the large dictionary is
K_fixed = 1024 - n.  Prints one JSON record (profiles/r13a_semi_supervised_bench.json)."""
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

FIXED_W = 1 << 16


def timed(fn, reps, before=None):
    out = []
    for _ in range(reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def recorded_hbm_rate():
    """bytes per second of the HBM copy the spatial-filter bench measured on this kind of machine (its stage rate / its fraction)"""
    with open(os.path.join(HERE, '..', 'profiles', 'r12a_spatial_filter_bench.json')) as f:
        k = json.load(f)['K']['128']
    return k['spatial_stage_bytes_per_s'] / k['spatial_stage_fraction_of_measured_hbm']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--iterations', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--shapes', default='128+16,128+64,1008+16,960+64')
    args = ap.parse_args()
    lib = _hip.lib()
    B, it = args.files, args.iterations
    x = synthetic_batch(0, B)
    s = torch.cuda.current_stream().cuda_stream
    hbm = recorded_hbm_rate()
    med = lambda v: float(np.median(v))
    rec = dict(files=B, iterations=it, n_fft=1024, hop=256, repeats=args.repeats, recorded_hbm_bytes_per_s=hbm, shapes={})
    for shape in args.shapes.split(','):
        Kf, n = (int(v) for v in shape.split('+'))
        K = Kf + n
        eng = GCCNMFEngine(x.shape[-1], batch=B, dictionarySize=K, numIterations=it)
        eng.upload(x)
        eng.stft()
        g = eng.g
        V = eng.V
        W0 = eng.W0.unsqueeze(0).expand(B, -1, -1).contiguous()
        H0 = eng.H0.unsqueeze(0).expand(B, -1, -1).contiguous()
        W, H = torch.empty_like(W0), torch.empty_like(H0)
        Wone = eng.W0.clone()
        ws = torch.zeros(lib.gccnmf_klnmf_workspace_floats(g.F, g.N, K, B), device='cuda')
        free = _hip.GCCNMF_FLAG_FREE_ATOMS(n)
        assert lib.gccnmf_klnmf_plan(g.F, g.N, K, B, free) == 32

        def reset():
            W.copy_(W0)
            H.copy_(H0)

        def call(flags, Wp=W):
            _hip.check(lib.gccnmf_klnmf(V.data_ptr(), Wp.data_ptr(), H.data_ptr(), ws.data_ptr(), g.F, g.N, K, B, it, 0.0, 1e-16, flags, s), 'klnmf')

        def stage(stage, flags):
            _hip.check(lib.gccnmf_klnmf_stage(V.data_ptr(), W.data_ptr(), H.data_ptr(), ws.data_ptr(), g.F, g.N, K, B, 0.0, 1e-16, flags, stage, s), 'stage')

        def set_chain(v):
            _hip.check(lib.gccnmf_set_tuning(21, v), 'gccnmf_set_tuning')

        def blind_plain():
            set_chain(0)
            try:
                call(0)
            finally:
                set_chain(1)

        runs = dict(semi=lambda: call(free), blind_plain=blind_plain, blind_default=lambda: call(0), fixed=lambda: call(FIXED_W, Wone))
        t = {k: [] for k in runs}
        for f in runs.values():
            reset()
            f()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for k, f in runs.items():
                t[k] += timed(f, 1, before=reset)

        # stages 4 + 5 on the same R and H: stages 0-3 with the bits leave a materialised R (the blind plain forms do as well at these shapes)
        def prepare(flags):
            reset()
            for st in (0, 1, 2, 3):
                stage(st, flags)
        st = dict(semi_45=[], blind_45=[], semi_4=[])
        set_chain(0)
        try:
            for _ in range(args.repeats + 1):
                prepare(free)
                st['semi_4'] += timed(lambda: stage(4, free), 1)
                prepare(free)
                st['semi_45'] += timed(lambda: (stage(4, free), stage(5, free)), 1)
                prepare(free)           # (the same R and H; the blind stages read them where the semi-supervised stages 0-3 left them)
                st['blind_45'] += timed(lambda: (stage(4, 0), stage(5, 0)), 1)
        finally:
            set_chain(1)
        st = {k: v[1:] for k, v in st.items()}          # the first round is the warm-up
        r_bytes = 4.0 * B * g.F * g.N
        per_it = {k: med(v) / it for k, v in t.items()}
        rec['shapes'][shape] = dict(
            K_fixed=Kf, free_atoms=n, K=K, F=g.F, N=g.N, blind_default_plan=lib.gccnmf_klnmf_plan(g.F, g.N, K, B, 0),
            semi_ms_per_iteration=per_it['semi'], blind_plain_ms_per_iteration=per_it['blind_plain'],
            blind_default_ms_per_iteration=per_it['blind_default'], fixed_ms_per_iteration=per_it['fixed'],
            semi_over_blind_plain=per_it['semi'] / per_it['blind_plain'], semi_over_blind_default=per_it['semi'] / per_it['blind_default'],
            semi_over_fixed=per_it['semi'] / per_it['fixed'],
            spread_ms={k: [min(v), max(v)] for k, v in t.items()},
            stage45_semi_us=1e3 * med(st['semi_45']), stage45_blind_us=1e3 * med(st['blind_45']),
            stage45_semi_over_blind=med(st['semi_45']) / med(st['blind_45']),
            stage4_semi_us=1e3 * med(st['semi_4']), stage4_R_bytes=r_bytes, stage4_bytes_per_s=r_bytes / (med(st['semi_4']) * 1e-3),
            stage4_fraction_of_recorded_hbm=r_bytes / (med(st['semi_4']) * 1e-3) / hbm,
            stage_spread_us={k: [1e3 * min(v), 1e3 * max(v)] for k, v in st.items()})
        print(shape, json.dumps(rec['shapes'][shape]), file=sys.stderr, flush=True)
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(rec, indent=1))


if __name__ == '__main__':
    main()
