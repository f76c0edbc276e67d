"""Offline speech enhancement at batch scale: the full-grid atom TDOA arg-max stage (csrc/atom_tdoa.hip) and the whole engine step.

64 synthetic 10 s mixtures, n_fft 1024, hop 256, 128 TDOAs, K = 128 and K = 1024 (``--atoms``), HIP events after a warm-up:
  the atom-TDOA launch alone, its rate 2 K F D T batch / time as a fraction of the f32 MFMA peak (157.3 TFLOP/s), and the floor that
  peak sets (34 ms at K = 1024, 4.3 ms at K = 128); the masks launch; the whole GCCNMFEnhancementEngine step (STFT ... inverse STFT on
  resident samples) next to the GCCNMFEngine separation step (three targets: what the code before this stage could do) at the same
  shape, alternating in one process.
Prints one JSON record (profiles/r14a_enhancement_bench.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
from gcc_nmf_amd import _hip                                           # noqa: E402
from gcc_nmf_amd.engine import GCCNMFEngine, GCCNMFEnhancementEngine   # noqa: E402
from gcc_nmf_amd.synthetic import synthetic_batch                      # noqa: E402

F32_MFMA_PEAK = 157.3e12


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
    ap.add_argument('--atoms', default='128,1024')
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--stage-only', action='store_true', help='skip the two whole-engine steps')
    args = ap.parse_args()
    B = args.files
    x = synthetic_batch(0, B)
    med = lambda v: float(np.median(v))
    rec = dict(files=B, seconds_per_file=10, n_fft=1024, hop=256, numTDOAs=128, iterations=args.iterations, repeats=args.repeats,
               f32_mfma_peak_flops=F32_MFMA_PEAK, K={})
    for K in [int(v) for v in args.atoms.split(',')]:
        enh = GCCNMFEnhancementEngine(x.shape[-1], batch=B, dictionarySize=K, numIterations=args.iterations, targetTDOAEpsilon=4.0)
        enh.upload(x)
        enh.run()
        torch.cuda.synchronize()
        enh.check_status()
        g = enh.g
        flops = 2.0 * K * g.F * g.D * g.T * B
        stage = timed(enh.masks, args.repeats + 1)[1:]
        atom = timed(lambda: _hip.atom_tdoa_indexes(enh.CC, enh.trig, enh.W, g.F, g.T, g.K, g.D, B, enh.atom_tdoa), args.repeats + 1)[1:]
        r = dict(F=g.F, T=g.T, D=g.D, flops=flops, atom_tdoa_ms=med(atom), atom_tdoa_spread_ms=[min(atom), max(atom)],
                 atom_tdoa_fraction_of_f32_mfma_peak=flops / (med(atom) * 1e-3) / F32_MFMA_PEAK, floor_ms_at_peak=1e3 * flops / F32_MFMA_PEAK,
                 masks_stage_ms=med(stage), hbm_bytes_written=2.0 * B * g.Kp * g.Tp)
        if not args.stage_only:
            sep = GCCNMFEngine(x.shape[-1], batch=B, dictionarySize=K, numIterations=args.iterations)
            sep.upload(x)
            sep.run()
            torch.cuda.synchronize()
            t = dict(enhancement=[], separation=[])
            for _ in range(args.repeats):
                t['enhancement'] += timed(enh.run, 1)
                t['separation'] += timed(sep.run, 1)
            sep_masks = timed(sep.masks, args.repeats + 1)[1:]
            r.update(enhancement_step_ms=med(t['enhancement']), separation_step_ms=med(t['separation']),
                     enhancement_over_separation=med(t['enhancement']) / med(t['separation']),
                     step_spread_ms={k: [min(v), max(v)] for k, v in t.items()}, separation_masks_stage_ms=med(sep_masks),
                     atom_tdoa_fraction_of_step=med(atom) / med(t['enhancement']))
            del sep
        rec['K'][str(K)] = r
        print(K, json.dumps(r), file=sys.stderr, flush=True)
        del enh
        torch.cuda.empty_cache()
    print(json.dumps(rec, indent=1))


if __name__ == '__main__':
    main()
