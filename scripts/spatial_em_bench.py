"""The reconstruct() stage alone with EM iterations behind the spatial mode (``spatialIterations``, csrc/spatial_em.hip).

64 synthetic 10 s mixtures, n_fft 1024, hop 256, S = 3, K = 128 and K = 1024; n in {0, 1, 2, 5, 10, 20}, alternated in one process.  The
factors, the arg-max image and X come from a short run of the pipeline itself (--iterations KL-NMF iterations: the stage's time does
not depend on their values); HIP events time each call after warm-up; median of --repeats with the range.

``--parent-lib <path>``: a library built from the parent commit.  The measurement then runs in child processes, one library each
(GCCNMF_HIP_LIB=<path> selects it), alternated --rounds times in the same session: this library, the parent's, this library, ...  The
parent's library has no iteration bits, so its children time the ratio and the spatial mode only; n = 0 here against its spatial mode is
the comparison, and the SHA-256 of spec must be equal.

Reported per K: the medians, the cost per iteration (the slope between n = 10 and n = 20, and (n = 20 - n = 0) / 20), the bytes an
iteration must move -- X read once, the S powers read and written: (16 + 8 S) Fp Tp per file -- against the measured HBM copy rate, and an
estimate of its float32 operations (each product or sum one operation: -ffp-contract=off, nothing packed) against the plain VALU issue
rate of 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz.  Writes one JSON record (default profiles/r17a_spatial_em_bench.json) and prints it."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)

HBM_MEASURED = 6.29e12        # bytes/s, float4 copy on an MI355X (8.0e12 is the data sheet's figure)
VALU_PLAIN = 256 * 4 * 16 * 2.4e9     # one float32 operation per lane and clock, no fma, nothing packed


def operations_per_frame(S):
    """Float32 products and sums of spatial_em_frame<S> (csrc/spatial.h), counted from the source, a division as one: the 2 x 2 solve,
    then per target u_i, N_i, k_i, v"_i, P_i and the four terms, and the eight float64 conversions and additions of the reduction."""
    solve = (S - 1) + S + 4 + 8 * (S - 1) + 5 + 1 + 28
    per_target = 20 + (4 + 8 * max(S - 2, 0)) + 8 + 7 + 5 + 6 + 13 + 26 + 25 + 8
    return solve + S * per_target


def child(args):
    import torch
    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_batch

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    B, S = args.files, args.targets
    counts = [] if args.child == 'parent' else [int(v) for v in args.counts.split(',')]
    x = synthetic_batch(0, B)
    rec = {}
    for K in [int(k) for k in args.K.split(',')]:
        eng = GCCNMFEngine(x.shape[-1], batch=B, dictionarySize=K, numIterations=args.iterations, numTargets=S)
        eng.upload(x)
        eng.run()
        g = eng.g
        cases = [('ratio', 'ratio', 0)] + ([('spatial', 'spatial', 0)] if args.child == 'parent' else [('n%d' % n, 'spatial', n) for n in counts])

        def run(case):
            eng.reconstruction = case[1]
            if case[2] or hasattr(eng, 'spatialIterations'):
                eng.spatialIterations = case[2]
            eng.reconstruct()

        for c in cases:
            run(c)
        torch.cuda.synchronize()
        t = dict((c[0], []) for c in cases)
        for _ in range(args.repeats):
            for c in cases:
                t[c[0]].append(timed(lambda: run(c)))
        r = dict(F=g.F, T=g.T, Fp=g.Fp, Tp=g.Tp)
        for c in cases:
            r[c[0] + '_ms'] = float(np.median(t[c[0]]))
            r[c[0] + '_range'] = [min(t[c[0]]), max(t[c[0]])]
            run(c)
            torch.cuda.synchronize()
            r[c[0] + '_spec_sha256'] = hashlib.sha256(eng.spec.cpu().numpy().tobytes()).hexdigest()
        rec[str(K)] = r
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(rec))


def summarise(rec, B, S, counts):
    for K, runs in rec['K'].items():
        ours = [r for who, r in runs if who == 'this']
        theirs = [r for who, r in runs if who == 'parent']
        s = dict(F=ours[0]['F'], T=ours[0]['T'], Fp=ours[0]['Fp'], Tp=ours[0]['Tp'])
        for n in counts:
            meds = [r['n%d_ms' % n] for r in ours]
            s['n%d_ms' % n] = float(np.median(meds))
            s['n%d_range' % n] = [min(r['n%d_range' % n][0] for r in ours), max(r['n%d_range' % n][1] for r in ours)]
        s['ratio_ms'] = float(np.median([r['ratio_ms'] for r in ours]))
        if theirs:
            s['parent_spatial_ms'] = float(np.median([r['spatial_ms'] for r in theirs]))
            s['parent_spatial_range'] = [min(r['spatial_range'][0] for r in theirs), max(r['spatial_range'][1] for r in theirs)]
            s['parent_ratio_ms'] = float(np.median([r['ratio_ms'] for r in theirs]))
            s['n0_sha256_equals_parent_spatial'] = len(set([r['n0_spec_sha256'] for r in ours] + [r['spatial_spec_sha256'] for r in theirs])) == 1
        if 10 in counts and 20 in counts and 0 in counts:
            per = (s['n20_ms'] - s['n10_ms']) / 10.0
            s['ms_per_iteration_slope_10_20'] = per
            s['ms_per_iteration_mean_0_20'] = (s['n20_ms'] - s['n0_ms']) / 20.0
            moved = B * (16 + 8 * S) * s['Fp'] * s['Tp']
            ops = B * operations_per_frame(S) * s['F'] * s['T']
            s['iteration_bytes'] = moved
            s['iteration_fraction_of_measured_hbm'] = moved / (per * 1e-3) / HBM_MEASURED
            s['iteration_float32_operations_estimate'] = ops
            s['iteration_fraction_of_plain_valu_issue'] = ops / (per * 1e-3) / VALU_PLAIN
        rec['summary'][K] = s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--targets', type=int, default=3)
    ap.add_argument('--iterations', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--K', default='128,1024')
    ap.add_argument('--counts', default='0,1,2,5,10,20')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r17a_spatial_em_bench.json'))
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    counts = [int(v) for v in args.counts.split(',')]
    rec = dict(files=args.files, targets=args.targets, n_fft=1024, hop=256, repeats=args.repeats, rounds=args.rounds, counts=counts,
               parent_lib=bool(args.parent_lib), K={}, summary={})
    order = (['this', 'parent'] if args.parent_lib else ['this']) * args.rounds
    for who in order:                                          # fresh processes: a process loads one library
        env = dict(os.environ)
        env.pop('GCCNMF_HIP_LIB', None)
        if who == 'parent':
            env['GCCNMF_HIP_LIB'] = os.path.abspath(args.parent_lib)
        cmd = [sys.executable, os.path.abspath(__file__), '--child', who, '--files', str(args.files), '--targets', str(args.targets),
               '--iterations', str(args.iterations), '--repeats', str(args.repeats), '--K', args.K, '--counts', args.counts]
        out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, check=True, timeout=600).stdout.decode()
        got = json.loads(out.strip().splitlines()[-1])
        for K, r in got.items():
            rec['K'].setdefault(K, []).append((who, r))
        print(who, json.dumps(got), file=sys.stderr, flush=True)
    summarise(rec, args.files, args.targets, counts)
    text = json.dumps(rec)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
