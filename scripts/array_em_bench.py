"""Device times of the EM refinement of the M x M spatial filter of the microphone-array engine (gcc_nmf_amd/array.py,
reconstruction='spatial', spatialIterations=n) beside the two launches it runs between.

--files synthetic 10 s recordings (default 64), n_fft 1024, hop 256, S = 3, K = 128, at M = 4 and M = 8 (the lines of
scripts/array_spatial_bench.py).  Per M one 'spatial' engine, warmed by a run of the whole path (--iterations KL-NMF iterations: the
stage times do not depend on the factors' quality); then, alternated in one process on copies of its ratio estimates, HIP events time
gccnmf_array_spatial (n = 0: the two existing launches) and gccnmf_array_em at n = 1 and n = 1 + --span: the median of --repeats with the
range.  ms per iteration = (t(1 + span) - t(1)) / span; t(1) - t(0) is the first iteration with the launch and the powers' pass.

--zero-only times the n = 0 call alone, and --package-root imports gcc_nmf_amd from another tree: run once on the parent commit and once
on this tree (two processes of the same shape), the two records are set side by side by --parent-record and --zero-only-record (the
time counts as equal when the ranges of the repeats overlap; the SHA-256 of spec must be equal).

Needs a device: there is no CPU path.  Writes one JSON record (default profiles/r26a_array_em_bench.json) and prints it."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
LINE = [[0.0, 0, 0], [0.2, 0, 0], [0.5, 0, 0], [1.0, 0, 0]]
LINE8 = [[0.03 * v, 0, 0] for v in (0.0, 1, 4, 9, 15, 22, 32, 34)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--targets', type=int, default=3)
    ap.add_argument('--K', type=int, default=128)
    ap.add_argument('--iterations', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--span', type=int, default=4)
    ap.add_argument('--channels', default='4,8')
    ap.add_argument('--directions', type=int, default=181)
    ap.add_argument('--zero-only', action='store_true')
    ap.add_argument('--package-root', default=REPO)
    ap.add_argument('--parent-record', default=None)
    ap.add_argument('--zero-only-record', default=None)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r26a_array_em_bench.json'))
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)

    import torch
    import gcc_nmf_amd
    assert os.path.samefile(os.path.dirname(gcc_nmf_amd.__file__), os.path.join(args.package_root, 'gcc_nmf_amd')), 'the package of --package-root'
    from gcc_nmf_amd import _array, _array_spatial
    from gcc_nmf_amd.array import GCCNMFArrayEngine, azimuthDirections
    from gcc_nmf_amd.synthetic import array_mixture
    if not args.zero_only:
        from gcc_nmf_amd import _array_em

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def stats(r, key, v):
        r[key + '_ms'] = float(np.median(v))
        r[key + '_range'] = [float(min(v)), float(max(v))]

    B, S, K = args.files, args.targets, args.K
    n = int(round(args.seconds * 16000))
    rec = dict(files=B, seconds=args.seconds, targets=S, K=K, iterations=args.iterations, n_fft=1024, hop=256, directions=args.directions,
               repeats=args.repeats, span=args.span, zero_only=bool(args.zero_only), M={})
    parent = json.load(open(args.parent_record)) if args.parent_record else None
    alone = json.load(open(args.zero_only_record)) if args.zero_only_record else None
    for M in [int(m) for m in args.channels.split(',')]:
        line = np.array(LINE if M <= 4 else LINE8)[:M]
        distinct = [array_mixture(i, line, [40, 90, 130], n, 16000) for i in range(4)]      # the stage times do not depend on the samples
        x = np.stack([distinct[i % 4] for i in range(B)])
        e = GCCNMFArrayEngine(n, numChannels=M, microphonePositions=line, directions=azimuthDirections(args.directions), numTargets=S,
                              dictionarySize=K, numIterations=args.iterations, batch=B, reconstruction='spatial')
        e.upload(x)
        e.run()                                                # warm-up, and the n = 0 spec of the engine
        torch.cuda.synchronize()
        r = dict(F=e.F, T=e.T, Fp=e.Fp, Tp=e.Tp, nsig_pitch=e.nsig_pitch)
        r['zero_spec_sha256'] = hashlib.sha256(e.spec.cpu().numpy().tobytes()).hexdigest()
        ratio = torch.zeros_like(e.spec)
        _array.reconstruct(e.W, e.H, e.argmax, None, e.X, M, e.F, e.T, K, S, B, e.nsig_pitch, ratio)
        scratch, cov = torch.empty_like(ratio), torch.empty_like(e.cov)
        calls = {0: lambda: _array_spatial.spatial(e.X, M, e.F, e.T, S, B, e.nsig_pitch, cov, scratch)}
        if not args.zero_only:
            ws = torch.zeros(_array_em.workspace_floats(M, e.F, e.T, S, B), dtype=torch.float32, device=e.device)
            for m in (1, 1 + args.span):
                calls[m] = (lambda m: lambda: _array_em.em(e.X, M, e.F, e.T, S, B, e.nsig_pitch, m, ws, scratch))(m)
        t = dict((m, []) for m in calls)
        for rep in range(args.repeats + 1):                    # (the first round warms every launch and is dropped)
            for m in sorted(calls):
                scratch.copy_(ratio)
                v = timed(calls[m])
                if rep:
                    t[m].append(v)
        for m in sorted(calls):
            stats(r, 'n%d_call' % m, t[m])
        if not args.zero_only:
            hi = 1 + args.span
            r['ms_per_iteration'] = (r['n%d_call_ms' % hi] - r['n1_call_ms']) / args.span
            r['first_iteration_ms'] = r['n1_call_ms'] - r['n0_call_ms']
            r['frames_per_s_per_iteration'] = B * e.F * e.T / (r['ms_per_iteration'] * 1e-3)
        if parent is not None and str(M) in parent['M']:
            p, own = parent['M'][str(M)], (alone['M'][str(M)] if alone is not None else r)
            r['parent_n0_call_ms'], r['parent_n0_call_range'] = p['n0_call_ms'], p['n0_call_range']
            r['alone_n0_call_ms'], r['alone_n0_call_range'] = own['n0_call_ms'], own['n0_call_range']
            r['zero_spec_equals_parent'] = p['zero_spec_sha256'] == r['zero_spec_sha256'] == own['zero_spec_sha256']
            lo, hi = own['n0_call_range']
            plo, phi = p['n0_call_range']
            r['n0_time_within_spread_of_parent'] = bool(lo <= phi and plo <= hi)
        rec['M'][str(M)] = r
        print(M, json.dumps(r), file=sys.stderr, flush=True)
        del e, ratio, scratch, cov
        torch.cuda.empty_cache()
    text = json.dumps(rec)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
