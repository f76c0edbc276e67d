"""Device times of the M x M spatial filter of the microphone-array engine (gcc_nmf_amd/array.py, reconstruction='spatial'; DESIGN
section 4j) beside the ratio mask it runs behind.

--files synthetic 10 s recordings (default 64), n_fft 1024, hop 256, S = 3, K = 128, 100 KL-NMF iterations, at M = 4 (the line of
tests/test_array_host.py) and M = 8 (the line of tests/stacked_pairs.py).  Per M one 'ratio' and one 'spatial' engine on the same
samples, warmed by a run of the whole path, then alternated in one process: HIP events time reconstruct() of each engine and the
gccnmf_array_spatial call alone (on a copy of the ratio estimates), the median of --repeats with the range.  The call is two launches;
events cannot come between them, so their split comes from a rocprofv3 --kernel-trace --stats run of this script (a run of its own):
--kernel-stats <its *_kernel_stats.csv> --into <record> adds the two kernels' average times to a record, without a device.

Bytes the two launches must move, from the shapes: the covariance launch reads S M planes, the filter reads S M + M and writes S M
(2 S M + M), a plane = Fp Tp complex64 per file.  The rate over those bytes stands beside the HBM copy rate measured in the same
process (a 1 GiB device-to-device copy, read + write).  Recorded, not asserted.

Also recorded: the time of 'ratio' reconstruct() and the SHA-256 of its spec.  --ratio-only builds the engine WITHOUT the keyword and
times it alone, and --package-root imports gcc_nmf_amd from another tree: run once on the parent commit and once on this tree (two
processes of the same shape; beside a 'spatial' engine the ratio launch finds other data in the caches), the two records are set side
by side by --parent-record and --ratio-only-record (the time counts as equal when the ranges of the repeats overlap).

Needs a device: there is no CPU path.  Writes one JSON record (default profiles/r25a_array_spatial_bench.json) and prints it."""
import argparse
import csv
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
LINE = [[0.0, 0, 0], [0.2, 0, 0], [0.5, 0, 0], [1.0, 0, 0]]
LINE8 = [[0.03 * v, 0, 0] for v in (0.0, 1, 4, 9, 15, 22, 32, 34)]


def merge_kernel_stats(stats, into):
    """The two kernels' rows of a rocprofv3 kernel-stats CSV -> average times and rates in the record (no device needed)."""
    rec = json.load(open(into))
    rows = list(csv.DictReader(open(stats)))
    for M, r in rec['M'].items():
        for kind, moved in (('cov', r['cov_bytes']), ('filter', r['filter_bytes'])):
            hit = [x for x in rows if 'array_spatial_%s_kernel<%s' % (kind, M) in x['Name']]
            if not hit:
                continue
            ns = float(hit[0]['AverageNs'])
            r['%s_kernel_ms' % kind] = ns * 1e-6
            r['%s_kernel_calls' % kind] = int(hit[0]['Calls'])
            r['%s_kernel_bytes_per_s' % kind] = moved / (ns * 1e-9)
            r['%s_kernel_fraction_of_measured_copy' % kind] = r['%s_kernel_bytes_per_s' % kind] / rec['hbm_copy_bytes_per_s']
    with open(into, 'w') as f:
        f.write(json.dumps(rec) + '\n')
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--targets', type=int, default=3)
    ap.add_argument('--K', type=int, default=128)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--channels', default='4,8')
    ap.add_argument('--directions', type=int, default=181)
    ap.add_argument('--ratio-only', action='store_true')
    ap.add_argument('--package-root', default=REPO)
    ap.add_argument('--parent-record', default=None)
    ap.add_argument('--ratio-only-record', default=None)
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--into', default=None)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r25a_array_spatial_bench.json'))
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.kernel_stats, args.into or args.out)
    sys.path.insert(0, args.package_root)

    import torch
    from gcc_nmf_amd.array import GCCNMFArrayEngine, azimuthDirections
    from gcc_nmf_amd.synthetic import array_mixture

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
               repeats=args.repeats, ratio_only=bool(args.ratio_only), M={})
    # the copy rate of this session: 1 GiB device to device, read + write
    src = torch.empty(1 << 28, dtype=torch.float32, device='cuda')
    dst = torch.empty_like(src)
    src.fill_(1.0)
    dst.copy_(src)
    copies = [timed(lambda: dst.copy_(src)) for _ in range(args.repeats)]
    rec['hbm_copy_bytes_per_s'] = 2.0 * src.numel() * 4 / (float(np.median(copies)) * 1e-3)
    rec['hbm_copy_ms_range'] = [float(min(copies)), float(max(copies))]
    del src, dst
    torch.cuda.empty_cache()
    parent = json.load(open(args.parent_record)) if args.parent_record else None
    alone = json.load(open(args.ratio_only_record)) if args.ratio_only_record else None
    for M in [int(m) for m in args.channels.split(',')]:
        line = np.array(LINE if M <= 4 else LINE8)[:M]
        distinct = [array_mixture(i, line, [40, 90, 130], n, 16000) for i in range(4)]      # the stage times do not depend on the samples
        x = np.stack([distinct[i % 4] for i in range(B)])
        kw = dict(numChannels=M, microphonePositions=line, directions=azimuthDirections(args.directions), numTargets=S, dictionarySize=K,
                  numIterations=args.iterations, batch=B)
        modes = ['ratio'] if args.ratio_only else ['ratio', 'spatial']
        eng = dict((m, GCCNMFArrayEngine(n, **(kw if args.ratio_only else dict(kw, reconstruction=m)))) for m in modes)
        for e in eng.values():                                 # warm-up: every shape the timed window uses
            e.upload(x)
            e.run()
        torch.cuda.synchronize()
        e0 = eng['ratio']
        r = dict(F=e0.F, T=e0.T, Fp=e0.Fp, Tp=e0.Tp, nsig_pitch=e0.nsig_pitch, indexes_file0=e0.get_tdoa_indexes()[0].tolist())
        try:
            for e in eng.values():
                e.check_status()
        except ValueError as err:                              # fewer peaks than talkers in a file: its spec is still computed and timed
            r['status'] = str(err)
        plane = e0.Fp * e0.Tp * 8
        r['cov_bytes'], r['filter_bytes'] = B * S * M * plane, B * (2 * S * M + M) * plane
        t = dict((m, []) for m in modes)
        call = []
        if not args.ratio_only:
            from gcc_nmf_amd import _array_spatial
            sp = eng['spatial']
            scratch, cov = torch.empty_like(e0.spec), torch.empty_like(sp.cov)
        for _ in range(args.repeats):
            for m in modes:
                t[m].append(timed(eng[m].reconstruct))
            if not args.ratio_only:
                scratch.copy_(e0.spec)
                call.append(timed(lambda: _array_spatial.spatial(sp.X, M, sp.F, sp.T, S, B, sp.nsig_pitch, cov, scratch)))
        for m in modes:
            stats(r, m + '_reconstruct', t[m])
            r[m + '_spec_sha256'] = hashlib.sha256(eng[m].spec.cpu().numpy().tobytes()).hexdigest()
        if not args.ratio_only:
            stats(r, 'spatial_call', call)
            moved = r['cov_bytes'] + r['filter_bytes']
            r['spatial_call_bytes'] = moved
            r['spatial_call_bytes_per_s'] = moved / (r['spatial_call_ms'] * 1e-3)
            r['spatial_call_fraction_of_measured_copy'] = r['spatial_call_bytes_per_s'] / rec['hbm_copy_bytes_per_s']
            r['spatial_over_ratio'] = r['spatial_reconstruct_ms'] / r['ratio_reconstruct_ms']
            assert torch.equal(scratch.view(torch.int32), sp.spec.view(torch.int32)), 'the timed call computes what the engine computes'
        if parent is not None and str(M) in parent['M']:
            p, own = parent['M'][str(M)], (alone['M'][str(M)] if alone is not None else r)
            r['parent_ratio_reconstruct_ms'], r['parent_ratio_reconstruct_range'] = p['ratio_reconstruct_ms'], p['ratio_reconstruct_range']
            r['parent_ratio_spec_sha256'] = p['ratio_spec_sha256']
            r['alone_ratio_reconstruct_ms'], r['alone_ratio_reconstruct_range'] = own['ratio_reconstruct_ms'], own['ratio_reconstruct_range']
            r['ratio_spec_equals_parent'] = p['ratio_spec_sha256'] == r['ratio_spec_sha256'] == own['ratio_spec_sha256']
            lo, hi = own['ratio_reconstruct_range']
            plo, phi = p['ratio_reconstruct_range']
            r['ratio_time_within_spread_of_parent'] = bool(lo <= phi and plo <= hi)
        rec['M'][str(M)] = r
        print(M, json.dumps(r), file=sys.stderr, flush=True)
        del eng, e0
        if not args.ratio_only:
            del sp, scratch, cov
        torch.cuda.empty_cache()
    text = json.dumps(rec)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
