"""numSources='auto'  beside the fixed count, HIP events after warm-up, median of --repeats (>= 20).

Count launch: the count mode of gccnmf_pick_tdoa_peaks next to the fixed-count launch at S = 3 on the same 64 mean angular spectra, at
D = 128 and D = 1024 (spectra with a dozen peaks each over a noise floor of small ones, as a mean angular spectrum has).

Whole step: GCCNMFEngine.run() on 64 synthetic 10 s mixtures, n_fft 1024, hop 256, D = 128, at K = 128 and K = 1024, with numTargets=3
beside numTargets='auto' at maxTargets 3, 4 and 8, the engines taking turns within every round.  The difference at maxTargets = 3 is the
price of the mode; the differences at 4 and 8 are the price of carrying slots that stay empty (every file holds three talkers).

Writes one JSON record (default profiles/r15a_source_count_bench.json)."""
import argparse
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    import numpy as np
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), n=len(v))


def count_launch(args, D):
    import numpy as np
    import torch
    from gcc_nmf_amd import _hip
    rng = np.random.RandomState(D)
    B, Dp = args.files, -(-D // 64) * 64
    m = np.zeros((B, Dp))
    m[:, :D] = 1e-3 * rng.standard_normal((B, D))
    for b in range(B):
        m[b, rng.choice(np.arange(1, D - 1, 2), 12, replace=False)] += rng.uniform(0.2, 1.0, 12)
    dm = torch.from_numpy(m).cuda()
    fixed_idx = torch.zeros((B, 3), dtype=torch.int32, device='cuda')
    auto_idx = torch.zeros((B, 8), dtype=torch.int32, device='cuda')
    st = torch.zeros((B,), dtype=torch.int32, device='cuda')
    forms = {'fixed_S3': lambda: _hip.pick_tdoa_peaks(dm, D, Dp, 3, B, fixed_idx, st),
             'count_max8': lambda: _hip.count_tdoa_peaks(dm, D, Dp, 8, B, auto_idx, st)}
    for _ in range(5):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    t = dict((name, []) for name in forms)
    for _ in range(args.repeats):
        for name, fn in forms.items():
            t[name].append(timed(fn))
    rec = dict((name, stats(v)) for name, v in t.items())
    rec['peaks_per_file'] = float(np.mean([((m[b, 1:D - 1] > m[b, :D - 2]) & (m[b, 1:D - 1] > m[b, 2:D])).sum() for b in range(B)]))
    rec['counts'] = np.bincount((auto_idx.cpu().numpy() >= 0).sum(axis=1), minlength=9).tolist()
    return rec


def whole_step(args, K):
    import torch
    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_batch
    x = synthetic_batch(0, args.files)
    kw = dict(batch=args.files, dictionarySize=K)
    engines = {'numTargets_3': GCCNMFEngine(x.shape[-1], numTargets=3, **kw)}
    for m in (3, 4, 8):
        engines['auto_max%d' % m] = GCCNMFEngine(x.shape[-1], numTargets='auto', maxTargets=m, **kw)
    for e in engines.values():
        e.upload(x)
        for _ in range(2):
            e.run()
    torch.cuda.synchronize()
    t = dict((name, []) for name in engines)
    for _ in range(args.repeats):                              # taking turns: every engine once per round
        for name, e in engines.items():
            t[name].append(timed(e.run))
    rec = dict((name, stats(v)) for name, v in t.items())
    rec['counts'] = dict((name, e.get_num_sources().tolist()) for name, e in engines.items())
    for e in engines.values():
        e.check_status()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=21)
    ap.add_argument('--K', type=lambda s: [int(k) for k in s.split(',') if k], default=[128, 1024])
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r15a_source_count_bench.json'))
    args = ap.parse_args()
    if args.repeats < 20:
        raise SystemExit('--repeats must be at least 20')
    import torch
    rec = dict(files=args.files, n_fft=1024, hop=256, seconds=10.0, repeats=args.repeats, device=torch.cuda.get_device_name(0))
    for D in (128, 1024):
        rec['count_launch_D%d' % D] = count_launch(args, D)
    for K in args.K:
        rec['run_K%d' % K] = whole_step(args, K)
        torch.cuda.empty_cache()
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
