"""Time-varying TDOA tracks (GCCNMFEngine(tdoaTracking=True)) beside the static path, HIP events after warm-up.

64 synthetic 10 s mixtures, n_fft 1024, hop 256, D = 128, three targets, K = 128 and 1024: localize() + masks() with tracking (window of
64 frames) and without, alternating in one process, median of --repeats (>= 7); the windowed-mean / per-frame peak stage (the tracks
mode of gccnmf_pick_tdoa_peaks) and the two masks() forms on their own; the SHA-256 of the static path's ``spec``.

One process binds one library, so the comparison against another build of the library (--baseline-lib: the parent commit's
libgccnmf_hip.so) runs the static half of the same measurement in child processes under GCCNMF_HIP_LIB, alternating with this tree's
library: --rounds children each.  The parent process never opens the device.  --bench-steps N also runs the flagship bench.py step under
both libraries, alternating.  Writes one JSON record (default profiles/r10a_tdoa_tracking_bench.json)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)


def timed(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(v):
    import numpy as np
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), n=len(v))


def worker(args):
    """One library, one process: static (and, unless --static-only, tracked) stage times for every K; prints one JSON line."""
    import numpy as np
    import torch
    from gcc_nmf_amd import _hip
    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.synthetic import moving_source_mixture, synthetic_batch
    x = synthetic_batch(0, args.files)
    # a few of the files hold a talker who moves, so that the tracks are not constant everywhere
    for b in range(0, args.files, 8):
        x[b] = moving_source_mixture(b, numSamples=x.shape[-1])
    rec = dict(library='baseline' if os.environ.get('GCCNMF_HIP_LIB') else 'this tree', files=args.files, window_frames=args.window, repeats=args.repeats)
    for K in args.K:
        kw = dict(batch=args.files, dictionarySize=K, numIterations=2)
        engines = {'static': GCCNMFEngine(x.shape[-1], **kw)}
        if not args.static_only:
            engines['tracked'] = GCCNMFEngine(x.shape[-1], tdoaTracking=True, localizationWindowSize=args.window, **kw)
        for e in engines.values():
            e.upload(x)
            e.stft()
            e.klnmf()
        pair = lambda e: (e.localize(), e.masks())
        for _ in range(3):
            for e in engines.values():
                pair(e)
        torch.cuda.synchronize()
        t = dict((name + '_' + what, []) for name in engines for what in ('localize_masks', 'localize', 'masks'))
        if 'tracked' in engines:
            t['windowed_peak_stage'] = []
            e1 = engines['tracked']
            g = e1.g
            word = _hip.peaks_tracks_word(g.S, args.window, g.T)
            s = torch.cuda.current_stream().cuda_stream

            def windowed():
                _hip.check(e1.lib.gccnmf_pick_tdoa_peaks(e1.ang.data_ptr(), g.D, g.T, word, e1.batch, e1.tracks.data_ptr(),
                                                         e1.track_status.data_ptr(), s), 'gccnmf_pick_tdoa_peaks (tracks)')
        for _ in range(args.repeats):                          # alternating: every form once per round
            for name, e in engines.items():
                t[name + '_localize_masks'] += timed(lambda: pair(e), 1)
                t[name + '_localize'] += timed(e.localize, 1)
                t[name + '_masks'] += timed(e.masks, 1)
            if 'tracked' in engines:
                t['windowed_peak_stage'] += timed(windowed, 1)
        r = dict((k, stats(v)) for k, v in t.items())
        e0 = engines['static']
        e0.reconstruct()
        torch.cuda.synchronize()
        r['static_spec_sha256'] = hashlib.sha256(e0.spec.cpu().numpy().tobytes()).hexdigest()
        if 'tracked' in engines:
            g = e1.g
            tr, st = e1.get_tdoa_tracks(), e1.get_track_status()
            r['window_adds'] = float(args.files) * g.D * g.T * min(args.window, g.T)
            r['files_with_moving_tracks'] = int((tr != tr[:, :, :1]).any(axis=(1, 2)).sum())
            r['short_frames'] = int((st != 0).sum())
        rec['K_%d' % K] = r
        del engines
        torch.cuda.empty_cache()
    print('RESULT ' + json.dumps(rec), flush=True)


def child(argv, lib=None, timeout=900):
    env = dict(os.environ)
    env.pop('GCCNMF_HIP_LIB', None)
    if lib:
        env['GCCNMF_HIP_LIB'] = os.path.abspath(lib)
    p = subprocess.run([sys.executable] + argv, env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout,
                       universal_newlines=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-4000:])
        raise SystemExit('child failed with status %d: %s' % (p.returncode, ' '.join(argv)))      # nothing more is started on the device
    return p.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--window', type=int, default=64, help='localizationWindowSize in frames')
    ap.add_argument('--K', type=lambda s: [int(k) for k in s.split(',')], default=[128, 1024])
    ap.add_argument('--baseline-lib', default=None, help="another build of libgccnmf_hip.so (the parent commit's) to measure the static path with")
    ap.add_argument('--rounds', type=int, default=2, help='child processes per library')
    ap.add_argument('--bench-steps', type=int, default=0, help='also run bench.py --gpus 1 --steps N under both libraries')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r10a_tdoa_tracking_bench.json'))
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--static-only', action='store_true')
    args = ap.parse_args()
    if args.repeats < 7:
        raise SystemExit('--repeats must be at least 7')
    if args.worker:
        return worker(args)
    me = [os.path.abspath(__file__), '--worker', '--files', str(args.files), '--repeats', str(args.repeats), '--window', str(args.window),
          '--K', ','.join(str(k) for k in args.K)]
    result = lambda out: json.loads([line for line in out.splitlines() if line.startswith('RESULT ')][-1][7:])
    rec = dict(n_fft=1024, hop=256, D=128, targets=3, seconds=10.0, this_tree=[], baseline=[], bench_this_tree=[], bench_baseline=[])
    for _ in range(args.rounds):                               # alternating: baseline, this tree, baseline, ...
        if args.baseline_lib:
            rec['baseline'].append(result(child(me + ['--static-only'], lib=args.baseline_lib)))
        rec['this_tree'].append(result(child(me)))
    bench = [os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', str(args.bench_steps), '--warmup', '2', '--skip-roofline',
             '--skip-cpu-baseline', '--skip-config-lines', '--skip-extras']                  # the timed flagship steps only

    def last_json(out):
        r = json.loads([line for line in out.splitlines() if line.startswith('{')][-1])
        return dict((k, r[k]) for k in ('metric', 'value', 'unit', 'ms_per_step', 'steps', 'warmup'))
    for _ in range(args.rounds if args.bench_steps else 0):
        if args.baseline_lib:
            rec['bench_baseline'].append(last_json(child(bench, lib=args.baseline_lib, timeout=1500)))
        rec['bench_this_tree'].append(last_json(child(bench, timeout=1500)))
    sha = set(r['K_%d' % K]['static_spec_sha256'] for r in rec['this_tree'] + rec['baseline'] for K in args.K if 'K_%d' % K in r)
    rec['static_spec_identical'] = dict(('K_%d' % K, len(set(r['K_%d' % K]['static_spec_sha256'] for r in rec['this_tree'] + rec['baseline'])) == 1)
                                        for K in args.K)
    rec['distinct_sha256'] = len(sha)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
