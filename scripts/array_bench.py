"""Per-stage device times of the M-channel engine (gcc_nmf_amd/array.py) beside the stereo engine in ratio mode.

64 synthetic 10 s recordings, n_fft 1024, hop 256, S = 3, 100 KL-NMF iterations, K = 128 and K = 1024: GCCNMFArrayEngine at M = 4 (the
4-microphone line of tests/test_array_host.py, 181 azimuths) and GCCNMFEngine(reconstruction='ratio') at the same file count and
length, alternated stage by stage in one process.  HIP events time each stage call after a warm-up run of the whole path; the median
of --repeats with the range.  'stft' of the array engine is the STFT of all signals plus gccnmf_array_features ('features' times that
call alone); 'masks' includes the copy of W under every pair's rows.  Recorded, not asserted.

Also recorded, from the shapes: the multiply-accumulates of the stacked score GEMM, P K F S T per file, against the 4 F K (M T) per
KL-NMF iteration (400 F K M T for 100) -- the score GEMM does P times the work of a pair-summing steering kernel.

Needs a device: there is no CPU path.  Writes one JSON record (default profiles/r23a_array_bench.json) and prints it."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)

LINE = [[0.0, 0, 0], [0.2, 0, 0], [0.5, 0, 0], [1.0, 0, 0]]
STAGES = ('stft', 'klnmf', 'localize', 'masks', 'reconstruct', 'istft')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--targets', type=int, default=3)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--K', default='128,1024')
    ap.add_argument('--directions', type=int, default=181)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r23a_array_bench.json'))
    args = ap.parse_args()

    import torch
    from gcc_nmf_amd import _array
    from gcc_nmf_amd.array import GCCNMFArrayEngine, azimuthDirections
    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.synthetic import array_mixture, synthetic_batch

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    B, S, M = args.files, args.targets, len(LINE)
    n = int(round(args.seconds * 16000))
    azimuths = [40, 90, 130, 65, 110, 20, 150, 75][:max(S, 2)]
    # a few distinct recordings repeated: the stage times do not depend on the samples
    distinct = [array_mixture(i, np.array(LINE), azimuths, n, 16000) for i in range(4)]
    xa = np.stack([distinct[i % 4] for i in range(B)])
    xs = synthetic_batch(0, 4, numSamples=n)
    xs = np.stack([xs[i % 4] for i in range(B)])
    rec = dict(files=B, seconds=args.seconds, channels=M, pairs=_array.num_pairs(M), targets=S, iterations=args.iterations, n_fft=1024,
               hop=256, directions=args.directions, repeats=args.repeats, K={})
    for K in [int(k) for k in args.K.split(',')]:
        arr = GCCNMFArrayEngine(n, numChannels=M, microphonePositions=LINE, directions=azimuthDirections(args.directions), numTargets=S,
                                dictionarySize=K, numIterations=args.iterations, batch=B)
        ste = GCCNMFEngine(n, numTDOAs=128, numTargets=S, dictionarySize=K, numIterations=args.iterations, batch=B, reconstruction='ratio')
        arr.upload(xa)
        ste.upload(xs)
        for e in (arr, ste):                                   # warm-up: every shape the timed window uses
            e.run()
        torch.cuda.synchronize()
        arr.check_status()
        ste.check_status()
        t = dict(((who, s), []) for who in ('array', 'stereo') for s in STAGES + ('total',))
        t[('array', 'features')] = []
        for _ in range(args.repeats):
            for who, e in (('array', arr), ('stereo', ste)):
                total = 0.0
                for s in STAGES:
                    ms = timed(getattr(e, s))
                    t[(who, s)].append(ms)
                    total += ms
                t[(who, 'total')].append(total)
            t[('array', 'features')].append(timed(lambda: _array.features(arr.X, M, arr.F, arr.T, B, arr.V, arr.CC)))
        F, T, P = arr.F, arr.T, arr.P
        r = dict(F=F, T=T, Fs=arr.Fs, N_array=arr.N, N_stereo=ste.g.N, stereo_nmf_groups=ste.nmf_groups,
                 score_gemm_macs_per_file=P * K * F * S * T, klnmf_macs_per_file=4 * args.iterations * F * K * M * T,
                 array_indexes_file0=arr.get_tdoa_indexes()[0].tolist())
        r['score_gemm_share_of_klnmf_macs'] = r['score_gemm_macs_per_file'] / float(r['klnmf_macs_per_file'])
        for (who, s), v in sorted(t.items()):
            r['%s_%s_ms' % (who, s)] = float(np.median(v))
            r['%s_%s_range' % (who, s)] = [float(min(v)), float(max(v))]
        r['array_frames_per_second'] = B * T / (r['array_total_ms'] * 1e-3)
        r['stereo_frames_per_second'] = B * ste.g.T / (r['stereo_total_ms'] * 1e-3)
        rec['K'][str(K)] = r
        print(K, json.dumps(r), file=sys.stderr, flush=True)
        del arr, ste
        torch.cuda.empty_cache()
    text = json.dumps(rec)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
