"""GCC-NONLIN localisation (gccPHATNLEnabled) beside GCC-PHAT, same process, HIP events after warm-up.

Offline: the angular-spectrogram stage (+ time mean) of 64 synthetic 10 s mixtures and of one file alone, n_fft 1024, hop 256, D = 128,
NL and PHAT alternating.  Streaming: the block time of a StreamingGCCNMFBank (config 5: window 512, hop 64, block 64, K = 1024, D = 64,
two coefficient updates) at 1 and 256 streams with NL on and off.  Prints one JSON record."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gcc_nmf_amd import _hip                                       # noqa: E402
from gcc_nmf_amd.engine import GCCNMFEngine                        # noqa: E402
from gcc_nmf_amd.synthetic import synthetic_batch, synthetic_mixture  # noqa: E402


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


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), n=len(v))


def offline(files, repeats, alpha):
    lib = _hip.lib()
    x = synthetic_batch(0, files)
    eng = GCCNMFEngine(x.shape[-1], batch=files, dictionarySize=64, numIterations=1)
    eng.upload(x)
    eng.stft()
    g, s = eng.g, torch.cuda.current_stream().cuda_stream
    rec = {}
    for B in sorted({files, 1}, reverse=True):
        Dn, Bn = _hip.angular_nl_words(g.D, B, alpha)

        def run(D, batch):
            _hip.check(lib.gccnmf_angular_spectrogram(eng.CC.data_ptr(), eng.trig.data_ptr(), g.F, g.T, D, batch, eng.ang.data_ptr(),
                                                      eng.mean_ang.data_ptr(), s), 'gccnmf_angular_spectrogram')
        for _ in range(3):
            run(Dn, Bn)
            run(g.D, B)
        torch.cuda.synchronize()
        nl, phat = [], []
        for _ in range(repeats):
            nl += timed(lambda: run(Dn, Bn), 1)
            phat += timed(lambda: run(g.D, B), 1)
        evals = float(B) * g.D * g.T * g.F
        rec['files_%d' % B] = dict(nl=stats(nl), phat=stats(phat), evaluations=evals,
                                   nl_evaluations_per_ns=evals / (np.median(nl) * 1e6))
    return rec


def streaming(streams, blocks, alpha):
    from gcc_nmf_amd.realtime import GCCNMFProcessor, StreamingGCCNMFBank, asymmetricWindows
    ws, hop, B, K, D = 512, 64, 64, 1024, 64
    rng = np.random.RandomState(3)
    W = rng.uniform(0.01, 1.0, (ws // 2 + 1, K)).astype(np.float32)
    a, sy = asymmetricWindows(ws, 128)
    x = synthetic_mixture(0, numSamples=(blocks + 20) * B)
    rec = {}
    for S in streams:
        xs = np.repeat(x[None], S, axis=0)
        for nl in (False, True):
            p = GCCNMFProcessor(16000, ws, 1, {'P': {K: W}}, 'P', K, 2, 1.0, True, 6, numTDOAs=D, analysisWindow=a, synthesisWindow=sy,
                                gccPHATNLEnabled=nl, gccPHATNLAlpha=alpha)
            p.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
            bk = StreamingGCCNMFBank(p, S, hop, B, outputDelayBlocks=1)
            for b in range(20):
                bk.process_block(xs[:, :, b * B:(b + 1) * B])
            wall = []
            for b in range(20, 20 + blocks):
                blk = xs[:, :, b * B:(b + 1) * B]
                t0 = time.perf_counter()
                bk.process_block(blk)
                torch.cuda.synchronize()                   # the tracking update (the kernel NL changes) runs behind the hand-out
                wall.append((time.perf_counter() - t0) * 1e3)
            rec['streams_%d_%s' % (S, 'nl' if nl else 'phat')] = dict(p50_ms=float(np.percentile(wall, 50)), p99_ms=float(np.percentile(wall, 99)),
                                                                      blocks=blocks, block_ms=1e3 * B / 16000.0)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--alpha', type=float, default=2.0)
    ap.add_argument('--streams', default='1,256')
    ap.add_argument('--blocks', type=int, default=300)
    args = ap.parse_args()
    rec = dict(alpha=args.alpha, n_fft=1024, hop=256, D=128, offline=offline(args.files, args.repeats, args.alpha),
               streaming=streaming([int(s) for s in args.streams.split(',')], args.blocks, args.alpha))
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
