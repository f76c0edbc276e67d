"""Multiple mode of the real-time path (TARGET_MODE_MULTIPLE: N talkers separated per stream) against the single-target mode, on the
stream bank at BASELINE config 5 and at the reference's own streaming configuration: per-block host-to-host latency for all S streams
together and the device-resident cost per block, for N = 1, 2, 3, 4 and the single-target window-function mode.  Prints one JSON
record; --out writes it to a file as well.

    python scripts/multi_target_bench.py --out profiles/multi_target_bench.json
    python scripts/multi_target_bench.py --streams 256 --modes 3 --configs config5 --blocks 100 --device-blocks 100   # for a kernel trace
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

WS, HOP, B, D, SR = 512, 64, 64, 64, 16000        # bench.py: streaming_measure


def make_bank(S, K, low_latency, mode):
    """mode 'single' = TARGET_MODE_WINDOW_FUNCTION; an integer N = TARGET_MODE_MULTIPLE with N sources."""
    from gcc_nmf_amd.realtime import GCCNMFProcessor, StreamingGCCNMFBank, asymmetricWindows, TARGET_MODE_MULTIPLE
    rng = np.random.RandomState(0)
    W = rng.rand(WS // 2 + 1, K).astype(np.float32) + 0.02
    W /= np.linalg.norm(W, axis=0)
    N = 2 if mode == 'single' else int(mode)
    if low_latency:        # config 5: asymmetric 512 / 128 windows, 2 H updates per frame, output one block late
        a, sy = asymmetricWindows(WS, 2 * HOP)
        p = GCCNMFProcessor(SR, WS, B // HOP, {'Pretrained': {K: W}}, 'Pretrained', K, 2, 0.1, True, 6, numTDOAs=D,
                            analysisWindow=a, synthesisWindow=sy, numSources=N)
        delay = 1
    else:                  # the reference's own: symmetric sqrt-hamming window, no H updates, delay 2
        p = GCCNMFProcessor(SR, WS, B // HOP, {'Pretrained': {K: W}}, 'Pretrained', K, 0, 0.1, True, 6, numTDOAs=D, numSources=N)
        delay = 2
    p.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
    if mode != 'single':
        p.targetMode = TARGET_MODE_MULTIPLE
    return StreamingGCCNMFBank(p, S, HOP, B, outputDelayBlocks=delay)


def measure(S, K, low_latency, mode, x, n_blocks, warmup, device_blocks):
    import torch
    bk = make_bank(S, K, low_latency, mode)
    for b in range(warmup):
        bk.process_block(x[:, :, b * B:(b + 1) * B])
    lat = []
    for b in range(warmup, warmup + n_blocks):
        t0 = time.perf_counter()
        y = bk.process_block(x[:, :, b * B:(b + 1) * B])
        lat.append(time.perf_counter() - t0)
    lat = np.array(lat) * 1e3
    r = {'mode': mode, 'streams': S, 'p50_ms': float(np.percentile(lat, 50)), 'p99_ms': float(np.percentile(lat, 99)),
         'max_ms': float(lat.max()), 'blocks': int(len(lat)), 'output_shape': list(y.shape), 'output_finite': bool(np.isfinite(y).all()),
         'graph': bk.capture_error is None}
    if device_blocks:
        bk2 = make_bank(S, K, low_latency, mode)
        xs = x[:, :, :device_blocks * B]
        bk2.process_streams(xs[:, :, :4 * B])              # allocation and first launches out of the timing
        bk2 = make_bank(S, K, low_latency, mode)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bk2.process_streams(xs)
        torch.cuda.synchronize()
        r['device_resident_ms_per_block'] = (time.perf_counter() - t0) * 1e3 / device_blocks
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, nargs='+', default=[1, 64, 256])
    ap.add_argument('--modes', nargs='+', default=['single', '1', '2', '3', '4'])
    ap.add_argument('--K', type=int, default=1024)
    ap.add_argument('--blocks', type=int, default=300, help='timed host-to-host blocks per point')
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--device-blocks', type=int, default=150, help='blocks of the device-resident run (0: skip)')
    ap.add_argument('--configs', nargs='+', default=['config5', 'reference'])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from gcc_nmf_amd.synthetic import synthetic_mixture
    torch.cuda.set_device(0)
    n = (a.warmup + max(a.blocks, a.device_blocks)) * B
    signals = {}
    rec = {'metric': 'multiple mode: N talkers per real-time stream, S streams per call, per-block latency host to host', 'unit': 'ms',
           'block_ms': 1e3 * B / SR, 'shape': dict(ws=WS, hop=HOP, B=B, D=D, sr=SR, K=a.K), 'configs': {}}
    for cfg in a.configs:
        rows = []
        for S in a.streams:
            for s in range(len(signals), S):          # each stream its own seeded mixture
                signals[s] = synthetic_mixture(s, numSamples=n, delays=(-3 + s % 5, 1, 4 - s % 3)).astype(np.float32)
            x = np.stack([signals[s] for s in range(S)])
            base = None
            for mode in a.modes:
                r = measure(S, a.K, cfg == 'config5', mode, x, a.blocks, a.warmup, a.device_blocks)
                if mode == 'single':
                    base = r
                elif base is not None and 'device_resident_ms_per_block' in r:
                    r['device_vs_single'] = r['device_resident_ms_per_block'] / base['device_resident_ms_per_block']
                rows.append(r)
                print(json.dumps(dict(config=cfg, **r)), file=sys.stderr, flush=True)
        rec['configs'][cfg] = {'points': rows}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
