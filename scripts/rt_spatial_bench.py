"""What the online spatial filter of the real-time path costs per block (csrc/rt_spatial.hip: one more launch between the mask and the
synthesis kernel), at BASELINE config 5 (window 512, hop = block = 64, K = 1024, 64 TDOAs, asymmetric windows, output one block late).

Grid: one stream (StreamingGCCNMF) and the bank at S = 256; single target and multiple mode with N = 3; numHUpdates 0 and the config's
own 2.  Per point two objects of the same build, filter off and filter on, are fed the same blocks ALTERNATELY in one session, so that
drift of the machine hits both alike: host-to-host time per block (median, minimum, maximum, p99) and the device-resident time per
block (process_block_device in a loop, one synchronisation; off and on alternated, the median of the repeats).  ``--parent-lib`` names a
library built from the parent commit: the same filter-off measurement runs on it in a child process of this session (GCCNMF_HIP_LIB), as
the baseline that does not contain this change at all.  Prints one JSON record; --out writes it to a file as well.

    python scripts/rt_spatial_bench.py --parent-lib /path/to/parent/libgccnmf_hip.so --out profiles/rt_spatial_bench.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

WS, HOP, B, D, SR, K = 512, 64, 64, 64, 16000, 1024
TAU = 16.0


def make(S, targets, nH, spatial):
    from gcc_nmf_amd.realtime import GCCNMFProcessor, StreamingGCCNMF, StreamingGCCNMFBank, asymmetricWindows, TARGET_MODE_MULTIPLE
    rng = np.random.RandomState(0)
    W = rng.rand(WS // 2 + 1, K).astype(np.float32) + 0.02
    W /= np.linalg.norm(W, axis=0)
    a, sy = asymmetricWindows(WS, 2 * HOP)
    kw = dict(spatialFilterEnabled=spatial, spatialFilterFrames=TAU) if spatial else {}
    p = GCCNMFProcessor(SR, WS, B // HOP, {'Pretrained': {K: W}}, 'Pretrained', K, nH, 0.1, True, 6, numTDOAs=D, analysisWindow=a,
                        synthesisWindow=sy, numSources=max(targets, 1), **kw)
    if targets:
        p.targetMode = TARGET_MODE_MULTIPLE
        p.reset()
    p.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
    if S == 1:
        return StreamingGCCNMF(p, HOP, B, outputDelayBlocks=1)
    return StreamingGCCNMFBank(p, S, HOP, B, outputDelayBlocks=1)      # every stream's row starts with the processor's filter setting


def stats(v):
    v = np.asarray(v) * 1e6
    return dict(median_us=float(np.median(v)), min_us=float(v.min()), max_us=float(v.max()), p99_us=float(np.percentile(v, 99)))


def point(S, targets, nH, x, blocks, warmup, device_blocks, repeats, sides):
    """sides: ('off', 'on') for this build, ('off',) for the parent's library."""
    import torch
    objs = {k: make(S, targets, nH, k == 'on') for k in sides}
    xb = x[0] if S == 1 else x[:S]
    lat = {k: [] for k in sides}
    for b in range(warmup + blocks):
        blk = xb[..., b * B:(b + 1) * B]
        for k in sides:                                        # alternated: off, on, off, on, ...
            t0 = time.perf_counter()
            y = objs[k].process_block(blk)
            if b >= warmup:
                lat[k].append(time.perf_counter() - t0)
            assert np.isfinite(y).all()
    r = dict(streams=S, targets=targets or 'single', numHUpdates=nH, blocks=blocks, graph=all(o.capture_error is None for o in objs.values()))
    for k in sides:
        r['host_to_host_' + k] = stats(lat[k])
    dev = {k: [] for k in sides}
    xin = torch.from_numpy(np.ascontiguousarray(xb[..., :B])).cuda()
    outs = {k: torch.zeros_like(objs[k]._outputs()[1]) for k in sides}
    for rep in range(repeats + 1):
        for k in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(device_blocks):
                objs[k].process_block_device(xin, outs[k])
            torch.cuda.synchronize()
            if rep:                                            # the first repeat warms the direct-launch path up
                dev[k].append((time.perf_counter() - t0) / device_blocks)
    for k in sides:
        r['device_resident_' + k] = dict(median_us=float(np.median(dev[k]) * 1e6), min_us=float(min(dev[k]) * 1e6), max_us=float(max(dev[k]) * 1e6))
    if 'on' in sides:
        r['added_us_host_to_host_median'] = r['host_to_host_on']['median_us'] - r['host_to_host_off']['median_us']
        r['added_us_device_resident_median'] = r['device_resident_on']['median_us'] - r['device_resident_off']['median_us']
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, nargs='+', default=[1, 256])
    ap.add_argument('--blocks', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=40)
    ap.add_argument('--device-blocks', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--parent-lib', default=None, help="a library built from the parent commit: its filter-off numbers, in a child process")
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from gcc_nmf_amd.synthetic import synthetic_mixture
    torch.cuda.set_device(0)
    n = (a.warmup + a.blocks) * B
    x = np.stack([synthetic_mixture(s, numSamples=n, delays=(-3 + s % 5, 1, 4 - s % 3)).astype(np.float32) for s in range(max(a.streams))])
    sides = ('off',) if a.child else ('off', 'on')
    rows = []
    for S in a.streams:
        for targets in (0, 3):
            for nH in (0, 2):
                rows.append(point(S, targets, nH, x, a.blocks, a.warmup, a.device_blocks, a.repeats, sides))
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    if a.child:
        print(json.dumps(rows))
        return
    block_us = 1e6 * B / SR
    rec = {'metric': 'online spatial filter: added time per block, filter off / on alternated in one session', 'unit': 'us', 'block_us': block_us,
           'shape': dict(ws=WS, hop=HOP, B=B, D=D, sr=SR, K=K, tau=TAU), 'points': rows}
    if a.parent_lib:
        cmd = [sys.executable, os.path.abspath(__file__), '--child', '--blocks', str(a.blocks), '--warmup', str(a.warmup), '--device-blocks',
               str(a.device_blocks), '--repeats', str(a.repeats), '--streams'] + [str(s) for s in a.streams]
        out = subprocess.run(cmd, env=dict(os.environ, GCCNMF_HIP_LIB=os.path.abspath(a.parent_lib)), stdout=subprocess.PIPE, check=True, timeout=900)
        for r, pr in zip(rows, json.loads(out.stdout.decode().strip().splitlines()[-1])):
            r['parent_library_host_to_host_off'] = pr['host_to_host_off']
            r['parent_library_device_resident_off'] = pr['device_resident_off']
    for r in rows:
        if r['streams'] > 1:
            r['p99_within_block_off'] = r['host_to_host_off']['p99_us'] <= block_us
            r['p99_within_block_on'] = r['host_to_host_on']['p99_us'] <= block_us
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
