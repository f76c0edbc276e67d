#!/usr/bin/env python
"""Headline benchmark: stereo STFT frames/s through the whole GCC-NMF hot path on MI355X.

    python bench.py --gpus 1 --steps 5 --warmup 1
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json metric, config 2 parameters on config 3's batch): every rank owns `--files`
(default 64) synthetic 10 s stereo mixtures @16 kHz (SURVEY.md 8d recipe), 1024-pt FFT, hop 256,
K = 1024 atoms, 100 KL-NMF iterations, 128 TDOAs, 3 targets.  One step = one pass of the hot path over
the rank's batch: samples already resident in HBM -> STFT -> KL-NMF -> GCC-PHAT localisation ->
GCC-NMF masks -> reconstruction -> iSTFT/OLA -> separated waveforms in HBM.  Files are independent,
so ranks share nothing on the data path (weak scaling, no collective inside the timed region).

Prints ONE JSON line (rank 0).  `value` is the bench contract's rate (inputs resident in HBM when the timed region starts).
A plain run only sets up, warms up, times the steps and prints that line.  With `--full` the line also carries everything else
the benchmark measures: `sec8d_host_to_host` is SURVEY 8(d)'s metric (host samples in -> host waveforms out, 8 batches pipelined);
`roofline` times the dominant kernel live with HIP events on the launch stream; `cpu_baseline` times the NumPy oracle (a port of
the reference) on one file at the best of a few BLAS thread counts; the other BASELINE configurations are timed in sub-records.
`--dump-outputs DIR` writes what the last timed step computed as .npy files (see dump_outputs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

F32_MFMA_PEAK_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md: dense f32 matrix peak


def parse():
    p = argparse.ArgumentParser()
    p.add_argument('--gpus', type=int, default=1)
    p.add_argument('--steps', type=int, default=5)
    p.add_argument('--warmup', type=int, default=1)
    p.add_argument('--files', type=int, default=64, help='mixture files per GPU per step')
    p.add_argument('--dictionary-size', type=int, default=1024)
    p.add_argument('--iterations', type=int, default=100)
    p.add_argument('--hop', type=int, default=256)
    p.add_argument('--seconds', type=float, default=10.0)
    p.add_argument('--no-xcd-affinity', action='store_true')
    p.add_argument('--nmf-groups', type=int, default=None,
                   help='KL-NMF file groups on separate streams (engine default: 2 from 32 files up); 1 = one launch per stage over the '
                        'whole batch, the configuration the roofline kernel is timed in')
    p.add_argument('--skip-roofline', action='store_true')
    p.add_argument('--skip-cpu-baseline', action='store_true')
    p.add_argument('--skip-config-lines', action='store_true', help='no sub-records of the other BASELINE configurations (K = 128 batch, K sweep, 200 iterations, shared dictionary, streaming, big matrix)')
    p.add_argument('--no-live-traffic', action='store_true', help='roofline.traffic from the recorded passes (profiles/pmc_traffic.json) instead of two child runs under rocprofv3 --pmc')
    p.add_argument('--skip-extras', action='store_true', help='sweeps: only the timed steps and the roofline kernel (no host-to-host, single-file, drop-in, CPU legs)')
    p.add_argument('--tune', action='append', default=[], metavar='KEY=VALUE', help='gccnmf_set_tuning(KEY, VALUE) before running (A/B experiments)')
    p.add_argument('--h-updates', type=int, default=2, help='streaming mode: KL-NMF coefficient updates per frame (W fixed)')
    p.add_argument('--mode', choices=['separate', 'shared-dictionary', 'streaming', 'time-sharded'], default='separate',
                   help="'separate' = the headline path (independent dictionary per file); 'shared-dictionary' = BASELINE config 4; 'streaming' = config 5; 'time-sharded' = ONE long mixture (--seconds, default 160 s there) sharded over frame windows, strong scaling")
    p.add_argument('--full', action='store_true',
                   help='also run every measurement and check beyond the headline figure (roofline kernel, host-to-host, single file, drop-in, '
                        'mixed lengths, the other BASELINE configurations, CPU baseline, live HBM traffic); the --skip-* options prune these')
    p.add_argument('--dump-outputs', metavar='DIR', default=None,
                   help="after the timed steps, write what the last one computed as DIR/<name>.npy ('separate' mode; rank 0's files)")
    a = p.parse_args()
    if a.steps < 1:
        p.error('--steps must be at least 1')
    if a.dump_outputs and a.mode != 'separate':
        p.error("--dump-outputs writes the outputs of the 'separate' mode only")
    return a


DUMP_BUDGET_BYTES = 40 << 20          # the waveform sample of --dump-outputs; with the index files it writes well under 64 MB


def dump_outputs(d, e, seed=0):
    """--dump-outputs: what the timed path handed its caller in the last step -- the separated waveforms `e.y` (files, targets, 2, samples)
    and the TDOA indexes -- as .npy files in `d`, well under 64 MB in all:
      waveforms.npy        float32, the waveforms of the files listed in waveform_files.npy, all of them if they fit in DUMP_BUDGET_BYTES,
                           else a fixed seeded choice of files (and, should one file alone not fit, of sample positions: waveform_samples.npy)
      waveform_files.npy   float64, which files (index in the batch) waveforms.npy holds
      waveform_rms.npy     float64 (files, targets, 2), RMS of every waveform of the batch
      tdoa_indexes.npy     float64 (files, targets), the target TDOA indexes of every file"""
    import torch
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    y = e.y
    B, per_file = y.shape[0], y[0].numel() * y.element_size()
    files = np.arange(B) if B * per_file <= DUMP_BUDGET_BYTES else np.sort(rng.choice(B, max(1, DUMP_BUDGET_BYTES // per_file), replace=False))
    sample = y[torch.from_numpy(files).to(y.device)]
    if per_file > DUMP_BUDGET_BYTES:
        L = y.shape[-1]
        cols = np.sort(rng.choice(L, DUMP_BUDGET_BYTES // (per_file // L), replace=False))
        sample = sample[..., torch.from_numpy(cols).to(y.device)]
        np.save(os.path.join(d, 'waveform_samples.npy'), cols.astype(np.float64))
    np.save(os.path.join(d, 'waveforms.npy'), sample.float().cpu().numpy())
    np.save(os.path.join(d, 'waveform_files.npy'), files.astype(np.float64))
    np.save(os.path.join(d, 'waveform_rms.npy'), y.double().square().mean(dim=-1).sqrt().cpu().numpy())
    np.save(os.path.join(d, 'tdoa_indexes.npy'), e.get_tdoa_indexes().astype(np.float64))


def live_traffic(a, timeout_s=150, chained=False):
    """HBM bytes per launch of the K1 / K3 kernel, measured NOW: two child runs of this file (10 KL-NMF iterations of the same batch on
    one stream, nothing else) under `rocprofv3 --kernel-trace --pmc FETCH_SIZE` and `... --pmc WRITE_SIZE` -- separate passes, the
    counter units and the gfx950 correction of /opt/skills/guides/MI355X_MICROARCH.md's HBM section (KB = 1024 B; FETCH_SIZE reports half
    of the bytes of 16 B/lane coalesced reads, so it is doubled).  Returns (record or None, note).  Never raises: a missing profiler, a
    profiler already wrapped around this process, a child that fails or overruns `timeout_s` leave the recorded figure in place."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    roc = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    if not os.path.exists(roc):
        return None, 'rocprofv3 not found'
    if any(k.startswith(('ROCPROF', 'ROCP_', 'ROCPROFILER')) for k in os.environ) or 'rocprofiler' in os.environ.get('LD_PRELOAD', ''):
        return None, 'this process already runs under a profiler'
    res, t0 = {}, time.perf_counter()
    for counter in ('FETCH_SIZE', 'WRITE_SIZE'):
        d = tempfile.mkdtemp(prefix='gccnmf_pmc_', dir='/tmp')
        cmd = [roc, '--kernel-trace', '--pmc', counter, '--output-format', 'csv', '-d', d, '-o', 'pass', '--',
               sys.executable, os.path.abspath(__file__), '--gpus', '1', '--steps', '1', '--warmup', '0', '--iterations', str(a.iterations if chained else 10),
               '--files', str(a.files), '--dictionary-size', str(a.dictionary_size), '--hop', str(a.hop), '--seconds', str(a.seconds),
               '--nmf-groups', '1', '--skip-extras', '--skip-roofline', '--skip-config-lines', '--skip-cpu-baseline', '--no-live-traffic']
        env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
        env['TMPDIR'] = '/tmp'
        try:
            p = subprocess.Popen(cmd, cwd='/tmp', env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, start_new_session=True)
            try:
                _o, err = p.communicate(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                import signal
                os.killpg(p.pid, signal.SIGKILL)             # the process group this call started, nothing else
                p.wait()
                shutil.rmtree(d, ignore_errors=True)
                return None, 'the %s pass overran %d s' % (counter, timeout_s)
            if p.returncode != 0:
                shutil.rmtree(d, ignore_errors=True)
                return None, 'the %s pass exited %d: %s' % (counter, p.returncode, err.decode(errors='replace')[-200:])
            vals = []
            for f in glob.glob(os.path.join(d, '**', '*counter_collection.csv'), recursive=True):
                for r in csv.DictReader(open(f)):
                    # K1 and K3 are the same instantiation: A stored [row][k], B not, EPI_DIV (= 1)
                    # the chained launch: ONE kernel holds every GEMM of every iteration of the call
                    want = 'void gccnmf_gemm_chain_kernel<' if chained else 'void gccnmf_gemm_dma_kernel<true, false, 1,'
                    if r['Counter_Name'] == counter and r['Kernel_Name'].startswith(want):
                        vals.append(float(r['Counter_Value']))
            if not vals:
                return None, 'no %s rows for the K1 / K3 kernel' % counter
            res[counter] = (sum(vals) / len(vals), len(vals))
        except Exception as ex:                              # noqa: BLE001 -- a measurement leg must not take the bench line down
            return None, '%s pass: %r' % (counter, ex)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    fetch_kb, n = res['FETCH_SIZE']
    write_kb, _ = res['WRITE_SIZE']
    return ({'hbm_bytes_per_launch': (2.0 * fetch_kb + write_kb) * 1024.0, 'fetch_size_kb_raw': fetch_kb, 'write_size_kb': write_kb,
             'launches': n, 'seconds': time.perf_counter() - t0},
            'measured in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / --pmc WRITE_SIZE (two child runs of bench.py --iterations %d '
            '--nmf-groups 1, mean over %d launches of %s); FETCH_SIZE doubled (gfx950 reports '
            'half of 16 B/lane coalesced reads, MI355X_MICROARCH.md HBM section), KB = 1024 B'
            % (a.iterations if chained else 10, n, 'gccnmf_gemm_chain_kernel<true,4> = the whole KL-NMF call, %d iterations x (K1 | K2 | K3 | K4)' % a.iterations if chained
               else 'gccnmf_gemm_dma_kernel<true,false,1,...> = K1 + K3'))


def kernel_timings(e, iterations=10, launches=20):
    """(ms per KL-NMF iteration, ms per launch of the roofline kernel), HIP events on the stream the kernels are launched on
    (torch's current stream), whole batch per launch on one stream.
      * the iteration: the library's own loop (gccnmf_klnmf, the call the timed steps make, here as ONE file group on one stream) run
        for 3 x `iterations` and for `iterations` iterations between event pairs (best of three each); the difference / (2 x iterations)
        is one iteration without the call's set-up.  (Until round 5 this was timed through gccnmf_klnmf_stage, whose stages 4 + 5 are the UNFUSED
        R.H^T and W-update launches: 8 % more than the loop the product runs at K = 1024.)
      * the roofline kernel (K3: R = V / (W.H), == K1 without the lazy row scale) is a pure function of V, W, H, so it is
        launched `launches` times back to back between one event pair.  Per-kernel averages of the other three launches:
        the committed rocprofv3 summary (profiles/*_g1_bench_kernel_stats.csv)."""
    import torch
    from gcc_nmf_amd import _hip
    from gcc_nmf_amd.engine import _ptr, _stream
    g, lib = e.g, e.lib
    e.W.copy_(e.W0.unsqueeze(0).expand_as(e.W))
    e.H.copy_(e.H0.unsqueeze(0).expand_as(e.H))

    def stage(s):
        _hip.check(lib.gccnmf_klnmf_stage(_ptr(e.V), _ptr(e.W), _ptr(e.H), _ptr(e.ws_nmf), g.F, g.N, g.K, e.batch, e.alpha,
                                          e.eps, e.klnmf_flags, s, _stream()), 'gccnmf_klnmf_stage')
    ws = torch.zeros(lib.gccnmf_klnmf_workspace_floats(g.F, g.N, g.K, e.batch), dtype=torch.float32, device=e.V.device)

    def loop(n):
        _hip.check(lib.gccnmf_klnmf(_ptr(e.V), _ptr(e.W), _ptr(e.H), _ptr(ws), g.F, g.N, g.K, e.batch, n, e.alpha, e.eps, e.klnmf_flags,
                                    _stream()), 'gccnmf_klnmf')
    loop(2)
    stage(0)
    for s in range(1, 6):
        stage(s)
    e2, e3 = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    t_long, t_short = [], []
    for _ in range(3):                      # best of three of each length: a call is a few milliseconds for a short dictionary
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        loop(3 * iterations)
        ev[1].record()
        loop(iterations)
        ev[2].record()
        torch.cuda.synchronize()
        t_long.append(ev[0].elapsed_time(ev[1]))
        t_short.append(ev[1].elapsed_time(ev[2]))
    stage(0)
    stage(3)
    e2.record()
    for _ in range(launches):
        stage(3)
    e3.record()
    torch.cuda.synchronize()
    call_ms = None
    if lib.gccnmf_klnmf_plan(g.F, g.N, g.K, e.batch, e.klnmf_flags) & 8:
        # the chained launch: the whole call (e.iters iterations) is ONE kernel -- time it as the product runs it (the call's few small kernels --
        # zeroing R and the counters, the prepare / final H-scale launches, ~50 us together -- ride inside the event pair)
        ts = []
        for _ in range(3):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e.W.copy_(e.W0.unsqueeze(0).expand_as(e.W))
            e.H.copy_(e.H0.unsqueeze(0).expand_as(e.H))
            ev[0].record()
            loop(e.iters)
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]))
        call_ms = min(ts)
    return (min(t_long) - min(t_short)) / (2 * iterations), e2.elapsed_time(e3) / launches, call_ms


def shared_dictionary_mode(a, e, xs, world, rank, local_rank, barrier, ranks_seen=1, backend='nccl'):
    """BASELINE config 4: ONE dictionary for every file of every rank.  Columns (files) are sharded over ranks, W is
    replicated; each KL-NMF iteration is local GEMMs + one RCCL all-reduce of [num (Fp*Kp) || den (Kp)] floats."""
    import torch
    import torch.distributed as dist
    from gcc_nmf_amd.distributed import HipSharedNMF, shared_initial_factors, train_shared_dictionary
    g, B, K, iters = e.g, e.batch, e.g.K, e.iters
    e.stft()                                                     # V of this rank's files, on device
    files = list(range(rank * B, rank * B + B))
    W0, H0 = shared_initial_factors(g.F, [g.N] * (world * B), K, files, mode='per_file')
    local = HipSharedNMF.from_device(e.V, g.F, g.N, W0, H0)

    def step():
        local.reset()                     # the initial factors uploaded by from_device()
        train_shared_dictionary(local, iters)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device='cuda')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0:
        W = local.W()
        print(json.dumps({
            'metric': 'stereo frames/sec, shared-dictionary KL-NMF training (K=%d, %d iters)' % (K, iters),
            'value': world * B * g.T * a.steps / elapsed, 'unit': 'frames/s', 'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup,
            'ms_per_step': 1e3 * elapsed / a.steps, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32',
            'data': 'synthetic',
            'config': {'workload': '%d files/GPU, one shared dictionary, all-reduce of %d floats per iteration' %
                                   (B, local.partial.numel()), 'files_per_gpu': B, 'dictionary_size': K, 'nmf_iterations': iters,
                       'parallelism': 'columns sharded x%d, W replicated, 1 all-reduce/iteration' % world},
            'ranks_seen': ranks_seen, 'collective_backend': backend if world > 1 else None, 'collective': local.collective,
            'iteration_loop': 'gccnmf_klnmf_shared_run: kernels and the all-reduce enqueued from C, one library call per training',
            'dictionary_finite_unit_norm': bool(np.isfinite(W).all() and np.allclose(np.linalg.norm(W, axis=0), 1.0, atol=1e-4)),
        }))
    if world > 1:
        from gcc_nmf_amd.distributed import destroy_rccl_communicators
        destroy_rccl_communicators()
        dist.destroy_process_group()


def time_sharded_mode(a, world, rank, local_rank, barrier, ranks_seen, backend):
    """ONE long mixture, frame windows sharded over the ranks (north_star's second partitioning): W all-reduce per iteration, one
    all-reduce of the angular spectrum, halo frames all-gathered for the overlap-add seam.  Strong scaling: total work is fixed."""
    import torch
    import torch.distributed as dist
    from gcc_nmf_amd.distributed import HipTimeShard, separate_time_sharded
    from gcc_nmf_amd.synthetic import synthetic_mixture
    sr = 16000
    seconds = a.seconds if a.seconds != 10.0 else 160.0
    x = synthetic_mixture(7, numSamples=int(seconds * sr), sampleRate=sr)
    local = HipTimeShard(x, rank, world, sampleRate=sr, hopSize=a.hop, dictionarySize=a.dictionary_size, device='cuda:%d' % local_rank)

    def step():
        return separate_time_sharded(local, a.iterations)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        seg, start = step()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device='cuda')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0:
        print(json.dumps({
            'metric': 'stereo frames/sec, ONE %.0f s mixture sharded over frame windows (1024-FFT, K=%d, %d NMF iters)' % (seconds, a.dictionary_size, a.iterations),
            'value': local.T_total * a.steps / elapsed, 'unit': 'frames/s', 'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup,
            'ms_per_step': 1e3 * elapsed / a.steps, 'higher_is_better': True, 'scaling': 'strong', 'vs_baseline': None, 'dtype': 'f32',
            'data': 'synthetic',
            'config': {'workload': 'one %.0f s stereo mixture (%d frames), samples resident in HBM -> host waveform segments out; frames sharded x%d, '
                                   'W replicated: %d all-reduces of F*K+K floats, 1 of 128 doubles, 1 all-gather of 3 halo frames per signal'
                                   % (seconds, local.T_total, world, a.iterations), 'frames': local.T_total, 'dictionary_size': a.dictionary_size,
                       'nmf_iterations': a.iterations, 'parallelism': 'frame windows sharded x%d' % world},
            'ranks_seen': ranks_seen, 'collective_backend': backend if world > 1 else None, 'collective': local.nmf.collective,
            'column_blocks': [list(b) for b in local.nmf.blocks],
            'tdoa_indexes': local.tdoa_indexes().tolist(), 'segment_finite': bool(np.isfinite(seg).all())}))
    if world > 1:
        barrier()
        from gcc_nmf_amd.distributed import destroy_rccl_communicators
        destroy_rccl_communicators()
        dist.destroy_process_group()


def streaming_measure(K, n_h, seconds=10.0):
    """(low-latency configuration, the reference's own configuration) of BASELINE config 5, each a dict of per-block latencies; see
    streaming_mode."""
    import torch
    from gcc_nmf_amd.realtime import GCCNMFProcessor, StreamingGCCNMF, asymmetricWindows
    from gcc_nmf_amd.synthetic import synthetic_mixture
    ws, hop, B, D, sr = 512, 64, 64, 64, 16000
    rng = np.random.RandomState(0)
    W = rng.rand(ws // 2 + 1, K).astype(np.float32) + 0.02
    W /= np.linalg.norm(W, axis=0)
    x = synthetic_mixture(0, numSamples=int(sr * seconds), delays=(-3, 1, 4))
    n_blocks = x.shape[1] // B
    block_ms = 1e3 * B / sr

    def measure(numHUpdates, windows, delay):
        kw = dict(analysisWindow=windows[0], synthesisWindow=windows[1]) if windows else {}
        p = GCCNMFProcessor(sr, ws, B // hop, {'Pretrained': {K: W}}, 'Pretrained', K, numHUpdates, 0.1, True, 6, numTDOAs=D, **kw)
        p.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
        s = StreamingGCCNMF(p, hop, B, outputDelayBlocks=delay)
        for b in range(50):
            s.process_block(x[:, b * B:(b + 1) * B])
        lat = []
        for b in range(50, n_blocks):
            t0 = time.perf_counter()
            y = s.process_block(x[:, b * B:(b + 1) * B])
            lat.append(time.perf_counter() - t0)
        lat = np.array(lat) * 1e3
        p.reset()
        p.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
        s2 = StreamingGCCNMF(p, hop, B, outputDelayBlocks=delay)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s2.process_stream(x)
        torch.cuda.synchronize()
        dev_ms = (time.perf_counter() - t0) * 1e3 / n_blocks
        return {'p50_ms': float(np.percentile(lat, 50)), 'p99_ms': float(np.percentile(lat, 99)), 'max_ms': float(lat.max()),
                'mean_ms': float(lat.mean()), 'blocks': int(len(lat)), 'real_time_factor_p50': float(np.percentile(lat, 50) / block_ms),
                'real_time_factor_p99': float(np.percentile(lat, 99) / block_ms), 'device_resident_ms_per_block': dev_ms,
                'device_resident_real_time_factor': dev_ms / block_ms, 'tracked_tdoa_index': p.targetTDOAIndex,
                'output_finite': bool(np.isfinite(y).all())}

    return measure(n_h, asymmetricWindows(ws, 2 * hop), 1), measure(0, None, 2), dict(ws=ws, hop=hop, B=B, D=D, sr=sr, block_ms=block_ms)


def streaming_mode(a):
    """BASELINE config 5: RT-GCC-NMF, pre-trained-size K = 1024 dictionary, 512-pt ASYMMETRIC analysis / synthesis windows (synthesis
    window 128 samples), hop = block = 64 samples (4 ms at 16 kHz), per-frame coefficient inference (numHUpdates KL-NMF H updates with
    W fixed) + mask, 64 TDOAs, online localisation.  Reports p50 / p99 of the fused device call per block (host block in -> host block
    out, i.e. including both PCIe copies and the stream sync), the real-time factor, and the device-resident rate; the same numbers
    for the reference's own configuration of that path (symmetric sqrt-hamming window, no coefficient inference) ride along."""
    import torch
    torch.cuda.set_device(0)
    K, n_h = a.dictionary_size, a.h_updates
    low, ref, c = streaming_measure(K, n_h)
    ws, hop, B, sr, block_ms = c['ws'], c['hop'], c['B'], c['sr'], c['block_ms']
    print(json.dumps({
        'metric': 'RT-GCC-NMF p50 per-frame latency (512-pt asymmetric window, hop 64, K=%d, %d H updates per frame)' % (K, n_h),
        'value': low['p50_ms'], 'unit': 'ms', 'n_gpus': 1, 'steps': low['blocks'], 'warmup': 50, 'ms_per_step': low['mean_ms'],
        'higher_is_better': False, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
        'config': {'workload': 'streaming: 1 frame of 512 samples per 64-sample block; asymmetric analysis (512) / synthesis (128) windows, '
                               'output one block late; K=%d, %d coefficient (H) updates per frame with W fixed, soft TDOA mask, 64 TDOAs, '
                               'online localisation window 6; host block in -> host block out per call' % (K, n_h),
                   'window': ws, 'synthesis_window': 2 * hop, 'hop': hop, 'block': B, 'numHUpdates': n_h,
                   'algorithmic_latency_ms': 1e3 * 2 * hop / sr},
        'p99_ms': low['p99_ms'], 'max_ms': low['max_ms'], 'block_duration_ms': block_ms,
        'real_time_factor_p50': low['real_time_factor_p50'], 'real_time_factor_p99': low['real_time_factor_p99'],
        'device_resident_ms_per_block': low['device_resident_ms_per_block'],
        'device_resident_real_time_factor': low['device_resident_real_time_factor'], 'tracked_tdoa_index': low['tracked_tdoa_index'],
        'output_finite': low['output_finite'],
        'reference_configuration': dict(ref, note='the reference processor as it is: symmetric sqrt-hamming 512-pt window for analysis and '
                                                  'synthesis, no coefficient inference (its numHUpdates is unused), output two blocks late')}))


def config_lines(a, e, xs, sr, n, local_rank):
    """BASELINE.json's OTHER configurations and the dictionary sizes between the two tuned points, each timed LIVE on rank 0 after the
    timed region of the default line (until round 4 these rested on builder-kept files under profiles/ only).  Compact
    sub-records; every engine is released before the next one is built.  Whole call: about a minute."""
    import torch
    from gcc_nmf_amd.engine import GCCNMFEngine
    B, dev = e.batch, 'cuda:%d' % local_rank
    res = {}

    def timed_runs(eng, steps):
        eng.run()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(steps):
            eng.run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t1) / steps

    def batch_line(K, hop, steps, iters=100):
        eng = GCCNMFEngine(n, sampleRate=sr, windowSize=1024, hopSize=hop, numTDOAs=128, microphoneSeparationInMetres=1.0, numTargets=3,
                           dictionarySize=K, numIterations=iters, batch=B, device=dev)
        eng.upload(xs)
        dt = timed_runs(eng, steps)
        g = eng.g
        iter_ms, k3_ms, _call_ms = kernel_timings(eng, iterations=10, launches=10)
        gemm_flop = 2.0 * g.F * g.K * g.N * B
        plan = int(eng.lib.gccnmf_klnmf_plan(g.F, g.N, g.K, eng.batch, eng.klnmf_flags))
        slabs = bool(plan & 4)
        rec = {'files': B, 'hop': hop, 'dictionary_size': K, 'nmf_iterations': iters, 'frames_per_s': B * g.T / dt, 'ms_per_step': 1e3 * dt,
               'nmf_file_groups': eng.nmf_groups, 'klnmf_plan': plan,
               'iteration_ms_one_stream': float(iter_ms), 'iteration_frac': 4 * gemm_flop / (iter_ms * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS,
               'roofline': {'bound': 'mfma', 'kernel': 'gccnmf_whdiv_rht_kernel (K3 + K4a, one launch)' if slabs else 'gccnmf_gemm_dma_kernel (K3)',
                            'achieved': (2 if slabs else 1) * gemm_flop / (k3_ms * 1e-3) / 1e12, 'peak': F32_MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s',
                            'frac': (2 if slabs else 1) * gemm_flop / (k3_ms * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS, 'avg_launch_ms': float(k3_ms)},
               'tdoa_indexes_as_expected': bool((eng.get_tdoa_indexes() == np.array([27, 59, 91])).all()) if (n, hop) == (160000, 256) else None}
        del eng
        torch.cuda.empty_cache()
        return rec

    # config 1's dictionary (the reference driver's K = 128, runGCCNMF.py:41) at batch scale, at BASELINE's hop and at the driver's own (:60)
    res['k128_batch'] = {'hop256': batch_line(128, 256, 5), 'hop128': batch_line(128, 128, 3),
                         'what': 'BASELINE config 1 parameters (K = 128, 100 iterations) on config 3\'s batch; hop 128 = runGCCNMF.py:60'}
    # realtime/config.py:71 trains [64, 128, 256, 512, 1024]: the sizes between the tuned points
    res['k_sweep'] = {str(K): batch_line(K, 256, 2) for K in (64, 256, 512)}
    # config 3 as written: 200 iterations
    e.iters = 200
    dt = timed_runs(e, 2)
    e.iters = a.iterations
    e.run()                              # e.y is the headline configuration's result again (the CPU-baseline leg compares it with the oracle)
    torch.cuda.synchronize()
    res['it200'] = {'files': B, 'nmf_iterations': 200, 'frames_per_s': B * e.g.T / dt, 'ms_per_step': 1e3 * dt, 'what': 'BASELINE config 3 as written'}
    # config 4's per-rank shape: one dictionary for the rank's files (no exchange at one rank)
    from gcc_nmf_amd.distributed import HipSharedNMF, shared_initial_factors, train_shared_dictionary
    g = e.g
    e.stft()
    W0, H0 = shared_initial_factors(g.F, [g.N] * B, g.K, list(range(B)), mode='per_file')
    local = HipSharedNMF.from_device(e.V, g.F, g.N, W0, H0)

    def shared_step():
        local.reset()
        train_shared_dictionary(local, a.iterations)
    shared_step()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(2):
        shared_step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t1) / 2
    res['shared_dictionary_n1'] = {'files': B, 'frames_per_s': B * g.T / dt, 'ms_per_step': 1e3 * dt, 'collective': local.collective,
                                   'what': 'BASELINE config 4 on one rank: one dictionary for %d files, the iteration loop in C' % B}
    del local, W0, H0
    torch.cuda.empty_cache()
    # config 5
    low, ref, c = streaming_measure(a.dictionary_size, a.h_updates, seconds=4.0)
    res['streaming'] = {'p50_ms': low['p50_ms'], 'p99_ms': low['p99_ms'], 'real_time_factor_p50': low['real_time_factor_p50'],
                        'device_resident_ms_per_block': low['device_resident_ms_per_block'], 'blocks': low['blocks'],
                        'reference_configuration_p50_ms': ref['p50_ms'], 'block_duration_ms': c['block_ms'],
                        'what': 'BASELINE config 5: 512-pt asymmetric windows, hop 64, K = %d, %d H updates per frame, host block in -> out' % (a.dictionary_size, a.h_updates)}
    # the dictionary pre-training call (gccNMFPretraining.py:79-80): ONE matrix of 80 000 columns through the column-block path
    from gcc_nmf_amd.distributed import HipSharedColumns
    from gcc_nmf_amd.engine import Geometry
    N, K, iters, F = 80000, 1024, 10, 513
    gg = Geometry(F, 1, K)
    gen = torch.Generator(device=dev).manual_seed(80000)
    Vd = torch.zeros((gg.Fp, N), device=dev)
    Wd = torch.zeros((gg.Fp, gg.Kp), device=dev)
    Hd = torch.zeros((gg.Kp, N), device=dev)
    Vd[:F] = torch.rand((F, N), device=dev, generator=gen) + 0.01
    Wd[:F, :K] = torch.rand((F, K), device=dev, generator=gen) + 1e-16
    Hd[:K] = torch.rand((K, N), device=dev, generator=gen) + 1e-16
    run = HipSharedColumns(Vd, Hd, Wd, F, N, K)
    run.run(2, collective=False)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    run.run(iters, collective=False)
    ev1.record()
    torch.cuda.synchronize()
    ms = ev0.elapsed_time(ev1)
    res['big_matrix_n80000'] = {'N': N, 'K': K, 'iterations': iters, 'ms_per_iteration': ms / iters,
                                'frac_of_f32_mfma_peak': 4 * 2.0 * F * K * N * iters / ms / 1e9 / F32_MFMA_PEAK_TFLOPS,
                                'what': 'performKLNMF on ONE (513, 80000) matrix: in-place column blocks on the batched kernels (device-resident part)'}
    del run, Vd, Wd, Hd
    torch.cuda.empty_cache()
    return res


def dev1_mixture():
    """The reference driver's own input (data/dev1_female3_liverec_130ms_1m_mix.wav, committed under tests/golden/data), converted like
    the reference's wavread (gccNMF/wavfile.py:34-37).  The drop-in sequence computes the coherence quotient in the DRIVER's NumPy
    (runGCCNMF.py:44), where an exactly-zero f32 bin of a synthetic file is 0/0 = NaN; real recordings do not have one."""
    from scipy.io import wavfile
    sr, pcm = wavfile.read(os.path.join(REPO, 'tests', 'golden', 'data', 'dev1_female3_liverec_130ms_1m_mix.wav'))
    return (pcm.astype('float32') / 32768).T.copy()


def dropin_sequence(x, sr, hop, K, iters=100, resident=False, repeats=5, G=None):
    """The eight reference-named functions in the order of gccNMF/runGCCNMF.py:36-52, HOST arrays in and out of each, timed one by one
    (best of `repeats` per function after one warm-up pass that fills the buffer pools); `driver_numpy_ms` is the NumPy the reference
    driver itself runs between them (abs / concatenate / the coherence quotient / hsplit / mean), not part of the eight."""
    if G is None:
        from gcc_nmf_amd import gccNMFFunctions as G
    names = ['computeComplexMixtureSpectrogram', 'performKLNMF', 'getAngularSpectrogram', 'estimateTargetTDOAIndexesFromAngularSpectrum',
             'getTargetTDOAGCCNMFs', 'getTargetCoefficientMasks', 'getTargetSpectrogramEstimates', 'getTargetSignalEstimates']
    best = dict((nm, float('inf')) for nm in names)
    best_between, best_total = float('inf'), float('inf')
    if hasattr(G, 'set_resident'):
        G.set_resident(resident)
    try:
        for rep in range(repeats + 1):
            t = {}
            between = 0.0

            def timed(nm, *args, **kw):
                t0 = time.perf_counter()
                r = getattr(G, nm)(*args, **kw)
                t[nm] = time.perf_counter() - t0
                return r
            t_start = time.perf_counter()
            X = timed('computeComplexMixtureSpectrogram', x, 1024, hop, np.hanning)
            t0 = time.perf_counter()
            numChannels, numFrequencies, numTime = X.shape
            frequenciesInHz = np.linspace(0, sr / 2.0, numFrequencies)
            V = np.concatenate(abs(X), axis=-1)
            between += time.perf_counter() - t0
            W, H = timed('performKLNMF', V, K, iters, 0)
            t0 = time.perf_counter()
            stereoH = np.array(np.hsplit(H, numChannels))
            C = X[0] * X[1].conj() / abs(X[0]) / abs(X[1])
            between += time.perf_counter() - t0
            A = timed('getAngularSpectrogram', C, frequenciesInHz, 1.0, 128)
            t0 = time.perf_counter()
            meanA = np.mean(A, axis=-1)
            between += time.perf_counter() - t0
            idx = timed('estimateTargetTDOAIndexesFromAngularSpectrum', meanA, 1.0, 128, 3)
            Gs = timed('getTargetTDOAGCCNMFs', C, 1.0, 128, frequenciesInHz, idx, W, stereoH)
            M = timed('getTargetCoefficientMasks', Gs, 3)
            S = timed('getTargetSpectrogramEstimates', M, X, W, stereoH)
            y = timed('getTargetSignalEstimates', S, 1024, hop, np.hanning)
            total = time.perf_counter() - t_start
            if rep:
                for nm in names:
                    best[nm] = min(best[nm], t[nm])
                best_between = min(best_between, between)
                best_total = min(best_total, total)
            del X, V, W, H, stereoH, C, A, Gs, M, S
    finally:
        if hasattr(G, 'set_resident'):
            G.set_resident(False)
    return {'mode': 'resident' if resident else 'copying', 'frames': int(numTime), 'hop': hop, 'dictionary_size': K, 'iterations': iters,
            'ms': dict((nm, 1e3 * best[nm]) for nm in names), 'sum_of_the_eight_ms': 1e3 * sum(best.values()),
            'driver_numpy_ms': 1e3 * best_between, 'whole_sequence_ms': 1e3 * best_total, 'tdoa': [int(i) for i in idx],
            'y_rms': float(np.sqrt(np.mean(y.astype(np.float64) ** 2)))}


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run, one rank per GPU, rendezvous on
    127.0.0.1 (the container hostname may not resolve)."""
    import socket
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # dmabuf IPC: RCCL needs it on this driver
    sys.stdout.flush()
    os.execv(sys.executable, cmd)


def main():
    a = parse()
    if a.mode == 'streaming':
        return streaming_mode(a)
    if a.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        self_launch(a.gpus)
    import torch
    import torch.distributed as dist
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if world != a.gpus:
        raise SystemExit('bench.py: --gpus %d but WORLD_SIZE=%d: launch exactly one rank per GPU' % (a.gpus, world))
    # one rank per GPU over RCCL; GCCNMF_BENCH_BACKEND=gloo lets several ranks share one GPU to rehearse the N > 1 code path
    backend = os.environ.get('GCCNMF_BENCH_BACKEND', 'nccl')
    local_rank = local_rank % max(torch.cuda.device_count(), 1) if backend != 'nccl' else local_rank
    torch.cuda.set_device(local_rank)
    if world > 1:
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=torch.device('cuda', local_rank))
        else:
            import datetime
            dist.init_process_group(backend, timeout=datetime.timedelta(seconds=300))

    # every rank adds 1 over the data-path backend (RCCL unless GCCNMF_BENCH_BACKEND says otherwise): the job really is N ranks
    ranks_seen = 1
    if world > 1:
        t = torch.ones(1, dtype=torch.int32, device='cuda')
        dist.all_reduce(t)
        ranks_seen = int(t.item())
        if ranks_seen != a.gpus:
            raise SystemExit('bench.py: %d ranks answered the all-reduce, --gpus %d' % (ranks_seen, a.gpus))

    def barrier():
        if world > 1:
            if backend == 'nccl':
                dist.barrier(device_ids=[local_rank])
            else:
                dist.barrier()

    if a.mode == 'time-sharded':
        return time_sharded_mode(a, world, rank, local_rank, barrier, ranks_seen, backend)

    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_batch
    for kv in a.tune:
        from gcc_nmf_amd import _hip
        key, val = [int(v) for v in kv.split('=')]
        _hip.check(_hip.lib().gccnmf_set_tuning(key, val), 'gccnmf_set_tuning')

    sr = 16000
    n = int(a.seconds * sr)
    K, iters, B = a.dictionary_size, a.iterations, a.files
    xs = synthetic_batch(rank * B, B, numSamples=n, sampleRate=sr)          # each rank: its own shard of files
    e = GCCNMFEngine(n, sampleRate=sr, windowSize=1024, hopSize=a.hop, numTDOAs=128, microphoneSeparationInMetres=1.0,
                     numTargets=3, dictionarySize=K, numIterations=iters, batch=B, device='cuda:%d' % local_rank,
                     klnmf_flags=1 if a.no_xcd_affinity else 0, nmf_groups=a.nmf_groups)
    g = e.g
    e.upload(xs)                                                             # inputs resident in HBM before timing

    if a.mode == 'shared-dictionary':
        return shared_dictionary_mode(a, e, xs, world, rank, local_rank, barrier, ranks_seen, backend)

    for _ in range(a.warmup):
        e.run()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        e.run()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device='cuda')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    e.check_status()
    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, e)

    frames = world * B * g.T * a.steps
    out = {
        'metric': 'stereo frames/sec (1024-FFT, K=%d, %d NMF iters)' % (K, iters),
        'value': frames / elapsed, 'unit': 'frames/s', 'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup,
        'ms_per_step': 1e3 * elapsed / a.steps, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': 'f32', 'data': 'synthetic',
        'config': {'workload': 'HBM-resident (float32 samples in HBM -> separated float32 waveforms in HBM; the host-to-host rates are '
                               'the host_to_host_* fields of a --full run): %d x %.0f s stereo @16 kHz synthetic mixtures per GPU (SURVEY 8d recipe), '
                               '1024-pt FFT hop %d (F=513, T=%d/file), K=%d, %d KL-NMF iters, 128 TDOAs, 3 targets, independent '
                               'dictionary per file' % (B, a.seconds, a.hop, g.T, K, iters),
                   'files_per_gpu': B, 'frames_per_file': g.T, 'dictionary_size': K, 'nmf_iterations': iters,
                   'parallelism': 'file-sharded x%d, no data-path collective' % world,
                   'nmf_file_groups_per_gpu': e.nmf_groups},
        'ranks_seen': ranks_seen,
    }
    if a.full:
        out['tdoa_indexes_as_expected'] = bool((e.get_tdoa_indexes() == np.array([27, 59, 91])).all()) if a.seconds == 10.0 else None
    # the whole path against the f32-MFMA roofline -- algorithmic flop per stereo frame (NMF 16 F K iters + STFT,
    # angular spectrum, scores, reconstruction, iSTFT) / peak; per GPU, so the fraction holds at any N
    flop_per_frame = 16.0 * g.F * K * iters + 2 * 5 * 1024 * 10 + 2.0 * 128 * 2 * g.F + 3 * 2.0 * g.F * K + 3 * 2 * 2.0 * g.F * K + 3 * 2 * 5 * 1024 * 10
    ceiling = F32_MFMA_PEAK_TFLOPS * 1e12 / flop_per_frame
    out['end_to_end_vs_mfma_roofline'] = {'flop_per_frame': flop_per_frame, 'ceiling_frames_per_s_per_gpu': ceiling,
                                          'frac': frames / elapsed / world / ceiling}

    # --full: everything beyond the headline figure, after it is measured (and after --dump-outputs has saved the timed step's results)
    extras, roofline = a.full and not a.skip_extras, a.full and not a.skip_roofline
    if rank == 0 and extras:
        # host float32 samples in -> host float32 waveforms out (PCIe both ways); reported beside `value`, never as `value`
        e.separate(xs)                                           # allocates the page-locked staging buffers (slow, once per engine)
        t1 = time.perf_counter()
        e.separate(xs)
        out['host_to_host_frames_per_s'] = B * g.T / (time.perf_counter() - t1)           # one batch, copies not overlapped
        nb = 8                                                   # fill + drain of the pipeline are ~1/3 of a batch time: amortised over 8
        for _y in e.separate_batches([xs]):                      # allocates the second device slot + the pipeline's page-locked buffers
            pass
        t1 = time.perf_counter()
        for _y in e.separate_batches(xs for _ in range(nb)):
            pass
        out['host_to_host_pipelined_frames_per_s'] = nb * B * g.T / (time.perf_counter() - t1)   # transfers under the neighbours' compute
        # SURVEY 8(d) defines the metric host float32 samples in -> host float32 waveforms out; the bench contract defines `value`
        # with the inputs already resident in HBM (and forbids the PCIe-inclusive rate there).  Both are in this line:
        out['sec8d_host_to_host'] = {'value': out['host_to_host_pipelined_frames_per_s'], 'unit': 'frames/s', 'batches': nb,
                                     'what': 'SURVEY 8(d) metric: host float32 samples in -> host float32 separated waveforms out, %d batches '
                                             'of %d files back to back through GCCNMFEngine.separate_batches (pinned staging, copies of batch '
                                             'i+-1 under the compute of batch i), pipeline fill and drain included' % (nb, B),
                                     'single_batch_unpipelined': out['host_to_host_frames_per_s'],
                                     'hbm_resident': frames / elapsed / world}

    if rank == 0 and roofline:
        traffic_file = os.path.join(REPO, 'profiles', 'pmc_traffic.json')
        pmc = json.load(open(traffic_file)) if os.path.exists(traffic_file) else None
        iter_ms, k3_ms, chain_call_ms = kernel_timings(e)
        gemm_flop = 2.0 * g.F * g.K * g.N * B                                # algorithmic: F=513, N=2T, not the padded tile grid
        # short dictionaries: the library may run K3 + K4a as ONE launch of 64-bin slabs (gccnmf_klnmf_plan bit 2) -- then that launch is
        # the dominant kernel, and it holds two GEMMs
        slabs = bool(e.lib.gccnmf_klnmf_plan(g.F, g.N, g.K, e.batch, e.klnmf_flags) & 4)
        flop_per_launch = (2 if slabs else 1) * gemm_flop
        achieved = flop_per_launch / (k3_ms * 1e-3) / 1e12
        kernel_name = ('gccnmf_whdiv_rht_kernel (K3 + K4a in one launch: U = (V / (W.H)) . H^T, R never written)' if slabs else
                       'gccnmf_gemm_dma_kernel<A_KC,!B_KC,EPI_DIV,TAIL,TM=4,NARROW> (K1/K3: W.H with V/(.) epilogue; 19 wide + 1 narrow item per file)')
        out['roofline'] = {'bound': 'mfma', 'kernel': kernel_name,
                           'achieved': achieved, 'peak': F32_MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s', 'frac': achieved / F32_MFMA_PEAK_TFLOPS,
                           'traffic': None, 'flop_per_launch': flop_per_launch, 'avg_launch_ms': float(k3_ms),
                           'launch': 'one launch over all %d files on one stream, %d back to back (the timed steps run KL-NMF as %d file '
                                     'group(s) on separate streams, whose launches overlap in time; rocprofv3 averages of this launch: '
                                     'python bench.py --nmf-groups 1)' % (B, 20, e.nmf_groups)}
        chained = chain_call_ms is not None
        if chained:
            # The dominant kernel of the product path is now the chained launch itself: every GEMM of every iteration of the call in one kernel
            # (tuning key 21).  achieved = the call's algorithmic flop (4 GEMMs x iterations) / the launch's duration; the K3 launch ALONE (the
            # dominant kernel of rounds 1-5, still what a forced plain form runs) stays in `k3_alone`.
            out['roofline'].update({
                'kernel': 'gccnmf_gemm_chain_kernel<TAIL,4> (the whole KL-NMF call: %d iterations x (K1 | K2 | K3 | K4 with the fused W update), tiles handed '
                          'over through ready counters in the XCD\'s L2)' % iters,
                'achieved': 4 * gemm_flop * iters / (chain_call_ms * 1e-3) / 1e12, 'flop_per_launch': 4 * gemm_flop * iters, 'avg_launch_ms': float(chain_call_ms),
                'launch': 'ONE launch per gccnmf_klnmf call over all %d files on one stream, best of 3 (HIP events on the launch stream)' % B,
                'k3_alone': {'kernel': kernel_name, 'achieved': achieved, 'frac': achieved / F32_MFMA_PEAK_TFLOPS, 'flop_per_launch': flop_per_launch,
                             'avg_launch_ms': float(k3_ms), 'launch': '20 plain launches of K3 back to back'}})
            out['roofline']['frac'] = out['roofline']['achieved'] / F32_MFMA_PEAK_TFLOPS
            # unique operand bytes of one iteration: K1 / K3 read V, W, H and write R; K2 reads W, R, H and writes H; K4 reads R, H, W and writes W
            per_file = 4.0 * (2 * (g.F * g.N * 2 + g.F * K + K * g.N) + (g.F * K + g.F * g.N + 2 * K * g.N) + (g.F * g.N + K * g.N + 2 * g.F * K))
            out['roofline']['traffic_algorithmic_unique_bytes'] = per_file * B * iters
        if not chained and pmc and pmc.get('files_per_gpu') == B and pmc.get('dictionary_size') == K and a.seconds == 10.0 and a.hop == 256:
            # HBM bytes per launch of this kernel from separate rocprofv3 --pmc passes (profiles/README.md), gfx950-corrected
            out['roofline']['traffic'] = pmc['k1_hbm_bytes_per_launch']
            out['roofline']['traffic_source'] = pmc['source']
            out['roofline']['traffic_algorithmic_unique_bytes'] = pmc.get('k1_algorithmic_unique_bytes')
        # one KL-NMF iteration = the four dependent GEMM launches of the library's own loop (W update fused into the R.H^T launch), whole
        # batch on ONE stream: difference of two gccnmf_klnmf calls of different lengths.  The kernel trace shows the launches back to
        # back (start of n+1 = end of n, profiles/r05o_launch_gaps.json), so this is the sum of the four kernel durations; the timed
        # steps run two file groups on two streams and overlap the tail of one group's launch with the head of the other's.  Round 6: where the
        # library chains the call (gccnmf_klnmf_plan bit 3) there are no launches per iteration any more -- this is the steady-state cost of one
        # iteration inside the call's single launch, and the timed steps run ONE file group.
        out['nmf_iteration_one_stream'] = {'ms': float(iter_ms), 'tflops': 4 * gemm_flop / (iter_ms * 1e-3) / 1e12,
                                           'frac_of_peak': 4 * gemm_flop / (iter_ms * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS}

    if rank == 0 and world == 1 and extras:
        # the same parameters on ONE mixture (BASELINE config 2's shape): latency-bound, small-batch GEMM tile
        e1 = GCCNMFEngine(n, sampleRate=sr, windowSize=1024, hopSize=a.hop, numTDOAs=128, microphoneSeparationInMetres=1.0,
                          numTargets=3, dictionarySize=K, numIterations=iters, batch=1, device='cuda:%d' % local_rank)
        e1.upload(xs[0])
        e1.run()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(3):
            e1.run()
        torch.cuda.synchronize()
        dt1 = (time.perf_counter() - t1) / 3
        out['single_file'] = {'frames_per_s': g.T / dt1, 'ms_per_file': 1e3 * dt1,
                              # the whole path's algorithmic flop per frame over the time of ONE mixture alone (latency path, csrc/direct.hip)
                              'frac_of_mfma_peak': flop_per_frame * g.T / dt1 / (F32_MFMA_PEAK_TFLOPS * 1e12),
                              # different GEMM tile (launch-size dependent) -> different summation grouping, not bitwise equal
                              'waveform_rms_vs_in_batch': float(np.sqrt(np.mean((e1.y[0].cpu().numpy().astype(np.float64) - e.y[0].cpu().numpy()) ** 2)))}

    if rank == 0 and world == 1 and extras:
        # the drop-in route: the reference-named host-array function (NumPy V in -> NumPy W, H out), as runGCCNMF.py calls it
        from gcc_nmf_amd import gccNMFFunctions as G
        V0 = e.get_V()[0]
        G.performKLNMF(V0, K, 2, 0)                                           # allocates the cached device buffers for this shape
        t1 = time.perf_counter()
        G.performKLNMF(V0, K, iters, 0)
        out['dropin_performKLNMF'] = {'ms': 1e3 * (time.perf_counter() - t1), 'frames_per_s': g.T / (time.perf_counter() - t1),
                                      'what': 'gcc_nmf_amd.gccNMFFunctions.performKLNMF(V (%d, %d) ndarray, %d, %d, 0): host arrays in and out'
                                              % (g.F, g.N, K, iters)}

    if rank == 0 and world == 1 and extras and (K, a.hop) != (128, 128):
        # the reference driver's OWN call (gccNMF/runGCCNMF.py:41,60: dictionarySize = 128, hopSize = 128 -> performKLNMF(V (513, 2486), 128, 100, 0)),
        # one mixture alone, next to the headline shape: what `python runGCCNMF.py` on top of dropin.install() spends on the device
        e2 = GCCNMFEngine(n, sampleRate=sr, windowSize=1024, hopSize=128, numTDOAs=128, microphoneSeparationInMetres=1.0,
                          numTargets=3, dictionarySize=128, numIterations=100, batch=1, device='cuda:%d' % local_rank)
        e2.upload(xs[0])
        e2.run()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(3):
            e2.run()
        torch.cuda.synchronize()
        dt2 = (time.perf_counter() - t1) / 3
        from gcc_nmf_amd import gccNMFFunctions as G
        V2 = e2.get_V()[0]
        G.performKLNMF(V2, 128, 2, 0)
        t1 = time.perf_counter()
        G.performKLNMF(V2, 128, 100, 0)
        out['reference_driver_shape'] = {'what': 'one mixture at the reference driver\'s own parameters (runGCCNMF.py:41,60): K = 128, hop 128, 100 iterations',
                                         'frames': e2.g.T, 'ms_per_file': 1e3 * dt2, 'frames_per_s': e2.g.T / dt2,
                                         'dropin_performKLNMF_ms': 1e3 * (time.perf_counter() - t1)}
        del e2

    if rank == 0 and world == 1 and extras and (K, iters, a.seconds) == (1024, 100, 10.0):
        # the whole drop-in sequence, function by function, host arrays in and out: the reference driver's own shape and BASELINE config 2's,
        # in the default (copying) mode and in the opt-in resident mode of dropin.install(resident=True)
        out['dropin_sequence'] = {
            'what': 'the eight reference-named functions of gcc_nmf_amd.gccNMFFunctions in runGCCNMF.py:36-52 order on the dev1 mixture (10 s, the reference driver\'s input), NumPy '
                    'arrays in and out of every call, best of 5 per function after one warm-up pass',
            'driver_shape_hop128_K128': {'copying': dropin_sequence(dev1_mixture(), sr, 128, 128), 'resident': dropin_sequence(dev1_mixture(), sr, 128, 128, resident=True)},
            'config2_hop256_K1024': {'copying': dropin_sequence(dev1_mixture(), sr, 256, 1024), 'resident': dropin_sequence(dev1_mixture(), sr, 256, 1024, resident=True)}}

    if rank == 0 and world == 1 and extras and (K, iters, a.hop, a.seconds) == (1024, 100, 256, 10.0):
        # mixtures of DIFFERENT lengths in one batch (runGCCNMF.py:30-36 takes a file of any length): 21 x 5 s + 21 x 10 s + 22 x 15 s, KL-NMF over
        # all 64 files in one ragged chained launch, against the equal-length rate of this run at (nearly) the same total frames
        from gcc_nmf_amd.engine import RaggedGCCNMFEngine
        from gcc_nmf_amd.synthetic import synthetic_mixture
        lengths = ([80000, 160000, 240000] * 22)[:64]
        mix = [synthetic_mixture(2000 + i, numSamples=m, sampleRate=sr) for i, m in enumerate(lengths)]
        er = RaggedGCCNMFEngine(lengths, sampleRate=sr, windowSize=1024, hopSize=a.hop, numTDOAs=128, microphoneSeparationInMetres=1.0, numTargets=3,
                                dictionarySize=K, numIterations=iters, device='cuda:%d' % local_rank)
        er.upload(mix)
        er.run()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(3):
            er.run()
        torch.cuda.synchronize()
        dtr = (time.perf_counter() - t1) / 3
        for sub in er.sub.values():
            sub.check_status()
        out['mixed_lengths'] = {'files': 64, 'seconds_per_file': {'5': lengths.count(80000), '10': lengths.count(160000), '15': lengths.count(240000)},
                                'frames': int(sum(er.frames)), 'ms_per_step': 1e3 * dtr, 'frames_per_s': sum(er.frames) / dtr,
                                'one_ragged_launch': er.ragged_klnmf_used, 'vs_equal_length_rate': sum(er.frames) / dtr / (frames / elapsed),
                                'what': 'HBM-resident, like `value`: samples in HBM -> waveforms in HBM; KL-NMF of all 64 files in ONE chained launch '
                                        '(gccnmf_klnmf_ragged: per-file column tiles, files dealt out to the XCDs by length), the one-shot stages per length'}
        del er

    if rank == 0 and world == 1 and extras and not a.skip_config_lines and (K, iters, a.hop, a.seconds) == (1024, 100, 256, 10.0):
        t1 = time.perf_counter()
        out.update(config_lines(a, e, xs, sr, n, local_rank))
        out['config_lines_seconds'] = time.perf_counter() - t1

    if rank == 0 and world == 1 and not a.skip_cpu_baseline and extras:
        from oracle import gccnmf_oracle as O                                # the checker, timed as the CPU baseline
        from threadpoolctl import threadpool_info, threadpool_limits
        threads = max([i.get('num_threads', 1) for i in threadpool_info()] or [1])

        def oracle_run():
            t1 = time.perf_counter()
            r = O.runGCCNMF(xs[0], sr, 1024, a.hop, 128, 1.0, 3, dictionarySize=K, numIterations=iters, return_intermediates=True)
            return time.perf_counter() - t1, r
        # best of 3 after one warm-up on all host cores, and one BLAS thread (OPENBLAS_NUM_THREADS=1 equivalent).  On
        # a 256-CPU box OpenBLAS's 128 threads are SLOWER than one on these matrix sizes (measured 183 vs 285 frames/s), so the
        # reported baseline is the best over a small thread sweep -- the CPU at its best, not at its default.
        oracle_run()
        runs = [oracle_run() for _ in range(3)]
        dt_all, r = min(runs, key=lambda v: v[0])
        sweep = {int(threads): dt_all}
        for th in (1, 4, 16, 64):
            if th < threads:
                with threadpool_limits(limits=th):
                    sweep[th] = min(oracle_run()[0] for _ in range(2))
        best_th = min(sweep, key=sweep.get)
        dt = sweep[best_th]
        out['cpu_baseline'] = {'value': g.T / dt, 'unit': 'frames/s', 'cores': int(best_th), 'kind': 'port',
                               'sample': '1 of the %d files (%d stereo frames), same parameters, NumPy/OpenBLAS oracle PORT of the reference '
                                         '(oracle/gccnmf_oracle.py; its angular-spectrum and score contractions are GEMM restatements, '
                                         'so it is FASTER than the reference code): warm-up, then best run per BLAS thread count, best count '
                                         'reported (%.1f s per run).  The reference checkout cannot travel with the repository; '
                                         "`reference_on_gpu_box` is the kept record of its unmodified functions timed on a GPU box's host cores "
                                         '(scripts/time_reference_cpu.py, checkout staged for that one call)' % (B, g.T, dt),
                               'host_cpus': os.cpu_count(),
                               'frames_per_s_by_blas_threads': {str(k): g.T / v for k, v in sorted(sweep.items())},
                               'all_cores': {'value': g.T / dt_all, 'cores': int(threads), 'runs_s': [v[0] for v in runs],
                                             'how': 'default OpenBLAS thread pool, best of 3 after one warm-up (SURVEY 8d)'},
                               'single_thread': {'value': g.T / sweep[1], 'unit': 'frames/s', 'cores': 1, 'seconds': sweep[1],
                                                 'how': 'threadpoolctl.threadpool_limits(1) around the same call (one BLAS thread)'} if 1 in sweep else None}
        rec = os.path.join(REPO, 'profiles', 'reference_cpu_on_gpu_box.json')
        if os.path.exists(rec) and K == 1024 and iters == 100 and a.hop == 256 and a.seconds == 10.0:
            r0 = json.load(open(rec))
            out['cpu_baseline']['reference_on_gpu_box'] = {
                'frames_per_s': r0['frames_per_s'], 'nmf_only_frames_per_s': r0['nmf_only_frames_per_s'], 'host_cpus': r0['host_cpus'],
                'blas_threads': max(t['num_threads'] for t in r0['thread_pools']) if r0.get('thread_pools') else None,
                'best_frames_per_s': r0.get('best_frames_per_s'), 'best_blas_threads': r0.get('best_blas_threads'),
                'recorded': r0.get('recorded', 'round 3'),
                'source': 'profiles/reference_cpu_on_gpu_box.json (same file 0, same parameters; the unmodified reference cannot travel with the '
                          'repository, so it is timed in a builder session with the checkout staged, not in this run)'}
        y0 = e.y[0].cpu().numpy()
        out['gpu_vs_cpu_waveform_rms'] = float(np.sqrt(np.mean((y0.astype(np.float64) - r['y']) ** 2)))
        out['gpu_vs_cpu_tdoa_equal'] = bool(e.get_tdoa_indexes()[0].tolist() == r['idx'])

    if rank == 0 and world == 1 and 'roofline' in out and not slabs and extras and not a.no_live_traffic:
        # LAST, with every other number already in `out` and this process idle on the device: the kernel's HBM traffic from the counters
        torch.cuda.synchronize()
        rec, note = live_traffic(a, chained='k3_alone' in out['roofline'])
        if rec:
            out['roofline']['traffic_recorded'] = out['roofline']['traffic']
            out['roofline']['traffic'] = rec['hbm_bytes_per_launch']
            out['roofline']['traffic_source'] = note
            out['roofline']['traffic_live'] = rec
        else:
            out['roofline']['traffic_live'] = {'skipped': note}
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        barrier()                      # rank 0's extra measurements are done: every rank leaves the group together
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
