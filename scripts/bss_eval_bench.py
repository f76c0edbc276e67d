"""Scoring on the device, timed stage by stage -> profiles/r22a_bss_eval_bench.json.

Workload: 64 files, J = 3 sources, 10 s at 16 kHz, stereo, L = 512 taps -- all 3 x 3 pairs, as bss_eval_images scores them.  Each stage
of gcc_nmf_amd.evaluation.pair_energies (correlations, Toeplitz expansion, solves, coefficient assembly, projections, energies) is timed
with device events over every chunk of files, after a warm-up run, over several repeats; the end-to-end time is a host clock around a run
that ends in a synchronise.  The float64 restatement (tests/bss_eval_restatement.py) is timed on ONE file on at most 16 CPU threads: what a
user would otherwise run.

    python scripts/bss_eval_bench.py [--files 64] [--seconds 10] [--repeats 3] [--skip-cpu] [--out profiles/r22a_bss_eval_bench.json]

Needs a ROCm device (HipLibraryError without one: nothing is timed on a fallback)."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '16')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import numpy as np          # noqa: E402
import torch                # noqa: E402

FP64_PEAK_TFLOPS = 78.6     # the public vector / matrix FP64 figure of the MI355X; not measured here


def make_batch(files, J, n, seed=0):
    """(s, e) float32 (files, J, 2, n): white sources through 4-tap FIRs per channel + an independent white component of 0.3 per channel
    image; estimates = image + 0.2 x its delayed copy + 0.1 x the other images + white artefacts at -40 dB."""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal((files, J, 1, n + 3)).astype(np.float32)
    h = (rng.standard_normal((files, J, 2, 4)) * np.array([1.0, 0.5, 0.25, 0.125])).astype(np.float32)
    s = sum(h[..., k:k + 1] * src[..., 3 - k:3 - k + n] for k in range(4)) + 0.3 * rng.standard_normal((files, J, 2, n)).astype(np.float32)
    e = s + 0.2 * np.roll(s, 1, axis=-1) + 0.1 * (s.sum(axis=1, keepdims=True) - s)
    e = e + 0.01 * s.std(axis=-1, keepdims=True) * rng.standard_normal(s.shape).astype(np.float32)
    return s.astype(np.float32), e.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--sources', type=int, default=3)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--filter-length', type=int, default=512)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--skip-cpu', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r22a_bss_eval_bench.json'))
    a = ap.parse_args()
    from gcc_nmf_amd import _eval, evaluation
    _eval.require_device()
    B, J, C, L, n = a.files, a.sources, 2, a.filter_length, int(round(a.seconds * 16000))
    s, e = make_batch(B, J, n)
    pairs = [(j, i) for j in range(J) for i in range(J)]
    dev = torch.device('cuda:0')
    rec = dict(workload=dict(files=B, sources=J, channels=C, samples=n, filterLength=L, pairs=len(pairs)),
               device=torch.cuda.get_device_name(0), torch=torch.__version__, repeats=a.repeats,
               gram_cap_bytes=evaluation.GRAM_CAP_BYTES, files_per_chunk=evaluation.files_per_chunk(J, C, L))
    with torch.cuda.device(dev):
        S, E = torch.from_numpy(s).to(dev), torch.from_numpy(e).to(dev)
        evaluation.pair_energies(S, E, L, pairs)                    # warm-up: code objects, solver handles, allocator
        torch.cuda.synchronize()
        stages, wall = {}, []
        for _ in range(a.repeats):
            timings = {}
            t0 = time.perf_counter()
            energies, status = evaluation.pair_energies(S, E, L, pairs, timings=timings)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            for name, events in timings.items():
                stages.setdefault(name, []).append(sum(x.elapsed_time(y) for x, y in events))
    assert not status.any()
    sdr, isr, sir, sar = evaluation.criteria_from_energies(energies.reshape(B, J, J, 7))
    rec['stage_ms'] = dict((k, dict(min=min(v), median=float(np.median(v)), max=max(v))) for k, v in stages.items())
    rec['end_to_end_ms'] = dict(min=min(wall), median=float(np.median(wall)), max=max(wall))
    rec['diagonal_db_file0'] = dict(sdr=np.diag(sdr[0]).tolist(), isr=np.diag(isr[0]).tolist(), sir=np.diag(sir[0]).tolist(), sar=np.diag(sar[0]).tolist())
    # the floor of the two kernels, derived from the shapes: what the definition needs, and what the launches execute
    JC, lags, M = J * C, 2 * L - 1, n + L - 1
    need_corr = (JC * (JC + 1) // 2 * lags + JC * JC * L) * n                 # G: a <= b, every lag; d: lags >= 0 only
    done_corr = (JC * (JC + 1) // 2 + JC * JC) * lags * n                     # the second call also sums the negative lags
    proj = (JC * JC * L + len(pairs) * C * C * L) * M
    floor_ms = 2.0 * (need_corr + proj) * B / (FP64_PEAK_TFLOPS * 1e12) * 1e3
    kernels_ms = rec['stage_ms']['correlations']['median'] + rec['stage_ms']['projections']['median']
    rec['floor'] = dict(correlation_gmac_per_file_needed=need_corr / 1e9, correlation_gmac_per_file_executed=done_corr / 1e9,
                        projection_gmac_per_file=proj / 1e9, fp64_peak_tflops_public_not_measured=FP64_PEAK_TFLOPS,
                        floor_ms=floor_ms, kernels_ms=kernels_ms, fraction_of_floor=floor_ms / kernels_ms,
                        correlations_tflops_executed=2.0 * done_corr * B / (rec['stage_ms']['correlations']['median'] * 1e-3) / 1e12,
                        projections_tflops=2.0 * proj * B / (rec['stage_ms']['projections']['median'] * 1e-3) / 1e12)
    rec['mfma_form'] = 'not built: only the VALU float64 form of the correlation kernel exists, so no MFMA timing was taken'
    if not a.skip_cpu:
        import bss_eval_restatement as R
        t0 = time.perf_counter()
        want = R.all_pairs(s[0], e[0], L, 'cholesky')
        rec['cpu_restatement_one_file_s'] = time.perf_counter() - t0
        rec['cpu_threads'] = int(os.environ['OMP_NUM_THREADS'])
        rec['cond_G_file0'] = want[4]
        rec['largest_db_difference_file0'] = float(max(np.abs(x[0] - y).max() for x, y in zip((sdr, isr, sir, sar), want[:4])))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(rec, sort_keys=True))


if __name__ == '__main__':
    main()
