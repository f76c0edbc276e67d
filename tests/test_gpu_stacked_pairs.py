"""-m gpu: gccnmf_angular_spectrogram, gccnmf_pick_tdoa_peaks and gccnmf_target_scores_masks through the C ABI at the shapes
GCCNMFArrayEngine hands them: F = Fs = (P - 1) Fp + F bins of P stacked microphone pairs, zero rows between the pair blocks inside both
reductions.  The method is that of tests/test_gpu_gcc_stages.py (host-built float32 inputs, NaN-filled outputs and workspaces, the scores a
second time over a workspace of other garbage, the same bits); cells, launch rule, inputs and checks are tests/stacked_pairs.py, which
tests/test_array_host.py runs on the host with mistakes planted.

The kernel a launch reaches is decided by the channel count: the angular reduction 2 P Fp and the scores reduction Fs (- 1 with a k-tail)
cross the ring kernel's limit of 4096 between M = 8 at n_fft = 64 and M = 8 at n_fft = 256.  CELLS names the kernel of each stage, and the
rule is restated beside it so that a cell that stops meaning what it says fails.  The largest cell (M = 8, n_fft = 4096: grid extent 57792
of the 65535 allowed, reductions 57776 and 115584) allocates about 30 MB per buffer."""
import numpy as np
import pytest

import stacked_pairs as SP
from test_gpu_gcc_stages import GARBAGE, geometry, nan_like, ptr, stream, tuning

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def lib():
    from gcc_nmf_amd import _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib()


def run_calls(lib, files, M, F, D, S, K, T, trig):
    """The three calls on a batch of host files -> one dict per file, as stacked_pairs.checks() reads it."""
    P, Fp, Fs = SP.shapes(M, F)
    g = geometry(Fs, T, K, D)
    assert g.Fp == P * Fp, 'the padded pitch of the stacked bins is P Fp'
    B = len(files)
    ops = [SP.stacked_operands(f, Fp, g.Kp, g.Tp) for f in files]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    CC, Ws = d(np.stack([o[0] for o in ops])), d(np.stack([o[1] for o in ops]))
    tdoa = d(np.stack([f['tdoa'] for f in files]).astype(np.int32))
    s = stream()
    ang, mean = nan_like((B, g.Dp, g.Tp)), nan_like((B, g.Dp), torch.float64)
    assert lib.gccnmf_angular_spectrogram(ptr(CC), ptr(trig), Fs, T, D, B, ptr(ang), ptr(mean), s) == 0
    idx, status = torch.full((B, S), -7, dtype=torch.int32, device='cuda'), torch.full((B,), -7, dtype=torch.int32, device='cuda')
    assert lib.gccnmf_pick_tdoa_peaks(ptr(mean), D, g.Dp, S, B, ptr(idx), ptr(status), s) == 0
    nws = lib.gccnmf_scores_workspace_floats(Fs, T, S, B)
    assert nws == B * g.Fp * S * g.Tp
    runs = []
    for fill in (float('nan'), GARBAGE):
        ws = torch.full((nws,), fill, dtype=torch.float32, device='cuda')
        scores = nan_like((B, g.Kp, S * g.Tp))
        am = torch.full((B, g.Kp, g.Tp), 0xAB, dtype=torch.uint8, device='cuda')
        assert lib.gccnmf_target_scores_masks(ptr(CC), ptr(trig), ptr(tdoa), ptr(Ws), Fs, T, K, D, S, B, ptr(ws), ptr(scores), ptr(am),
                                              s) == 0
        runs.append((ws, scores, am))
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()
    assert np.array_equal(host(runs[1][1]), host(runs[0][1]), equal_nan=True), 'scores depend on the workspace'
    assert np.array_equal(host(runs[1][2]), host(runs[0][2])), 'arg-max depends on the workspace'
    assert np.array_equal(host(runs[1][0]), host(runs[0][0]), equal_nan=True), 'the whole workspace is written'
    r = dict(ang=host(ang), mean=host(mean), idx=host(idx), status=host(status), P=host(runs[0][0]).reshape(B, g.Fp, S, g.Tp),
             scores=host(runs[0][1]).reshape(B, g.Kp, S, g.Tp), argmax=host(runs[0][2]))
    return [dict((k, v[b]) for k, v in r.items()) for b in range(B)]


@pytest.mark.parametrize('cell', list(SP.CELLS), ids=['M%d-F%d-D%d-S%d-K%d-T%d-b%d-tile%d-dma%d' % c for c in SP.CELLS])
def test_stacked_calls_against_float64(lib, cell):
    from gcc_nmf_amd.array import array_steering_tables
    M, F, D, S, K, T, batch, key2, key3 = cell
    assert SP.kernels(*cell) == SP.CELLS[cell], 'the cell no longer reaches the kernels it is named for'
    P, Fp, Fs = SP.shapes(M, F)
    trig = torch.from_numpy(array_steering_tables(SP.frequencies(F), SP.pair_tdoas(M, D), Fp, SP.rup(D, 64))).cuda()
    files = [SP.host_file(M, F, D, S, K, T, 1000 * F + 100 * M + 10 * b + K) for b in range(batch)]
    with tuning(lib, key2, key3):
        outs = run_calls(lib, files, M, F, D, S, K, T, trig)
        alone = [run_calls(lib, [files[b]], M, F, D, S, K, T, trig)[0] for b in sorted({0, batch - 1})] if batch > 1 else []
    print('M = %d, F = %d: Fs = %d, angular reduction %d, scores reduction %d: %s' % (M, F, Fs, 2 * P * Fp, Fs - (Fs % 16 == 1), SP.CELLS[cell]))
    for b in range(batch):
        for name, check in SP.checks(outs[b], files[b], M, F, D, S, K, T, what='file %d: ' % b):
            check()
    # a file's result does not depend on the batch it rides in (both batches run under a forced tile policy: the same kernels)
    assert key2 != 0 or batch == 1
    for b, a in zip(sorted({0, batch - 1}), alone):
        for name, check in SP.checks(a, files[b], M, F, D, S, K, T, what='file %d alone: ' % b):
            check()
        for name in ('ang', 'mean', 'idx', 'status', 'P', 'scores', 'argmax'):
            assert np.array_equal(outs[b][name], a[name], equal_nan=True), (name, b)
