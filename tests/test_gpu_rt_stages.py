"""-m gpu: every stage of the real-time block call (csrc/rt.hip: eleven kernels behind gccnmf_rt_process_block_ll) element-wise against
float64, each from the device's own inputs to that stage (tests/rt_checks.py states the nine rules and derives their bars; the CPU suite
tests/test_rt_checks.py shows they are sound and sensitive).

The call goes straight through the C ABI.  The test builds every buffer itself: outputs are NaN-filled (argmaxTDOA: a sentinel) before the
call, so an element left that way was never written; the window, tables, W, target row, rings and history are the test's own, which lets
it set state the Python classes never produce -- W columns K..Kp-1 near 1e3, steering columns D..Dp-1 that would win the arg-max,
duplicate steering columns, NaN columns in the history, a write position about to wrap.

A cell is one call (two for the coefficient inference: one update, then two on identical inputs) at the smallest shape at which a
mechanism can fail (rt_checks.CELLS names them):
  windows   64 (smallest radix-2 size, F = 33: two idle score waves), 256, 1024 (33 reduction steps per wave: two chunks, ragged second);
            direct sum: 4 (F = 3), 32 (a power of two below 64), 400, 602 (N % 4 = 2, F = 4 x 64 + 46), 4094 (raised dynamic-LDS limit)
  K / Kp    64/64, 33/64, 100/128;   D  32 (one tile), 33 (partial second tile), 65 (second pass), 130 (third pass);   Tc  1, 3, 5 > history
  streaming hop not dividing the window (256 / 100), B = 600 (the shift's second chunk straddles the channel boundary), hop > window
            (gaps no frame covers), out_delay_blocks 1, 2, 7 on both transform paths
  state     an all-zero frame, a silent right channel (both also under coefficient inference), NaN bins inside a live frame, NaN history
            columns, an all-NaN window
  layouts   a bank of 3 (stream 1 separation off, stream 2 localisation off), 1 / 3 / 8 targets, GCC-NONLIN through the 8-word row

The whole file (32 cells) takes 3.6 s on an MI355X (LABBOOK R15), most of it the float64 restatements on the host.
"""
import numpy as np
import pytest

import rt_checks as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

OK = 0
POINTERS = ('block_in', 'block_out', 'in_ring', 'out_ring', 'X', 'Y', 'C', 'HMask', 'argmax', 'tfMask', 'hist', 'hist_pos', 'target', 'gccphat',
            'W', 'cosT', 'sinT', 'window', 'swindow', 'twiddle', 'colsumW', 'Hcoef', 'Rv')
STATE = ('in_ring', 'out_ring', 'hist', 'hist_pos', 'target')
worst = {}


@pytest.fixture(scope='module')
def lib():
    from gcc_nmf_amd import _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib()


def run(lib, c, I):
    """One call on fresh device buffers -> every buffer the call may write, on the host (X, Y, C complex)."""
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in I.items()}
    for k, shape in R.output_shapes(c).items():
        if k == 'argmax':
            d[k] = torch.full(shape, R.SENTINEL_I, dtype=torch.int32, device='cuda')
        else:
            d[k] = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    rc = lib.gccnmf_rt_process_block_ll(*[d[k].data_ptr() for k in POINTERS], c.N, c.hop, c.B, c.K, c.Kp, c.D, c.Dp, c.Lh, c.mode, c.sep, c.loc,
                                        c.L, c.bits(), c.nH, c.od, torch.cuda.current_stream().cuda_stream)
    assert rc == OK, rc
    torch.cuda.synchronize()
    O = {k: d[k].cpu().numpy() for k in tuple(R.output_shapes(c)) + STATE}
    for k in ('X', 'Y', 'C'):
        O[k] = R.cplx(O[k])
    for k in POINTERS:                                          # the call's inputs proper are read-only
        if k not in O:
            assert np.array_equal(d[k].cpu().numpy().view(np.uint32), np.ascontiguousarray(I[k]).view(np.uint32)), k + ' was written'
    return O


def note(c, sh):
    print(c.name, sorted(sh.items()))
    for k, v in sh.items():
        if k not in ('decided', 'tie cells', 'multi agree'):
            worst[k] = max(worst.get(k, 0.0), v)
    if 'decided' in sh and c.decided:
        assert sh['decided'] >= 0.9, sh                         # rule 4 is not vacuous on the device's own coherence either
    if c.ties and 'tie cells' in sh:
        assert sh['tie cells'] >= 10, sh                        # the duplicate columns do win: the tie order was exercised
    assert sh.get('exp_units', 0) <= R.RT_EXP_U


@pytest.mark.parametrize('c', R.CELLS, ids=repr)
def test_every_stage_of_one_call(lib, c):
    I = R.make_inputs(c)
    O = run(lib, c, I)
    note(c, R.check_call(c, I, O))


@pytest.mark.parametrize('c', R.INFERENCE_CELLS, ids=repr)
def test_coefficient_inference_update_by_update(lib, c):
    """numHUpdates = 1, then 2 on identical inputs: the second run's Rv and Hcoef are checked from the first run's Hcoef (rule 7)."""
    I = R.make_inputs(c)
    O1 = run(lib, c, I)
    c2 = c.with_updates(c.nH + 1)
    O2 = run(lib, c2, I)
    for k in ('X', 'C', 'HMask'):                               # deterministic: the same bits up to the coefficient updates
        assert np.array_equal(O1[k].view(np.uint32), O2[k].view(np.uint32)), k
    note(c, R.check_call(c, I, O1))
    note(c2, R.check_call(c2, I, O2, first=O1))


def test_report_the_largest_share_of_every_bar():
    """Not a check of its own: prints what the cells above used (run the file as a whole)."""
    print('largest share of each bar over all cells:', sorted((k, round(v, 4)) for k, v in worst.items()))
