"""-m gpu: the online spatial filter of the real-time block call (csrc/rt_spatial.hip, GCCNMF_RT_SEPARATION_SPATIAL) element-wise against its
float64 restatement (tests/rt_spatial_restatement.py), through the C ABI.

Every cell of tests/rt_spatial_cells.py is an rt_checks.Cell (its inputs from rt_checks.make_inputs) with word 7 of the target rows set, a
prior state of the test's own behind the history images of `hist`, and runs twice on identical inputs:

  run 1  without the bit: passes rt_checks.check_call as the call always did, and leaves the state region (and the gap in front of it)
         bit for bit
  run 2  with the bit: every buffer but Y, out_ring, block_out and the state is bit-identical to run 1.  From run 1's Y (= tfMask . X bit
         for bit, rule 6) and X and the prior state the restatement gives run 2's Y and new state: EVERY element is compared, except
         where the restatement is non-finite -- there the device must be non-finite too.  out_ring: rt_checks.synthesis64 of run 2's Y
         under rule 8's bar; block_out = its out_ring slice bit for bit.

The bar is the project's rule: BAR_FACTOR (4) x the largest distance of the float32 NumPy evaluation of the recursion from the float64 one
on that cell's own Y, X and state -- Y relative to max|X|, the state relative to its largest entry.  tests/test_rt_spatial_host.py shows
on the CPU that this bar stays below 1e-4 outside the rank-deficient cell (an identity covariance fails) and sees four planted mistakes.

rt_checks.check_call does not take non-finite input (its rule 2 reads a NaN in X as "not written"), so the cell with a NaN sample passes
check_call on the same inputs without that sample, in a call of its own; its runs 1 and 2 are compared as for every other cell, which
includes Y = tfMask . X of run 1 where the inputs are finite.

The bank cell: stream 0 filters and is bit-equal to the single-stream call on its images; stream 1 has its separation off and stream 2 a
word 7 of 0: their state is bit-untouched and everything they write is as in run 1.
"""
import numpy as np
import pytest

import fft_checks as K
import rt_checks as R
import rt_spatial_cells as SC
import rt_spatial_restatement as RS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

OK = 0
POINTERS = ('block_in', 'block_out', 'in_ring', 'out_ring', 'X', 'Y', 'C', 'HMask', 'argmax', 'tfMask', 'hist', 'hist_pos', 'target', 'gccphat',
            'W', 'cosT', 'sinT', 'window', 'swindow', 'twiddle', 'colsumW', 'Hcoef', 'Rv')
STATE = ('in_ring', 'out_ring', 'hist', 'hist_pos', 'target')
FILTER_WRITES = ('Y', 'out_ring', 'block_out', 'spatial')
table = []


@pytest.fixture(scope='module')
def lib():
    from gcc_nmf_amd import _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib()


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.complex64 else np.uint32)


def run(lib, sc, I, spatial):
    """One call on fresh device buffers -> every buffer the call may write, on the host (X, Y, C complex), 'spatial' (S, NC, F, 4) and
    'gap' (the floats between the histories and the state) among them."""
    c = sc.c
    buf, off = SC.hist_buffer(sc, I)
    host = {k: v for k, v in I.items() if k != 'spatial'}
    host['hist'] = buf
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}
    for k, shape in R.output_shapes(c).items():
        if k == 'argmax':
            d[k] = torch.full(shape, R.SENTINEL_I, dtype=torch.int32, device='cuda')
        else:
            d[k] = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    assert d['hist'].data_ptr() % 16 == 0
    sep = (c.sep | SC.SPATIAL) if spatial else c.sep
    rc = lib.gccnmf_rt_process_block_ll(*[d[k].data_ptr() for k in POINTERS], c.N, c.hop, c.B, c.K, c.Kp, c.D, c.Dp, c.Lh, c.mode, sep, c.loc,
                                        c.L, sc.bits(), c.nH, c.od, torch.cuda.current_stream().cuda_stream)
    assert rc == OK, rc
    torch.cuda.synchronize()
    O = {k: d[k].cpu().numpy() for k in tuple(R.output_shapes(c)) + STATE}
    n = I['hist'].size
    O['hist'], O['gap'], O['spatial'] = O['hist'][:n].reshape(I['hist'].shape), O['hist'][n:off], O['hist'][off:].reshape(I['spatial'].shape)
    for k in ('X', 'Y', 'C'):
        O[k] = R.cplx(O[k])
    for k in POINTERS:                                          # the call's inputs proper are read-only
        if k not in O:
            assert np.array_equal(bits_of(d[k].cpu().numpy()), bits_of(host[k])), k + ' was written'
    return O


def same_bits(a, b, what):
    assert np.array_equal(bits_of(a), bits_of(b)), what


def check_synthesis(c, I, s, O2, what):
    """Rule 8 of rt_checks on run 2's Y of stream s (the device's own input to the synthesis)."""
    B, N, Tc = c.B, c.N, c.Tc
    h0 = c.ring - (c.od + 1) * B
    worst = 0.0
    for i in range(c.nM):
        Yi = O2['Y'][s][i]
        live = np.isfinite(Yi).all(axis=(0, 1))                # frames whose spectrum is finite
        fr, fbar = R.synthesis64(c, I, np.where(np.isfinite(Yi), Yi, 0))
        got = O2['out_ring'][s][i]
        if c.frames:
            for ch in range(2):
                g = got[ch].reshape(Tc, N)
                worst = max(worst, K.check_bar(g[live], fr[ch][live], fbar[live], '%s frames out target %d channel %d' % (what, i, ch)))
                assert not np.isfinite(g[~live]).any(), what + ': a non-finite spectrum must give a non-finite frame'
        else:
            assert live.all()
            shifted = np.concatenate([I['out_ring'][s][i][:, B:], np.zeros((2, B), np.float32)], axis=-1)
            acc, bar, pmax = shifted.astype(np.float64), np.zeros(c.ring), np.zeros((2, c.ring))
            for t, st in enumerate(c.starts()):
                acc[:, st:st + N] += fr[:, t]
                bar[st:st + N] += fbar[t]
                pmax = np.maximum(pmax, np.abs(acc))
            for ch in range(2):
                worst = max(worst, K.check_bar(got[ch], acc[ch], bar + Tc * R.U32 * pmax[ch], '%s out_ring target %d channel %d' % (what, i, ch)))
            same_bits(O2['block_out'][s][i], got[:, h0:h0 + B], '%s block_out target %d' % (what, i))
    return worst


def single_stream_of_the_bank(sc, I):
    """The single-stream cell (8-word row) on stream 0's images of a bank cell."""
    c = sc.c
    one = SC.SpatialCell(R.Cell(c.name + ' stream 0 alone', c.N, c.hop, c.B, c.K, c.D, Lh=c.Lh, L=c.L, mode=c.mode, od=c.od, nH=c.nH, row=c.row),
                         tau=sc.tau, state=sc.state)
    I1 = dict(I)
    for k in ('in_ring', 'block_in', 'out_ring', 'hist', 'hist_pos', 'target', 'spatial'):
        I1[k] = np.ascontiguousarray(I[k][:1])
    return one, I1


@pytest.mark.parametrize('sc', SC.CELLS, ids=repr)
def test_the_filter_of_one_call(lib, sc):
    c = sc.c
    I = SC.make_inputs(sc)
    Ic = {k: v for k, v in I.items() if k != 'spatial'}
    O1 = run(lib, sc, I, spatial=False)
    if sc.nan_frame is None:
        R.check_call(c, Ic, {k: v for k, v in O1.items() if k not in ('gap', 'spatial')})
    else:                                                       # check_call takes finite input only: the same call without the NaN sample
        clean = SC.SpatialCell(c, tau=sc.tau, state=sc.state)
        Iclean = SC.make_inputs(clean)
        Oc = run(lib, clean, Iclean, spatial=False)
        R.check_call(c, {k: v for k, v in Iclean.items() if k != 'spatial'}, {k: v for k, v in Oc.items() if k not in ('gap', 'spatial')})
        fin = np.isfinite(O1['X']).all(axis=1, keepdims=True)   # (S, 1, F, Tc)
        assert not fin[..., sc.nan_frame].any() and fin[..., [t for t in range(c.Tc) if t != sc.nan_frame]].all()
        for k in ('X', 'Y', 'C', 'tfMask', 'HMask', 'argmax'):      # the finite frames are the clean call's, bit for bit
            keep = [t for t in range(c.Tc) if t != sc.nan_frame]
            same_bits(O1[k][..., keep], Oc[k][..., keep], k + ' of the finite frames')
    same_bits(O1['spatial'], I['spatial'], 'run 1 wrote the state')
    assert (O1['gap'] == -3.0).all()

    O2 = run(lib, sc, I, spatial=True)
    for k in O1:
        if k not in FILTER_WRITES:
            same_bits(O2[k], O1[k], k + ' differs between the runs')
    for s in range(c.nS):
        what = '%s stream %d' % (sc.name, s)
        if not sc.filtered(s):
            for k in FILTER_WRITES:
                same_bits(O2[k][s], O1[k][s], '%s: %s of a stream that does not filter' % (what, k))
            same_bits(O2['spatial'][s], I['spatial'][s], what + ': state of a stream that does not filter')
            continue
        Y, X = SC.stream_io(sc, O1, s)
        m = RS.measured_bar(Y, X, I['spatial'][s], sc.taus()[s], c.multi)
        dY, dP = RS.distance(O2['Y'][s], O2['spatial'][s], m)
        eq = np.array_equal(bits_of(O2['Y'][s]), bits_of(m['Y32'])) and np.array_equal(bits_of(O2['spatial'][s]), bits_of(m['P32']))
        print('%s: Y float32 error %.3e bar %.3e device %.3e | state float32 error %.3e bar %.3e device %.3e | device == float32 NumPy bit for bit: %s'
              % (what, m['err_Y'], m['bar_Y'], dY, m['err_P'], m['bar_P'], dP, eq))
        table.append((what, m['err_Y'], m['bar_Y'], dY, m['err_P'], m['bar_P'], dP))
        assert dY <= m['bar_Y'], (what, dY, m['bar_Y'])
        assert dP <= m['bar_P'], (what, dP, m['bar_P'])
        if not sc.rank_deficient:
            assert m['bar_Y'] < 1e-4 and m['bar_P'] < 1e-4
        if c.multi and sc.nan_frame is None:                    # consequence: the N outputs add up to the mixture
            assert np.abs(O2['Y'][s].astype(np.complex128).sum(axis=0) - X).max() / m['scale_Y'] <= c.NT * m['bar_Y'] + 2.0 ** -23
        print('%s: synthesis, worst share of rule 8\'s bar %.4f' % (what, check_synthesis(c, Ic, s, O2, what)))
    assert (O2['gap'] == -3.0).all()

    if c.bank:                                                  # stream 0 of the bank = the single-stream call on its images, bit for bit
        one, I1 = single_stream_of_the_bank(sc, I)
        A = run(lib, one, I1, spatial=True)
        for k in A:
            if k != 'gap':
                same_bits(A[k][0], O2[k][0], k + ' of stream 0 differs from the single-stream call')


def test_report_the_error_table():
    """Not a check of its own: the per-cell table (run the file as a whole)."""
    for row in table:
        print('| %s | %.2e | %.2e | %.2e | %.2e | %.2e | %.2e |' % row)
