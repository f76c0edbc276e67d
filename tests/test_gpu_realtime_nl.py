"""-m gpu: GCC-NONLIN localisation in the real-time path (word 6 of the target row, csrc/rt.hip rt_localize_kernel) against the NumPy
restatement in tests/angular_nl_restatement.py: gccPHAT = nanmean_f phi on the device's own coherence, the tracked index and multiple
mode's indexes, graph replay, and the bank's per-stream switch.

The bar on gccPHAT (values in [0, 1]) is measured like the offline one: 4 x the largest distance of a float32 NumPy evaluation of the
same formulas (the processor's own float32 tables) from the float64 restatement; measured 2.2e-6 .. 2.6e-6 on the streams below, a bar
of 0.9e-5 .. 1.0e-5, the device at 2.2e-6 .. 2.5e-6.  Indexes are compared on the blocks whose restated window mean separates every
decision by more than 100 bars (25 and 21 of the 28 blocks after the warm-up here, 27 and 21 with the host framing of
tests/test_angular_nl_host.py; the stream is not stationary, so a window mean passes through ties now and then)."""
import warnings

import numpy as np
import pytest

import angular_nl_restatement as NL
import test_angular_nl_host as H
from oracle import rt_oracle as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

FS, SPACING, ALPHA = H.FS, H.SPACING, H.ALPHA
# name: (windowSize, hopSize, blockSize, K, D, numHUpdates, asymmetric synthesis size or None, outputDelayBlocks)
CONFIGS = {'config5': (512, 64, 64, 1024, 64, 2, 128, 1), 'direct_sum_ws400': (400, 100, 100, 96, 48, 0, None, 2)}


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        yield


def processor(name, nl=True, alpha=ALPHA, mode=2, N=3, loc=True, L=H.L_WINDOW):
    from gcc_nmf_amd.realtime import GCCNMFProcessor, asymmetricWindows
    ws, hop, B, K, D, nh, syn, _ = CONFIGS[name]
    kw = {}
    if syn:
        a, sy = asymmetricWindows(ws, syn)
        kw = dict(analysisWindow=a, synthesisWindow=sy)
    W = R.make_rt_dictionary(3, ws // 2 + 1, K)
    p = GCCNMFProcessor(FS, ws, B // hop, {'Pretrained': {K: W}}, 'Pretrained', K, nh, SPACING, loc, L, numTDOAs=D, numSources=N,
                        gccPHATNLEnabled=nl, gccPHATNLAlpha=alpha, **kw)
    p.targetMode = mode
    p.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
    return p


def stream(p, name, use_graph=True):
    from gcc_nmf_amd.realtime import StreamingGCCNMF
    ws, hop, B, K, D, nh, syn, delay = CONFIGS[name]
    return StreamingGCCNMF(p, hop, B, outputDelayBlocks=delay, use_graph=use_graph)


def mixture(name, seed=0, n_blocks=H.N_BLOCKS):
    from gcc_nmf_amd.synthetic import synthetic_mixture
    return synthetic_mixture(seed, numSamples=n_blocks * CONFIGS[name][2], sampleRate=FS, delays=H.DELAYS)


def blk(x, b, B):
    return x[..., b * B:(b + 1) * B]


def tables_of(p):
    """(exact float64 cos / sin of the processor's float32 grids, the float32 tables the device reads)."""
    cos64, sin64 = NL.tables(p.frequenciesInHz, p.hypothesisTDOAs)
    return cos64, sin64, p.expJOmegaTau.real.astype(np.float32), (-p.expJOmegaTau.imag).astype(np.float32)


@pytest.mark.parametrize('alpha', [0.5, 2.0, 8.0])
@pytest.mark.parametrize('name', list(CONFIGS))
def test_gccphat_of_a_given_coherence(name, alpha):
    """The localisation kernel alone (frames mode, localize='only') on a coherence written into the processor's buffer: random unit-modulus bins, a
    tenth of them NaN (zero magnitude: skipped, not counted), one frame with an exact grid delay, one frame of NaN only."""
    ws, hop, B, K, D, nh, syn, _ = CONFIGS[name]
    from gcc_nmf_amd.realtime import GCCNMFProcessor
    W = R.make_rt_dictionary(3, ws // 2 + 1, 64)
    Tc = 4
    p = GCCNMFProcessor(FS, ws, Tc, {'P': {64: W}}, 'P', 64, 0, SPACING, False, 6, numTDOAs=D, gccPHATNLEnabled=True, gccPHATNLAlpha=alpha)
    F = ws // 2 + 1
    rng = np.random.RandomState(int(alpha * 10) + ws)
    C = np.exp(1j * rng.uniform(-np.pi, np.pi, (F, Tc))).astype(np.complex64)
    C[rng.rand(F, Tc) < 0.1] = np.nan
    C[:, 1] = np.exp(2j * np.pi * p.frequenciesInHz.astype(np.float64) * float(p.hypothesisTDOAs[D // 3])).astype(np.complex64)
    C[:, 3] = np.nan
    p.dC.copy_(torch.view_as_real(torch.from_numpy(C)).to(p.device))
    p._call(None, None, p.dFramesIn, p.dFramesOut, ws, Tc * ws, frames=True, localize='only')
    torch.cuda.synchronize()
    got = p.dGccPhat.cpu().numpy().astype(np.float64)
    cos64, sin64, cos32, sin32 = tables_of(p)
    g64 = NL.gccphat_nl(C, cos64, sin64, alpha)
    g32 = NL.gccphat_nl(C, cos32, sin32, alpha, np.float32).astype(np.float64)
    err = float(np.nanmax(np.abs(g32 - g64)))
    bar = NL.BAR_FACTOR * err
    dev = float(np.nanmax(np.abs(got - g64)))
    print('%s alpha %g: float32 NumPy error %.3g -> bar %.3g, device %.3g' % (name, alpha, err, bar, dev))
    assert np.isnan(got[:, 3]).all() and np.isfinite(got[:, :3]).all() and np.isnan(g64[:, 3]).all()
    assert dev <= bar and np.all(got[:, :3] >= 0) and np.all(got[:, :3] <= 1 + 1e-6)
    assert int(np.argmax(got[:, 1])) == D // 3 and got[D // 3, 1] > 1 - alpha * 1e-3
    # a counted NaN bin would scale the column by (F - nNaN) / F ~ 0.9: far outside the bar
    assert abs(np.nanmean(got[:, 0] / g64[:, 0]) - 1) < 1e-4
    # the same coherence with NL off is plain PHAT, the bits of a processor that never heard of NL
    outs = []
    for kw in (dict(gccPHATNLEnabled=False, gccPHATNLAlpha=alpha), {}):
        q = GCCNMFProcessor(FS, ws, Tc, {'P': {64: W}}, 'P', 64, 0, SPACING, False, 6, numTDOAs=D, **kw)
        q.dC.copy_(torch.view_as_real(torch.from_numpy(C)).to(q.device))
        q._call(None, None, q.dFramesIn, q.dFramesOut, ws, Tc * ws, frames=True, localize='only')
        outs.append(q.dGccPhat.cpu().numpy())
    assert np.array_equal(outs[0], outs[1], equal_nan=True)
    phat = np.nanmean((C[:, :, None] * p.expJOmegaTau[:, None]).real.astype(np.float64), axis=0).T
    assert np.nanmax(np.abs(outs[0] - phat)) < 1e-5


@pytest.mark.parametrize('name', list(CONFIGS))
def test_stream_gccphat_and_tracked_indexes(name):
    """Check 6 on the stream: every block's gccPHAT against the restatement on the device's own coherence; the tracked index (window
    function mode) and multiple mode's three indexes equal the restatement's wherever it separates them by more than 100 bars."""
    ws, hop, B, K, D, nh, syn, _ = CONFIGS[name]
    x = mixture(name)
    single, multi = processor(name, mode=2), processor(name, mode=1, N=3)
    ss, sm = stream(single, name), stream(multi, name)
    cos64, sin64, cos32, sin32 = tables_of(single)
    tracker = NL.StreamTracker(D, single.numTDOAHistory, H.L_WINDOW)
    worst_err, worst_dev, rows = 0.0, 0.0, []
    for b in range(H.N_BLOCKS):
        ss.process_block(blk(x, b, B))
        ym = sm.process_block(blk(x, b, B))
        assert ym.shape == (3, 2, B)
        it = single.intermediates()
        C, got = it['C'], it['gccPHAT'].astype(np.float64)
        assert np.array_equal(got, multi.intermediates()['gccPHAT'].astype(np.float64), equal_nan=True)
        g64 = NL.gccphat_nl(C, cos64, sin64, ALPHA)
        wm = tracker.push(g64)
        if not np.isfinite(g64).all():
            assert np.array_equal(np.isnan(got), np.isnan(g64))
            continue
        g32 = NL.gccphat_nl(C, cos32, sin32, ALPHA, np.float32).astype(np.float64)
        worst_err = max(worst_err, float(np.abs(g32 - g64).max()))
        worst_dev = max(worst_dev, float(np.abs(got - g64).max()))
        rows.append((b, wm, it['targetTDOAIndex'], multi.targetTDOAIndexes))
    bar = NL.BAR_FACTOR * worst_err
    print('%s: float32 NumPy error %.3g -> bar %.3g, device %.3g' % (name, worst_err, bar, worst_dev))
    assert 0 < worst_dev <= bar
    checked = 0
    for b, wm, idx1, idxN in rows:
        if b < H.WARMUP:
            continue
        want = H.separated(wm, bar)
        if want is None:
            continue
        checked += 1
        assert int(idx1) == want[0], (b, idx1, want)
        assert [int(i) for i in idxN] == want[1], (b, idxN, want)
    print('%s: indexes compared on %d of %d blocks' % (name, checked, H.N_BLOCKS - H.WARMUP))
    assert checked >= (H.N_BLOCKS - H.WARMUP) // 2


def test_boxcar_mode_tracks_the_same_index():
    name = 'config5'
    B = CONFIGS[name][2]
    x = mixture(name, n_blocks=40)
    a, b_ = processor(name, mode=0), processor(name, mode=2)
    sa, sb = stream(a, name), stream(b_, name)
    for b in range(40):
        sa.process_block(blk(x, b, B))
        sb.process_block(blk(x, b, B))
        assert a.targetTDOAIndex == b_.targetTDOAIndex
    assert np.array_equal(a.intermediates()['gccPHAT'], b_.intermediates()['gccPHAT'])


@pytest.mark.parametrize('mode,N', [(2, 1), (1, 3)])
def test_graph_replay_equals_direct_launches(mode, N):
    name = 'config5'
    B = CONFIGS[name][2]
    x = mixture(name, seed=6, n_blocks=30)
    outs = []
    for use_graph in (False, True):
        p = processor(name, mode=mode, N=N)
        st = stream(p, name, use_graph=use_graph)
        ys = np.stack([st.process_block(blk(x, b, B)) for b in range(30)])
        assert (st._graph is not None) == use_graph and st.capture_error is None
        outs.append((ys, p.dHist.cpu().numpy(), p.targetTDOAIndexes if mode == 1 else p.targetTDOAIndex))
    for a, b in zip(*outs):
        assert np.array_equal(a, b, equal_nan=True)


def test_reset_applies_new_settings():
    """Like the reference (gccNMFProcessor.py:131-132), a new gccPHATNLEnabled / gccPHATNLAlpha takes effect with reset()."""
    name = 'direct_sum_ws400'
    B = CONFIGS[name][2]
    x = mixture(name, n_blocks=12)
    p = processor(name, nl=False)
    ref_off, ref_on = processor(name, nl=False), processor(name, nl=True, alpha=0.5)

    def run(q):
        st = stream(q, name)
        for b in range(12):
            st.process_block(blk(x, b, B))
        return q.dHist.cpu().numpy()
    h_off, h_on = run(ref_off), run(ref_on)
    p.gccPHATNLEnabled, p.gccPHATNLAlpha = True, 0.5
    assert np.array_equal(run(p), h_off, equal_nan=True)             # not before reset()
    p.reset()
    p.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
    assert np.array_equal(run(p), h_on, equal_nan=True) and not np.array_equal(h_on, h_off, equal_nan=True)
    p.gccPHATNLAlpha = -1.0
    with pytest.raises(ValueError):
        p.reset()


@pytest.mark.parametrize('mode,N', [(2, 1), (1, 2)])
def test_bank_streams_with_and_without_nl(mode, N):
    """A bank stream with NL on equals a StreamingGCCNMF of its own bit for bit, while its neighbour with NL off equals today's output
    (a processor that was never given the keywords) bit for bit; stream 2 takes another alpha, stream 3 switches over half way."""
    from gcc_nmf_amd.realtime import StreamingGCCNMFBank
    name = 'config5'
    ws, hop, B, K, D, nh, syn, delay = CONFIGS[name]
    S, n_blocks, r = 4, 24, 12
    x = np.stack([mixture(name, seed=10 + s, n_blocks=n_blocks) for s in range(S)])
    bk = StreamingGCCNMFBank(processor(name, nl=False, mode=mode, N=N), S, hop, B, outputDelayBlocks=delay)
    bk.setGCCPHATNL(0, True, ALPHA)
    bk.setGCCPHATNL(2, True, 0.5)
    own = [stream(processor(name, nl=True, mode=mode, N=N), name), None, stream(processor(name, nl=True, alpha=0.5, mode=mode, N=N), name),
           None]
    from gcc_nmf_amd.realtime import GCCNMFProcessor, asymmetricWindows
    a, sy = asymmetricWindows(ws, syn)
    for s in (1, 3):                                     # today's processor: constructed without the new keywords
        q = GCCNMFProcessor(FS, ws, B // hop, {'Pretrained': {K: R.make_rt_dictionary(3, ws // 2 + 1, K)}}, 'Pretrained', K, nh, SPACING,
                            True, H.L_WINDOW, numTDOAs=D, numSources=N, analysisWindow=a, synthesisWindow=sy)
        q.targetMode = mode
        q.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
        own[s] = stream(q, name)
    late = processor(name, nl=True, mode=mode, N=N)      # stream 3 after its restart with NL on
    late_stream = stream(late, name)
    for b in range(n_blocks):
        if b == r:
            bk.reset_stream(3)
            bk.setGCCPHATNL(3, True, ALPHA)
        yb = bk.process_block(blk(x, b, B))
        idx = bk.targetTDOAIndexes
        for s in range(S):
            st = late_stream if (s == 3 and b >= r) else own[s]
            assert np.array_equal(yb[s], st.process_block(blk(x[s], b, B))), (b, s)
            want = st.p.targetTDOAIndexes if mode == 1 else st.p.targetTDOAIndex
            assert np.array_equal(idx[s], want), (b, s)
    hist = bk.dHist.cpu().numpy()
    assert np.array_equal(hist[0], own[0].p.dHist.cpu().numpy(), equal_nan=True)
    assert np.array_equal(hist[1], own[1].p.dHist.cpu().numpy(), equal_nan=True)
    assert not np.array_equal(hist[0], hist[1], equal_nan=True)
    with pytest.raises(ValueError):
        bk.setGCCPHATNL(0, True, 0.0)
