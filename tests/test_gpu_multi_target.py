"""-m gpu: multiple mode of the real-time path (TARGET_MODE_MULTIPLE, frames_mode bit 20 of gccnmf_rt_process_block_ll): N talkers
separated per stream with one-hot arg-max-over-targets masks, N outputs, N tracked peaks.  Compared with the NumPy restatement in
tests/rt_multi_restatement.py, with itself (partition of unity, N = 1, graph replay, the bank) and with the single-target modes."""
import warnings

import numpy as np
import pytest

from oracle import rt_oracle as R
import rt_multi_restatement as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

FS, SPACING = 16000, 1.0              # 1 m: the synthetic mixture's delays -20 / 3 / 27 samples lie inside the TDOA grid
DELAYS = (-20, 3, 27)
# name: (windowSize, hopSize, blockSize, K, D, numHUpdates, asymmetric synthesis size or None, outputDelayBlocks)
CONFIGS = {
    'reference': (1024, 512, 512, 128, 64, 0, None, 2),
    'config5': (512, 64, 64, 1024, 64, 2, 128, 1),
    'direct_sum_ws400': (400, 100, 100, 96, 48, 0, None, 2),
    'tc4': (512, 64, 256, 128, 48, 1, None, 2),
}


def true_indexes(D):
    """Grid positions (fractional) of the three talkers: delay d samples -> TDOA d / FS on linspace(-maxTDOA, maxTDOA, D)."""
    maxT = SPACING / R.SPEED_OF_SOUND_IN_METRES_PER_SECOND
    return np.array(sorted((d / FS + maxT) / (2 * maxT) * (D - 1) for d in DELAYS))


def fixed_targets(D, N):
    return np.round(true_indexes(D))[:N] if N <= 3 else np.linspace(4, D - 5, N).round()


def mixture(n, seed=0):
    from gcc_nmf_amd.synthetic import synthetic_mixture
    return synthetic_mixture(seed, numSamples=n, sampleRate=FS, delays=DELAYS)


def processor(name, N, loc=False, nh=None, L=6, mode=1):
    from gcc_nmf_amd.realtime import GCCNMFProcessor, asymmetricWindows
    ws, hop, B, K, D, nh0, syn, _ = CONFIGS[name]
    kw = {}
    if syn:
        a, sy = asymmetricWindows(ws, syn)
        kw = dict(analysisWindow=a, synthesisWindow=sy)
    W = R.make_rt_dictionary(3, ws // 2 + 1, K)
    p = GCCNMFProcessor(FS, ws, B // hop, {'Pretrained': {K: W}}, 'Pretrained', K, nh0 if nh is None else nh, SPACING, loc, L,
                        numTDOAs=D, numSources=N, **kw)
    p.targetMode = mode
    p.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
    p.setTargetTDOAIndexes(fixed_targets(D, N))
    return p


def stream(p, name, use_graph=True):
    from gcc_nmf_amd.realtime import StreamingGCCNMF
    ws, hop, B, K, D, nh, syn, delay = CONFIGS[name]
    return StreamingGCCNMF(p, hop, B, outputDelayBlocks=delay, use_graph=use_graph)


def oracle_for(p, name, N, loc=False):
    ws, hop, B, K, D, nh, syn, delay = CONFIGS[name]
    kw = {}
    if syn:
        kw = dict(analysisWindow=p.windowFunction[:, 0], synthesisWindow=p.synthesisWindowFunction[:, 0])
    base = R.GCCNMFProcessorOracle(FS, ws, B // hop, p.W, SPACING, D, localizationEnabled=loc, localizationWindowSize=p.localizationWindowSize,
                                   numHUpdates=p.numHUpdates, **kw)
    return M.MultiTargetOracle(base, p.targetTDOAIndexes), M.MultiOverlapAdd(N, ws, hop, B, delay)


def blk(x, b, B):
    return x[..., b * B:(b + 1) * B]


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)           # nanmean of the all-zero start-up frames
        yield


@pytest.mark.parametrize('name', list(CONFIGS))
@pytest.mark.parametrize('N', [2, 3])
def test_masks_and_outputs_match_the_restatement(name, N):
    """Fixed targets at the talkers' grid positions: one-hot masks exact except near-ties of the target scores; outputs under the
    device's own decisions within the streaming tolerance."""
    B = CONFIGS[name][2]
    n_blocks = 24
    x = mixture(n_blocks * B)
    p = processor(name, N)
    st = stream(p, name)
    ora, ola = oracle_for(p, name, N)
    flips, total, worst = 0, 0, 0.0
    for b in range(n_blocks):
        y = st.process_block(blk(x, b, B))
        assert y.shape == (N, 2, B)
        it = p.intermediates()
        hm = it['HMask']                                             # (N, K, Tc)
        assert set(np.unique(hm)) <= {0.0, 1.0} and np.array_equal(hm.sum(axis=0), np.ones(hm.shape[1:]))
        dev = np.argmax(hm, axis=0)
        yr = ola.processFrames(blk(x, b, B), lambda ws: ora.processFrames(ws, target_override=dev))
        _, _, G = ora.scores(ola.olas[0].windowedSamples)
        dec, gap = ora.decisions(G)
        differ = dec != dev
        assert np.all(gap[differ] < 1e-4), (b, gap[differ])
        flips += int(differ.sum())
        total += dec.size
        worst = max(worst, float(np.abs(y - yr).max()))
    assert flips <= 1e-3 * total, (flips, total)
    assert worst < 2e-4 * np.abs(x).max(), worst
    assert np.isfinite(y).all()


@pytest.mark.parametrize('name,nh', [('reference', 0), ('reference', 2), ('config5', 0), ('config5', 2)])
def test_outputs_are_a_partition_of_the_mixture(name, nh):
    B = CONFIGS[name][2]
    x = mixture(30 * B, seed=2)
    on = stream(processor(name, 3, loc=True, nh=nh), name)
    p_off = processor(name, 3, loc=True, nh=nh)
    p_off.separationEnabled = False
    off = stream(p_off, name)
    worst = 0.0
    for b in range(30):
        y = on.process_block(blk(x, b, B))
        y0 = off.process_block(blk(x, b, B))
        assert np.array_equal(y0[0], y0[1]) and np.array_equal(y0[0], y0[2])       # separation off: the mixture on every output
        worst = max(worst, float(np.abs(y.sum(axis=0) - y0[0]).max()))
    assert worst < 1e-4 * np.abs(x).max(), worst


@pytest.mark.parametrize('name', list(CONFIGS))
def test_one_target_is_the_unmasked_mixture_bit_for_bit(name):
    B = CONFIGS[name][2]
    x = mixture(20 * B, seed=3)
    p1, p0 = processor(name, 1, loc=True), processor(name, 1, loc=True)
    p0.separationEnabled = False
    s1, s0 = stream(p1, name), stream(p0, name)
    for b in range(20):
        y1 = s1.process_block(blk(x, b, B))
        assert y1.shape == (1, 2, B)
        assert np.array_equal(y1, s0.process_block(blk(x, b, B))), b
    it = p1.intermediates()
    assert np.all(it['tfMask'] == 1.0) and np.all(it['HMask'] == 1.0)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_tracked_indexes_follow_the_peak_rule_on_the_device_history(name):
    B, D = CONFIGS[name][2], CONFIGS[name][4]
    N, L = 3, 8
    x = mixture(40 * B, seed=4)
    p = processor(name, N, loc=True, L=L)
    st = stream(p, name)
    prev = p.targetTDOAIndexes
    for b in range(40):
        st.process_block(blk(x, b, B))
        hist, pos = p.dHist.cpu().numpy(), int(p.dHistPos.cpu().numpy()[0])
        want = M.pick_peaks(M.window_mean_f32(hist, pos, L), N, prev)
        got = p.targetTDOAIndexes
        assert np.array_equal(got, want), (b, got, want)
        prev = got


def test_tracked_indexes_settle_on_the_three_talkers():
    name, N, L = 'reference', 3, 24
    B, D = CONFIGS[name][2], CONFIGS[name][4]
    x = mixture(60 * B, seed=0)
    p = processor(name, N, loc=True, L=L)
    p.setTargetTDOAIndexes([10, 30, 50])
    st = stream(p, name)
    true = true_indexes(D)
    for b in range(60):
        st.process_block(blk(x, b, B))
        if b >= L:
            assert np.all(np.abs(p.targetTDOAIndexes - true) <= 1.0), (b, p.targetTDOAIndexes, true)


@pytest.mark.parametrize('name', ['config5', 'reference', 'direct_sum_ws400', 'tc4'])
def test_bank_streams_equal_standalone_multi_streams(name):
    """Per-stream targets; stream 1 tracks nothing, stream 2 is passed through; stream 3 restarts half way."""
    from gcc_nmf_amd.realtime import StreamingGCCNMFBank
    ws, hop, B, K, D, nh, syn, delay = CONFIGS[name]
    S, N, n_blocks, r = 4, 2, 30, 15
    x = np.stack([mixture(n_blocks * B, seed=10 + s) for s in range(S)])
    bk = StreamingGCCNMFBank(processor(name, N, loc=True), S, hop, B, outputDelayBlocks=delay)
    targets = [fixed_targets(D, N), [5, 20], [12, 30], [D // 3, D // 2]]
    sts = []
    for s in range(S):
        p = processor(name, N, loc=(s != 1))
        p.separationEnabled = s != 2
        p.setTargetTDOAIndexes(targets[s])
        bk.setTargetTDOAIndexes(s, targets[s])
        sts.append(stream(p, name))
    bk.setLocalizationEnabled(1, False)
    bk.setSeparationEnabled(2, False)
    fresh = stream(processor(name, N, loc=True), name)
    for b in range(n_blocks):
        if b == r:
            bk.reset_stream(3)
        yb = bk.process_block(blk(x, b, B))
        assert yb.shape == (S, N, 2, B)
        idx = bk.targetTDOAIndexes
        assert idx.shape == (S, N)
        for s in range(S):
            st = fresh if (s == 3 and b >= r) else sts[s]
            assert np.array_equal(yb[s], st.process_block(blk(x[s], b, B))), (b, s)
            assert np.array_equal(idx[s], st.p.targetTDOAIndexes), (b, s)
    assert np.array_equal(bk.targetTDOAIndexes[1], np.float32([5, 20]))
    y = bk.process_streams(x[:, :, :3 * B])
    assert y.shape == (S, N, 2, 3 * B)


def test_graph_replay_equals_direct_launches():
    name, N = 'config5', 3
    B = CONFIGS[name][2]
    x = mixture(30 * B, seed=6)
    outs = []
    for use_graph in (False, True):
        p = processor(name, N, loc=True)
        st = stream(p, name, use_graph=use_graph)
        ys = [st.process_block(blk(x, b, B)) for b in range(30)]
        assert (st._graph is not None) == use_graph and st.capture_error is None
        outs.append((np.stack(ys), p.targetTDOAIndexes))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    from gcc_nmf_amd.realtime import StreamingGCCNMFBank
    ws, hop, B, K, D, nh, syn, delay = CONFIGS[name]
    xs = np.stack([x, x[::-1].copy()])
    bouts = []
    for use_graph in (False, True):
        bk = StreamingGCCNMFBank(processor(name, N, loc=True), 2, hop, B, outputDelayBlocks=delay, use_graph=use_graph)
        bouts.append(np.stack([bk.process_block(blk(xs, b, B)) for b in range(30)]))
    assert np.array_equal(bouts[0], bouts[1])


@pytest.mark.parametrize('mode', [0, 2])
def test_single_target_modes_are_unchanged_by_a_multi_session(mode):
    name = 'tc4'
    B = CONFIGS[name][2]
    x = mixture(20 * B, seed=7)
    p = processor(name, 2, loc=False, mode=mode)

    def single():
        p.targetMode = mode
        p.localizationEnabled = False
        p.setTargetTDOARange(20.0, 4.0, 2.0, 0.1)
        st = stream(p, name)
        return np.stack([st.process_block(blk(x, b, B)) for b in range(20)])
    before = single()
    p.targetMode = 1
    p.localizationEnabled = True
    ym = stream(p, name).process_stream(x)
    assert ym.shape == (2, 2, 20 * B) and np.isfinite(ym).all()
    after = single()
    assert before.shape == (20, 2, B) and np.array_equal(before, after)


def test_processFrames_returns_one_frame_set_per_target():
    name, N = 'reference', 3
    ws, hop, B, K, D, nh, syn, delay = CONFIGS[name]
    p = processor(name, N)
    frames = np.random.RandomState(0).standard_normal((2, ws, 1)).astype(np.float32) * 0.1
    out = p.processFrames(frames)
    assert out.shape == (N, 2, ws, 1)
    ora, _ = oracle_for(p, name, N)
    dev = np.argmax(p.intermediates()['HMask'], axis=0)
    want = ora.processFrames(frames, target_override=dev)
    assert np.abs(out - want).max() < 1e-5 * max(1.0, np.abs(want).max())


def test_multi_abi_errors():
    """bit 20 needs target_mode 1; bits 21..23 need bit 20; nothing above bit 23."""
    from gcc_nmf_amd.engine import _ptr, _stream
    name, N = 'reference', 2
    p = processor(name, N)
    st = stream(p, name)
    out_ring, block_out = st._outputs()

    def call(bits, mode):
        with torch.cuda.device(p.device):
            r = p.lib.gccnmf_rt_process_block_ll(
                _ptr(st.block_in), _ptr(block_out), _ptr(st.in_ring), _ptr(out_ring), _ptr(p.dX), _ptr(p.dYm), _ptr(p.dC),
                _ptr(p.dHMaskm), _ptr(p.dArgmax), _ptr(p.dTfMaskm), _ptr(p.dHist), _ptr(p.dHistPos), _ptr(p.dTarget), _ptr(p.dGccPhat),
                _ptr(p.dW), _ptr(p.dCos), _ptr(p.dSin), _ptr(p.dWindow), _ptr(p.dSynthWindow), _ptr(p.dTwiddle), _ptr(p.dColsum),
                _ptr(p.dHcoef), _ptr(p.dRv), p.windowSize, CONFIGS[name][1], CONFIGS[name][2], p.numAtom, p.Kp, p.numTDOAs, p.Dp,
                p.numTDOAHistory, mode, 1, 1, p.localizationWindowSize, bits, 0, 2, _stream())
            torch.cuda.synchronize()
        return r
    ok = (1 << 20) | ((N - 1) << 21)
    assert call(ok, 1) == 0
    assert call(ok, 2) == 1 and call(ok, 0) == 1
    assert call(1 << 21, 1) == 1
    assert call(ok | (1 << 24), 1) == 1
