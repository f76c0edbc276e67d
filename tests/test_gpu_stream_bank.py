"""-m gpu: the stream bank (gcc_nmf_amd.realtime.StreamingGCCNMFBank, frames_mode bit 3 of gccnmf_rt_process_block_ll): S streams of
one configuration in one device call per block.  Stream s runs the single-stream arithmetic on its own state, so every comparison
with standalone StreamingGCCNMF objects is bitwise."""
import warnings

import numpy as np
import pytest

from oracle import gccnmf_oracle as O
from oracle import rt_oracle as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

TARGET = (9.6, 5.0, 2.0, 0.0)
# name: (windowSize, hopSize, blockSize, K, D, numHUpdates, asymmetric synthesis size or None, outputDelayBlocks)
CONFIGS = {
    'reference': (1024, 512, 512, 128, 64, 0, None, 2),
    'config5': (512, 64, 64, 1024, 64, 2, 128, 1),
    'direct_sum_ws400': (400, 100, 100, 96, 48, 0, None, 2),
    'tc4': (512, 64, 256, 128, 48, 1, None, 2),
}


def processor(name, seed=3, loc=True, mode=None):
    from gcc_nmf_amd.realtime import GCCNMFProcessor, asymmetricWindows
    ws, hop, B, K, D, nh, syn, _ = CONFIGS[name]
    kw = {}
    if syn:
        a, sy = asymmetricWindows(ws, syn)
        kw = dict(analysisWindow=a, synthesisWindow=sy)
    W = R.make_rt_dictionary(seed, ws // 2 + 1, K)
    p = GCCNMFProcessor(16000, ws, B // hop, {'Pretrained': {K: W}}, 'Pretrained', K, nh, 0.1, loc, 6, numTDOAs=D, **kw)
    if mode is not None:
        p.targetMode = mode
    p.setTargetTDOARange(*TARGET)
    return p


def standalone(name, target=TARGET, loc=True, sep=True, mode=None, use_graph=True):
    from gcc_nmf_amd.realtime import StreamingGCCNMF
    ws, hop, B, K, D, nh, syn, delay = CONFIGS[name]
    p = processor(name, loc=loc, mode=mode)
    p.setTargetTDOARange(*target)
    p.separationEnabled = sep
    return StreamingGCCNMF(p, hop, B, outputDelayBlocks=delay, use_graph=use_graph)


def bank(name, S, mode=None, use_graph=True):
    from gcc_nmf_amd.realtime import StreamingGCCNMFBank
    ws, hop, B, K, D, nh, syn, delay = CONFIGS[name]
    return StreamingGCCNMFBank(processor(name, mode=mode), S, hop, B, outputDelayBlocks=delay, use_graph=use_graph)


def signals(S, n, seed0=0):
    """(S, 2, n): stream s hears the sources at its own delays."""
    return np.stack([O.synthetic_mixture(seed0 + s, numSamples=n, delays=(-3 + s % 4, 1, 4 - s % 3)) for s in range(S)])


def blocks_of(x, b, B):
    return x[..., b * B:(b + 1) * B]


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)           # nanmean of the all-zero start-up frames
        yield


@pytest.mark.parametrize('name', list(CONFIGS))
def test_one_stream_bank_is_the_single_stream_path(name):
    B = CONFIGS[name][2]
    x = signals(1, 44 * B, seed0=5)
    bk, st = bank(name, 1), standalone(name)
    for b in range(44):
        yb = bk.process_block(blocks_of(x, b, B))
        ys = st.process_block(blocks_of(x[0], b, B))
        assert np.array_equal(yb[0], ys), b
        assert bk.targetTDOAIndexes[0] == st.p.targetTDOAIndex, b
    assert np.isfinite(yb).all()


@pytest.mark.parametrize('name,mode', [(n, None) for n in CONFIGS] + [('reference', 0)])
def test_five_streams_each_equal_their_own_standalone_stream(name, mode):
    """Different inputs and targets; stream 1 tracks nothing (fixed target), stream 2 is passed through.  mode 0 = boxcar."""
    B = CONFIGS[name][2]
    S, n_blocks = 5, 44
    x = signals(S, n_blocks * B, seed0=11)
    targets = [(9.6, 5.0, 2.0, 0.0), (20.0, 3.0, 1.0, 0.2), (40.0, 4.0, 2.0, 0.0), (12.0, 6.0, 1.5, 0.1), (30.0, 2.0, 2.0, 0.0)]
    bk = bank(name, S, mode=mode)
    st = [standalone(name, targets[s], loc=(s != 1), sep=(s != 2), mode=mode) for s in range(S)]
    for s in range(S):
        bk.setTargetTDOARange(s, *targets[s])
    bk.setLocalizationEnabled(1, False)
    bk.setSeparationEnabled(2, False)
    for b in range(n_blocks):
        yb = bk.process_block(blocks_of(x, b, B))
        idx = bk.targetTDOAIndexes
        for s in range(S):
            assert np.array_equal(yb[s], st[s].process_block(blocks_of(x[s], b, B))), (b, s)
            assert idx[s] == st[s].p.targetTDOAIndex, (b, s)
    assert bk.targetTDOAIndexes[1] == targets[1][0]


def test_one_stream_changing_leaves_every_other_stream_alone():
    name, S, n_blocks = 'config5', 4, 40
    B = CONFIGS[name][2]
    x = signals(S, n_blocks * B, seed0=21)
    noise = (np.random.RandomState(0).standard_normal((2, n_blocks * B)) * 0.3).astype(np.float32)
    runs = []
    for disturb in (False, True):
        bk = bank(name, S)
        ys = []
        for b in range(n_blocks):
            blk = blocks_of(x, b, B).copy()
            if disturb and b >= 10:
                blk[2] = blocks_of(noise, b, B)
            if disturb and b == 15:
                bk.setTargetTDOARange(2, 40.0, 2.0, 1.0, 0.3)
                bk.setLocalizationEnabled(2, False)
            if disturb and b == 25:
                bk.setSeparationEnabled(2, False)
            ys.append(bk.process_block(blk))
        runs.append((np.stack(ys), bk.targetTDOAIndexes))
    (y0, i0), (y1, i1) = runs
    others = [0, 1, 3]
    assert np.array_equal(y0[:, others], y1[:, others])
    assert np.array_equal(i0[others], i1[others])
    assert not np.array_equal(y0[:, 2], y1[:, 2]) and i1[2] == 40.0


@pytest.mark.parametrize('name', ['config5', 'reference'])
def test_reset_stream_starts_one_stream_over(name):
    B = CONFIGS[name][2]
    S, n_blocks, r = 3, 44, 20
    x = signals(S, n_blocks * B, seed0=31)
    bk = bank(name, S)
    st = [standalone(name) for _ in range(S)]
    fresh = standalone(name)
    for b in range(n_blocks):
        if b == r:
            bk.reset_stream(1)
        yb = bk.process_block(blocks_of(x, b, B))
        for s in (0, 2):
            assert np.array_equal(yb[s], st[s].process_block(blocks_of(x[s], b, B))), (b, s)
            assert bk.targetTDOAIndexes[s] == st[s].p.targetTDOAIndex
        if b >= r:
            assert np.array_equal(yb[1], fresh.process_block(blocks_of(x[1], b, B))), b
            assert bk.targetTDOAIndexes[1] == fresh.p.targetTDOAIndex


def test_tracked_index_survives_switching_one_streams_localisation_off():
    name = 'config5'
    B = CONFIGS[name][2]
    S = 2
    x = signals(S, 80 * B, seed0=41)
    bk = bank(name, S)
    st = [standalone(name) for _ in range(S)]
    for b in range(60):
        yb = bk.process_block(blocks_of(x, b, B))
        for s in range(S):
            st[s].process_block(blocks_of(x[s], b, B))
    tracked = bk.targetTDOAIndexes[0]
    assert tracked != TARGET[0] and tracked == st[0].p.targetTDOAIndex     # the tracking did move the target
    bk.setLocalizationEnabled(0, False)
    st[0].p.localizationEnabled = False
    assert bk.targetTDOAIndexes[0] == tracked
    for b in range(60, 80):
        yb = bk.process_block(blocks_of(x, b, B))
        assert bk.targetTDOAIndexes[0] == tracked
        for s in range(S):
            assert np.array_equal(yb[s], st[s].process_block(blocks_of(x[s], b, B))), (b, s)
        assert bk.targetTDOAIndexes[1] == st[1].p.targetTDOAIndex
    bk.setTargetTDOARange(0, 20.0, 5.0, 2.0, 0.0)
    assert bk.targetTDOAIndexes[0] == 20.0                                 # an explicit set wins again


def test_three_streams_match_the_oracle_with_online_localisation():
    """As test_stream_matches_oracle_with_online_localisation, stream by stream."""
    from gcc_nmf_amd.realtime import StreamingGCCNMFBank, GCCNMFProcessor
    ws, hop, B, K, D, S = 1024, 512, 512, 64, 64, 3
    W = R.make_rt_dictionary(3, ws // 2 + 1, K)
    p = GCCNMFProcessor(16000, ws, 1, {'Pretrained': {K: W}}, 'Pretrained', K, 0, 0.1, True, 6, numTDOAs=D)
    p.setTargetTDOARange(*TARGET)
    bk = StreamingGCCNMFBank(p, S, hop, B)
    x = np.stack([O.synthetic_mixture(5 + s, numSamples=16000, delays=(-3 + s, 1, 4 - s)) for s in range(S)])
    oras, olas = [], []
    for s in range(S):
        ora = R.GCCNMFProcessorOracle(16000, ws, 1, W, 0.1, D, localizationEnabled=True, localizationWindowSize=6)
        ora.setTargetTDOARange(*TARGET)
        oras.append(ora)
        olas.append(R.OverlapAddOracle(2, ws, hop, B, 1))
    worst = np.zeros(S)
    for b in range(x.shape[2] // B):
        yd = bk.process_block(blocks_of(x, b, B))
        idx = bk.targetTDOAIndexes
        for s in range(S):
            yr = olas[s].processFrames(blocks_of(x[s], b, B), oras[s].processFrames)
            worst[s] = max(worst[s], float(np.abs(yd[s] - yr).max()))
            assert idx[s] == float(oras[s].targetTDOAIndex), (b, s)
    assert (worst < 2e-4 * np.abs(x).max()).all(), worst
    assert np.isfinite(yd).all()


def test_graph_replay_equals_direct_launches_and_reset_invalidates_the_capture():
    name, S = 'config5', 3
    B = CONFIGS[name][2]
    x = signals(S, 60 * B, seed0=51)
    outs = []
    for use_graph in (False, True):
        bk = bank(name, S, use_graph=use_graph)
        ys = [bk.process_block(blocks_of(x, b, B)) for b in range(30)]
        bk.p.targetMode = 0                                         # a different launch argument -> re-capture
        ys += [bk.process_block(blocks_of(x, b, B)) for b in range(30, 40)]
        key0 = bk._graph_key
        bk.p.reset()                                                # re-allocates the tables and (next call) the bank's state
        ys += [bk.process_block(blocks_of(x, b, B)) for b in range(40, 60)]
        assert (bk._graph is not None) == use_graph and bk.capture_error is None
        if use_graph:
            assert bk._graph_key != key0
        outs.append(np.stack(ys))
    assert np.array_equal(outs[0], outs[1])
    # after the reset every stream starts over: equal to a fresh bank fed from block 40
    fresh = bank(name, S, use_graph=False)
    fresh.p.targetMode = 0
    again = np.stack([fresh.process_block(blocks_of(x, b, B)) for b in range(40, 60)])
    assert np.array_equal(outs[1][40:], again)


def test_process_streams_equals_block_calls():
    name, S = 'tc4', 3
    B = CONFIGS[name][2]
    x = signals(S, 30 * B + 17, seed0=61)
    y = bank(name, S).process_streams(x)
    bk = bank(name, S)
    y2 = np.concatenate([bk.process_block(blocks_of(x, b, B)) for b in range(30)], axis=2)
    assert y.shape == (S, 2, 30 * B) and np.array_equal(y, y2)


def test_256_streams_at_config5():
    name, S, n_blocks = 'config5', 256, 20
    B = CONFIGS[name][2]
    base = signals(4, n_blocks * B, seed0=71)
    x = np.stack([base[s % 4] * np.float32(1.0 + 0.002 * s) for s in range(S)])
    bk = bank(name, S)
    st = {s: standalone(name) for s in (0, S - 1)}
    for b in range(n_blocks):
        yb = bk.process_block(blocks_of(x, b, B))
        assert np.isfinite(yb).all(), b
        for s in st:
            assert np.array_equal(yb[s], st[s].process_block(blocks_of(x[s], b, B))), (b, s)
    idx = bk.targetTDOAIndexes
    assert idx.shape == (S,) and idx[S - 1] == st[S - 1].p.targetTDOAIndex


def _raw_call(bk, bits):
    """The C entry point on a bank's buffers with an arbitrary frames_mode word; returns the status."""
    from gcc_nmf_amd.engine import _ptr, _stream
    p = bk.p
    with torch.cuda.device(p.device):
        st = p.lib.gccnmf_rt_process_block_ll(
            _ptr(bk.block_in), _ptr(bk.block_out), _ptr(bk.in_ring), _ptr(bk.out_ring), _ptr(bk.dX), _ptr(bk.dY), _ptr(bk.dC),
            _ptr(bk.dHMask), _ptr(bk.dArgmax), _ptr(bk.dTfMask), _ptr(bk.dHist), _ptr(bk.dHistPos), _ptr(bk.dTarget),
            _ptr(bk.dGccPhat), _ptr(p.dW), _ptr(p.dCos), _ptr(p.dSin), _ptr(p.dWindow), _ptr(p.dSynthWindow), _ptr(p.dTwiddle),
            _ptr(p.dColsum), _ptr(bk.dHcoef), _ptr(bk.dRv), p.windowSize, bk.hopSize, bk.blockSize, p.numAtom, p.Kp, p.numTDOAs,
            p.Dp, p.numTDOAHistory, int(p.targetMode), 1, 1, p.localizationWindowSize, bits, int(p.numHUpdates),
            bk.outputDelayBlocks, _stream())
        torch.cuda.synchronize()
    return st


def test_bank_abi_errors():
    from gcc_nmf_amd.realtime import StreamingGCCNMFBank
    name, S = 'reference', 2
    ws, hop, B = CONFIGS[name][:3]
    bk = bank(name, S)
    ok = 8 | ((S - 1) << 8)
    assert _raw_call(bk, ok) == 0
    assert _raw_call(bk, ok | 1) == 1                      # bank layout with frames mode
    assert _raw_call(bk, 8 | (4096 << 8)) == 1             # S - 1 = 4096 does not fit bits 8..19
    assert _raw_call(bk, 8 | (1 << 27)) == 1               # any bit above 19
    assert _raw_call(bk, (S - 1) << 8) == 1                # a stream count without the bank layout
    for n in (0, 4097, 2.5):
        with pytest.raises(ValueError):
            StreamingGCCNMFBank(bk.p, n, hop, B)
    with pytest.raises(ValueError):
        bk.process_block(np.zeros((S + 1, 2, B), np.float32))
