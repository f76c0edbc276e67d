"""-m gpu: the online spatial filter in the real-time classes (GCCNMFProcessor.spatialFilterEnabled / spatialFilterFrames,
StreamingGCCNMF, StreamingGCCNMFBank.setSpatialFilter).

The stage test (tests/test_gpu_rt_spatial_stage.py) checks one call element-wise; here the state is carried by the classes.  A stream's
filtered Y of every block is compared with the recursion restated in float64 (tests/rt_spatial_restatement.py) from the device's own
tfMask and X of that block (Y = float32(tfMask) . X bit for bit, rule 6 of rt_checks) and the RESTATED state carried from block to block, so
no arg-max has to agree and nothing is excluded.  The bar is the project's rule over the whole run: BAR_FACTOR x the largest distance of the
float32 NumPy evaluation, which carries its own float32 state through the same blocks, from the float64 one, relative to the largest |X| of
the run.  Everything else is bitwise: graph replay against direct launches, the attribute switched off against a stream that never had it,
a bank against standalone streams."""
import warnings

import numpy as np
import pytest

import fft_checks as K
import rt_spatial_restatement as RS
from oracle import gccnmf_oracle as O
from oracle import rt_oracle as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

TARGET = (9.6, 5.0, 2.0, 0.0)
# name: (windowSize, hopSize, blockSize, K, D, numHUpdates, asymmetric synthesis size or None, outputDelayBlocks)
CONFIGS = {
    'config5': (512, 64, 64, 1024, 64, 2, 128, 1),
    'tc4': (512, 64, 256, 128, 48, 1, None, 2),
    'plain': (256, 64, 128, 96, 48, 0, None, 2),
}
TAU = 8.0


def processor(name, mode=None, spatial=True, tau=TAU, sources=2):
    from gcc_nmf_amd.realtime import GCCNMFProcessor, asymmetricWindows
    ws, hop, B, Kd, D, nh, syn, _ = CONFIGS[name]
    kw = {}
    if syn:
        a, sy = asymmetricWindows(ws, syn)
        kw = dict(analysisWindow=a, synthesisWindow=sy)
    W = R.make_rt_dictionary(3, ws // 2 + 1, Kd)
    p = GCCNMFProcessor(16000, ws, B // hop, {'Pretrained': {Kd: W}}, 'Pretrained', Kd, nh, 0.1, True, 6, numTDOAs=D, numSources=sources,
                        spatialFilterEnabled=spatial, spatialFilterFrames=tau, **kw)
    if mode is not None:
        p.targetMode = mode
        p.reset()
    p.setTargetTDOARange(*TARGET)
    return p


def stream(name, use_graph=False, **kw):
    from gcc_nmf_amd.realtime import StreamingGCCNMF
    ws, hop, B, Kd, D, nh, syn, delay = CONFIGS[name]
    return StreamingGCCNMF(processor(name, **kw), hop, B, outputDelayBlocks=delay, use_graph=use_graph)


def signals(S, n, seed0=0):
    return np.stack([O.synthetic_mixture(seed0 + s, numSamples=n, delays=(-3 + s % 4, 1, 4 - s % 3)) for s in range(S)])


def masked(im, multi):
    """The mask kernel's Y (NY, 2, F, Tc) complex64 from the device's tfMask and X: float32(tfMask) . X, one rounding per component."""
    X, tf = im['X'], np.asarray(im['tfMask'], np.float32)
    if not multi:
        tf = tf[None]
    if tf.ndim == 3:                                          # no coefficient inference: one mask for both channels
        tf = np.repeat(tf[:, None], 2, axis=1)
    Y = np.empty(tf.shape, np.complex64)
    Y.real, Y.imag = tf * X.real[None], tf * X.imag[None]
    return Y, X


class Restated(object):
    """The recursion carried over a run, in float64 (the contract) and in float32 (what the bar is measured from)."""

    def __init__(self, NC, F):
        self.P64, self.P32 = np.zeros((NC, F, 4), np.float32), np.zeros((NC, F, 4), np.float32)
        self.err, self.dev, self.xmax = 0.0, 0.0, 0.0

    def block(self, Ymask, X, got, tau, multi):
        Y64, self.P64 = RS.rt_spatial(Ymask, X, self.P64, tau, multi, np.float64)
        Y32, self.P32 = RS.rt_spatial(Ymask, X, self.P32, tau, multi, np.float32)
        assert np.isfinite(Y64).all() and np.isfinite(got).all()
        self.err = max(self.err, float(np.abs(Y32 - Y64).max()))
        self.dev = max(self.dev, float(np.abs(got.astype(np.complex128) - Y64).max()))
        self.xmax = max(self.xmax, float(np.abs(X).max()))

    def bar(self):
        return RS.BAR_FACTOR * self.err / self.xmax


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)           # nanmean of the all-zero start-up frames
        yield


def test_forty_blocks_of_one_stream_follow_the_restated_recursion():
    name = 'config5'
    B = CONFIGS[name][2]
    x = signals(1, 40 * B, seed0=5)[0]
    st = stream(name)
    p = st.p
    rs = Restated(2, p.numFrequencies)
    for b in range(40):
        st.process_block(x[:, b * B:(b + 1) * B])
        im = p.intermediates()
        Ymask, X = masked(im, False)
        rs.block(Ymask, X, im['Y'][None], TAU, False)
    print('config 5, 40 blocks: float32 error %.3e, bar %.3e, device %.3e (relative to max|X| = %.3e)' % (rs.err / rs.xmax, rs.bar(), rs.dev / rs.xmax, rs.xmax))
    assert rs.bar() > 0
    assert rs.dev / rs.xmax <= rs.bar()
    cov = p.intermediates()['spatialCovariance']
    assert cov.shape == (2, p.numFrequencies, 4)
    assert np.abs(cov.astype(np.float64) - rs.P64).max() <= RS.BAR_FACTOR * max(np.abs(rs.P32.astype(np.float64) - rs.P64).max(), 2.0 ** -24 * np.abs(rs.P64).max())


@pytest.mark.parametrize('name,mode', [('config5', None), ('tc4', 1)], ids=['config5', 'tc4 multiple'])
def test_graph_replay_equals_direct_launches(name, mode):
    B = CONFIGS[name][2]
    x = signals(1, 14 * B, seed0=2)[0]
    a, d = stream(name, use_graph=True, mode=mode, sources=3), stream(name, use_graph=False, mode=mode, sources=3)
    for b in range(14):
        ya, yd = a.process_block(x[:, b * B:(b + 1) * B]), d.process_block(x[:, b * B:(b + 1) * B])
        assert np.array_equal(ya, yd), b
    assert a._graph is not None and a.capture_error is None
    assert np.array_equal(a.p.intermediates()['spatialCovariance'], d.p.intermediates()['spatialCovariance'])
    assert np.abs(a.p.intermediates()['spatialCovariance']).max() > 0


def test_switching_the_attribute_off_gives_the_plain_stream_from_that_block_on():
    """The masks do not depend on the filter (the tracking reads the coherence), so a stream that never filtered is the reference: Y is
    its Y from the block of the switch on, bit for bit, and the output blocks once the 8-block overlap-add buffer holds no filtered frame."""
    name = 'plain'
    B = CONFIGS[name][2]
    x = signals(1, 30 * B, seed0=4)[0]
    a, plain = stream(name, use_graph=True), stream(name, use_graph=True, spatial=False)
    differed = False
    for b in range(30):
        if b == 10:
            a.p.spatialFilterEnabled = False
        if b == 22:
            a.p.spatialFilterEnabled, a.p.spatialFilterFrames = True, 3
        ya, yp = a.process_block(x[:, b * B:(b + 1) * B]), plain.process_block(x[:, b * B:(b + 1) * B])
        same_Y = np.array_equal(a.p.intermediates()['Y'], plain.p.intermediates()['Y'])
        if b < 10 or b >= 22:
            differed = differed or not same_Y
        else:
            assert same_Y, b
            if b >= 18:
                assert np.array_equal(ya, yp), b
        assert a.p.targetTDOAIndex == plain.p.targetTDOAIndex
    assert differed
    assert float(a.p.dTarget[7]) == 3.0 and float(plain.p.dTarget[7]) == 0.0


def test_a_bank_of_five_is_five_standalone_streams():
    from gcc_nmf_amd.realtime import StreamingGCCNMFBank
    name = 'tc4'
    ws, hop, B, Kd, D, nh, syn, delay = CONFIGS[name]
    S, nb = 5, 18
    x = signals(S, nb * B, seed0=11)
    bk = StreamingGCCNMFBank(processor(name, spatial=False), S, hop, B, outputDelayBlocks=delay)
    alone = [stream(name, spatial=False) for s in range(S)]
    for s, tau in ((0, 4.0), (2, None), (4, 32.0)):           # stream 1 never filters, stream 3 is toggled below; None: the processor's frames
        bk.setSpatialFilter(s, True, tau)
        alone[s].p.spatialFilterEnabled, alone[s].p.spatialFilterFrames = True, TAU if tau is None else tau
    for b in range(nb):
        if b in (5, 12):
            on = b == 5
            bk.setSpatialFilter(3, on, 6.0)
            alone[3].p.spatialFilterEnabled, alone[3].p.spatialFilterFrames = on, 6.0
        yb = bk.process_block(x[..., b * B:(b + 1) * B])
        for s in range(S):
            assert np.array_equal(yb[s], alone[s].process_block(x[s][:, b * B:(b + 1) * B])), (b, s)
    assert bk._graph is not None and bk.capture_error is None
    state = bk.dSpatial.cpu().numpy()
    for s in range(S):
        assert np.array_equal(state[s], alone[s].p.intermediates()['spatialCovariance']), s
    assert not state[1].any() and state[3].any()
    # reset_stream zeroes one stream's state only
    bk.reset_stream(2)
    after = bk.dSpatial.cpu().numpy()
    assert not after[2].any()
    for s in (0, 1, 3, 4):
        assert np.array_equal(after[s], state[s])


def test_process_frames_carries_the_state_and_reset_clears_it():
    name = 'tc4'
    ws, hop, B, Kd, D, nh, syn, delay = CONFIGS[name]
    Tc = B // hop
    rng = np.random.RandomState(8)
    frames = (rng.standard_normal((2, ws, Tc)) * np.hanning(ws)[None, :, None]).astype(np.float32)
    p = processor(name)
    first = p.processFrames(frames)
    cov1 = p.intermediates()['spatialCovariance'].copy()
    rs = Restated(2, p.numFrequencies)
    im = p.intermediates()
    rs.block(*masked(im, False), im['Y'][None], TAU, False)
    second = p.processFrames(frames)                         # the same frames on a state that remembers them
    im = p.intermediates()
    rs.block(*masked(im, False), im['Y'][None], TAU, False)
    assert rs.dev / rs.xmax <= rs.bar()
    assert cov1.any() and not np.array_equal(cov1, im['spatialCovariance']) and not np.array_equal(first, second)
    p.reset()
    p.setTargetTDOARange(*TARGET)
    assert not p.intermediates()['spatialCovariance'].any()
    assert np.array_equal(p.processFrames(frames), first)


def test_the_outputs_of_multiple_mode_add_up_to_the_delayed_mixture():
    """sum_j Y_j = X within N x the stage bar per bin (the consequence the stage test asserts), and the synthesis is linear, so in exact
    arithmetic the N outputs add up to the synthesis of X -- what a stream with its separation off hands out -- within
    n_ov N bar max|X| (2F / n_fft): n_ov = n_fft / hop frames overlap in a sample, a synthesis window <= 1, and an inverse transform is
    at most the sum of its 2F - 2 Hermitian terms over n_fft.  In float32 each of the N + 1 signals adds rule 8's rounding per frame,
    C_FFT log2(n_fft) u sum|Z| / n_fft with sum|Z| <= 2 n_fft max|X| (fft_checks.frames_bar), and u |running sum| per overlap-add."""
    name = 'tc4'
    ws, hop, B, Kd, D, nh, syn, delay = CONFIGS[name]
    N, nb = 3, 14
    x = signals(1, nb * B, seed0=6)[0]
    st = stream(name, mode=1, sources=N)
    thru = stream(name, mode=1, sources=N, spatial=False)
    thru.p.separationEnabled = False
    rs = Restated(N, st.p.numFrequencies)
    worst = 0.0
    outs = []
    for b in range(nb):
        y, yt = st.process_block(x[:, b * B:(b + 1) * B]), thru.process_block(x[:, b * B:(b + 1) * B])
        im = st.p.intermediates()
        rs.block(*masked(im, True), im['Y'], TAU, True)
        outs.append((y, yt))
    assert rs.dev / rs.xmax <= rs.bar()
    n_ov, F = ws // hop, ws // 2 + 1
    for y, yt in outs:
        assert y.shape == (N, 2, B) and np.array_equal(yt[0], yt[N - 1])
        peak = max(float(np.abs(y).max()), float(np.abs(yt).max()))
        tol = n_ov * (N * rs.bar() * rs.xmax * 2.0 * F / ws + (N + 1) * (K.C_FFT * K.ilog2(ws) * K.U32 * 2 * rs.xmax + K.U32 * peak))
        worst = max(worst, float(np.abs(y.astype(np.float64).sum(axis=0) - yt[0]).max()) / tol)
    print('multiple mode, N = 3: the outputs add up to the mixture within %.4f of the propagated bar' % worst)
    assert worst <= 1.0
