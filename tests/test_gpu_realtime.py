"""-m gpu: the streaming GCC-NMF frame processor (csrc/rt.hip via gcc_nmf_amd.realtime) against the NumPy oracle of
gccNMF/realtime/gccNMFProcessor.py + utils.py (oracle/rt_oracle.py)."""
import copy
import warnings

import numpy as np
import pytest

from oracle import gccnmf_oracle as O
from oracle import rt_oracle as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def maxabs(a):
    return float(np.abs(a).max(initial=0.0))


def make(ws, K, D, Tc, seed=0, loc=True, L=6):
    from gcc_nmf_amd.realtime import GCCNMFProcessor
    rng = np.random.RandomState(seed)
    W = (rng.rand(ws // 2 + 1, K).astype(np.float32) + 0.02)
    W /= np.linalg.norm(W, axis=0)
    dev = GCCNMFProcessor(16000, ws, Tc, {'Pretrained': {K: W}}, 'Pretrained', K, 0, 0.1, loc, L, numTDOAs=D)
    ora = R.GCCNMFProcessorOracle(16000, ws, Tc, W, 0.1, D, localizationEnabled=loc, localizationWindowSize=L)
    return dev, ora, rng


@pytest.mark.parametrize('ws,K,D,Tc', [(1024, 64, 64, 1), (512, 200, 40, 4), (1024, 1024, 64, 2), (256, 96, 33, 8)])
def test_process_frames_matches_oracle(ws, K, D, Tc):
    dev, ora, rng = make(ws, K, D, Tc)
    compared = total = 0
    for mode, params in [(2, (9.6, 5.0, 2.0, 0.0)), (2, (20.0, 3.0, 1.0, 0.2)), (0, (12.0, 4.0, 1.0, 0.0))]:
        dev.targetMode = ora.targetMode = mode
        dev.localizationEnabled = ora.localizationEnabled = False
        dev.setTargetTDOARange(*params)
        ora.setTargetTDOARange(*params)
        frames = (rng.standard_normal((2, ws, Tc)) * 0.1).astype(np.float32)
        out = dev.processFrames(frames)
        ora_c = copy.deepcopy(ora)
        ref, im = ora.processFrames(frames, return_intermediates=True)
        d = dev.intermediates()
        assert np.abs(d['X'] - im['X']).max() < 1e-5 * np.abs(im['X']).max()
        strong = np.minimum(np.abs(im['X'][0]), np.abs(im['X'][1])) > 1e-2 * np.abs(im['X']).max()
        assert np.abs(d['C'] - im['C'])[strong].max() < 2e-3
        assert np.mean(d['argmaxTDOA'] != im['argmaxTDOA']) < 5e-3                 # near-ties of f32 vs f32-BLAS scores only
        same = d['argmaxTDOA'] == im['argmaxTDOA']
        assert np.abs(d['HMask'] - im['HMask'])[same].max() < 1e-5
        assert np.abs(d['gccPHAT'] - im['gccPHAT']).max() < 1e-3
        # the mask and output stages under the device's own arg-max, on every frame
        ref_c, im_c = ora_c.processFrames(frames, return_intermediates=True, argmax_override=d['argmaxTDOA'])
        assert np.abs(d['tfMask'] - im_c['tfMask']).max() < 1e-4
        assert np.abs(out - ref_c).max() < 1e-4 * max(np.abs(ref_c).max(), 1e-6)
        # ... and against the oracle's own run on every frame where no atom flipped
        ok = same.all(axis=0)
        compared, total = compared + int(ok.sum()), total + ok.size
        assert maxabs(d['tfMask'][..., ok] - im['tfMask'][..., ok]) < 1e-4
        assert maxabs(out[..., ok] - ref[..., ok]) < 1e-4 * max(np.abs(ref).max(), 1e-6)
        assert out.shape == (2, ws, Tc) and out.dtype == np.float32
    assert 2 * compared > total, (compared, total)


@pytest.mark.parametrize('ws', [3838, 4094])
def test_process_frames_at_the_largest_windows_off_the_powers_of_two(ws):
    """Windows near the 4096 bound on the direct-sum kernels: their cos / sin table + frame image pass the 64 KB of dynamic LDS a launch
    gets by default (the launcher raises the kernels' limit) -- the frames still match the oracle."""
    dev, ora, rng = make(ws, 64, 32, 1, loc=False)
    for p in (dev, ora):
        p.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
    frames = (rng.standard_normal((2, ws, 1)) * 0.1).astype(np.float32)
    out = dev.processFrames(frames)
    ora_c = copy.deepcopy(ora)
    ref, im = ora.processFrames(frames, return_intermediates=True)
    d = dev.intermediates()
    assert np.abs(d['X'] - im['X']).max() < 1e-4 * np.abs(im['X']).max()
    assert np.mean(d['argmaxTDOA'] != im['argmaxTDOA']) < 2e-2
    # the output under the device's own arg-max; against the oracle's run wherever no atom of the (single) frame flipped
    ref_c = ora_c.processFrames(frames, argmax_override=d['argmaxTDOA'])
    assert np.abs(out - ref_c).max() < 1e-3 * max(np.abs(ref_c).max(), 1e-6)
    ok = (d['argmaxTDOA'] == im['argmaxTDOA']).all(axis=0)
    assert maxabs(out[..., ok] - ref[..., ok]) < 1e-3 * max(np.abs(ref).max(), 1e-6)
    assert out.shape == (2, ws, 1) and np.isfinite(out).all()


@pytest.mark.parametrize('ws,hop,B,K,D', [(1024, 512, 512, 64, 64), (512, 64, 64, 256, 64), (512, 128, 256, 128, 48)])
def test_stream_matches_oracle_with_online_localisation(ws, hop, B, K, D):
    """Block-by-block streaming with TDOA tracking: the fused device call against OverlapAddOracle + processor oracle."""
    from gcc_nmf_amd.realtime import StreamingGCCNMF
    dev, ora, rng = make(ws, K, D, B // hop, seed=3, loc=True, L=6)
    for p in (dev, ora):
        p.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
    x = O.synthetic_mixture(5, numSamples=16000, delays=(-3, 1, 4))
    n_blocks = x.shape[1] // B
    stream = StreamingGCCNMF(dev, hop, B)
    ola = R.OverlapAddOracle(2, ws, hop, B, B // hop)
    tdoa_dev, tdoa_ref, worst = [], [], 0.0
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                                   # nanmean of the all-zero start-up frames
        for b in range(n_blocks):
            blk = x[:, b * B:(b + 1) * B]
            yd = stream.process_block(blk)
            yr = ola.processFrames(blk, ora.processFrames)
            tdoa_dev.append(dev.targetTDOAIndex)
            tdoa_ref.append(float(ora.targetTDOAIndex))
            worst = max(worst, float(np.abs(yd - yr).max()))
            if tdoa_dev[-1] != tdoa_ref[-1]:
                break
    assert tdoa_dev == tdoa_ref                                            # the tracked target, block by block
    assert worst < 2e-4 * np.abs(x).max()
    assert np.isfinite(yd).all()


def test_tracked_index_survives_switching_the_localisation_off():
    """The reference toggles ``localizationEnabled`` at run time (gccNMFProcessor.py:112-116, the GUI checkbox) and keeps the last tracked
    target.  So does the device (dTarget[0] stays what the tracking left and the masks keep using it) -- and so must the host property:
    after tracking has moved the target away from what setTargetTDOARange set, switching the localisation off must not bring the
    stale host copy back; the oracle processor is the witness, block by block, across the toggle."""
    from gcc_nmf_amd.realtime import StreamingGCCNMF
    ws, hop, B, K, D = 512, 64, 64, 128, 64
    dev, ora, rng = make(ws, K, D, B // hop, seed=3, loc=True, L=6)
    for p in (dev, ora):
        p.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
    x = O.synthetic_mixture(5, numSamples=16000, delays=(-3, 1, 4))
    stream = StreamingGCCNMF(dev, hop, B)
    ola = R.OverlapAddOracle(2, ws, hop, B, B // hop)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for b in range(60):
            blk = x[:, b * B:(b + 1) * B]
            stream.process_block(blk)
            ola.processFrames(blk, ora.processFrames)
        tracked = float(ora.targetTDOAIndex)
        assert tracked != 9.6                                              # the tracking did move the target
        dev.localizationEnabled = ora.localizationEnabled = False          # (no read of the property in between: the value is fetched after the toggle)
        assert dev.targetTDOAIndex == tracked
        for b in range(60, 80):
            blk = x[:, b * B:(b + 1) * B]
            yd = stream.process_block(blk)
            yr = ola.processFrames(blk, ora.processFrames)
            assert dev.targetTDOAIndex == float(ora.targetTDOAIndex) == tracked
        assert np.abs(yd - yr).max() < 2e-4 * np.abs(x).max()              # the masks still steer at the tracked index
        dev.setTargetTDOARange(20.0, 5.0, 2.0, 0.0)
        assert dev.targetTDOAIndex == 20.0                                 # an explicit set wins again


def test_process_stream_equals_block_calls_and_passthrough():
    from gcc_nmf_amd.realtime import StreamingGCCNMF
    ws, hop, B, K, D = 512, 128, 128, 64, 32
    dev, ora, rng = make(ws, K, D, 1, seed=4, loc=False)
    x = (rng.standard_normal((2, 40 * B)) * 0.05).astype(np.float32)
    dev.separationEnabled = False                                          # :210-211 pass-through
    y = StreamingGCCNMF(dev, hop, B).process_stream(x)
    ref = R.run_stream(x, type('P', (), {'processFrames': staticmethod(lambda w: w * ora.windowFunction * ora.windowFunction)})(), ws, hop, B)
    assert np.abs(y - ref).max() < 1e-5
    dev.separationEnabled = True
    dev.reset()
    y1 = StreamingGCCNMF(dev, hop, B).process_stream(x)
    dev.reset()
    s2 = StreamingGCCNMF(dev, hop, B)
    y2 = np.concatenate([s2.process_block(x[:, b * B:(b + 1) * B]) for b in range(40)], axis=1)
    assert np.array_equal(y1, y2)


# ---- against goldens of the UNMODIFIED reference processor (oracle/make_rt_golden.py, theano_stub) ---------------------
import os                                                                           # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
NEAR_TIE = 1e-4        # relative top-2 gap of the reference's float32 scores below which an arg-max may legitimately differ


@pytest.mark.parametrize('case', ['a', 'b', 'c', 'd', 'e', 'f'])        # e, f: windowSize 400 / 1000 -> the direct-sum kernels
def test_process_frames_vs_reference_goldens(case):
    from gcc_nmf_amd.realtime import GCCNMFProcessor
    g = np.load(os.path.join(GOLD, 'rt_frames_%s.npz' % case))
    ws, K, D, Tc, seed = [int(v) for v in g['params']]
    W = R.make_rt_dictionary(seed, ws // 2 + 1, K)
    dev = GCCNMFProcessor(16000, ws, Tc, {'Pretrained': {K: W}}, 'Pretrained', K, 0, float(g['d']), False, 6, numTDOAs=D)
    ora = R.GCCNMFProcessorOracle(16000, ws, Tc, W, float(g['d']), D, localizationEnabled=False)
    compared = total = 0
    for i in range(3):
        dev.targetMode = ora.targetMode = int(g['mode%d' % i])
        dev.setTargetTDOARange(*g['target%d' % i])
        ora.setTargetTDOARange(*g['target%d' % i])
        out = dev.processFrames(g['frames%d' % i])
        d = dev.intermediates()
        X, C, y = g['X%d' % i], g['C%d' % i], g['y%d' % i]
        assert np.abs(d['X'] - X).max() < 1e-5 * np.abs(X).max()
        strong = np.minimum(np.abs(X[0]), np.abs(X[1])) > 1e-2 * np.abs(X).max()
        assert np.abs(d['C'] - C)[strong].max() < 2e-3
        flipped = d['argmaxTDOA'] != g['argmax%d' % i]
        assert (g['gap%d' % i][flipped] < NEAR_TIE).all(), (int(flipped.sum()), float(g['gap%d' % i][flipped].max()))
        assert flipped.mean() < 2e-3
        assert np.abs(d['HMask'] - g['HMask%d' % i])[~flipped].max() < 1e-5
        assert np.abs(d['gccPHAT'] - g['gccPHAT%d' % i]).max() < 1e-4
        # the mask and output stages under the device's own arg-max (the oracle is pinned to these goldens), on every frame
        ref_c, im_c = ora.processFrames(g['frames%d' % i], return_intermediates=True, argmax_override=d['argmaxTDOA'])
        assert np.abs(d['tfMask'] - im_c['tfMask']).max() < 1e-5
        assert np.abs(out - ref_c).max() < 1e-5 * np.abs(y).max() + 1e-7
        # ... and against the reference's own run on every frame where no atom flipped
        ok = ~flipped.any(axis=0)
        compared, total = compared + int(ok.sum()), total + ok.size
        assert maxabs(d['tfMask'][..., ok] - g['tfMask%d' % i][..., ok]) < 1e-5
        assert maxabs(out[..., ok] - y[..., ok]) < 1e-5 * np.abs(y).max() + 1e-7
    assert 2 * compared > total, (compared, total)


@pytest.mark.parametrize('case', ['default', 'lowlatency', 'dev1', 'ws400', 'ws1000', 'bigblock'])
def test_stream_vs_reference_goldens(case):
    """The fused block call against a block-by-block run of the reference's OverlapAddProcessor + GCCNMFProcessor with online
    localisation: same tracked TDOA after every block, same audio."""
    from gcc_nmf_amd.realtime import GCCNMFProcessor, StreamingGCCNMF
    g = np.load(os.path.join(GOLD, 'rt_stream_%s.npz' % case))
    ws, hop, B, K, D, numBlocks, L, seed = [int(v) for v in g['params']]
    W = R.make_rt_dictionary(seed, ws // 2 + 1, K)
    dev = GCCNMFProcessor(16000, ws, B // hop, {'Pretrained': {K: W}}, 'Pretrained', K, 0, float(g['d']), True, L, numTDOAs=D)
    dev.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
    s = StreamingGCCNMF(dev, hop, B)
    x, yref = g['x'], g['y']
    worst, sq, compared = 0.0, 0.0, 0
    for b in range(numBlocks):
        y = s.process_block(x[:, b * B:(b + 1) * B])
        worst = max(worst, float(np.abs(y - yref[:, b * B:(b + 1) * B]).max()))
        sq += float(((y - yref[:, b * B:(b + 1) * B]) ** 2).sum())
        compared += 1
        if dev.targetTDOAIndex != g['tdoa'][b]:
            # only a genuine near-tie of the reference's own localisation spectrum may flip the track; the states diverge from here
            assert g['loc_gap'][b] < NEAR_TIE, (b, dev.targetTDOAIndex, g['tdoa'][b], g['loc_gap'][b])
            break
    assert compared > numBlocks // 2, compared
    # audio: float32 FFT/GEMM rounding plus the occasional near-tie arg-max flip of one atom in one frame (measured on MI355X:
    # worst sample 2.3e-5 at peak 0.1 in the 300-block hop-64 case, where every sample is covered by 8 windows)
    assert worst < 5e-4 * np.abs(x).max(), worst
    assert np.sqrt(sq / (2 * B * compared)) < 3e-5 * np.abs(x).max(), np.sqrt(sq / (2 * B * compared))


@pytest.mark.parametrize('case', ['default', 'lowlatency', 'dev1', 'ws400', 'bigblock'])
def test_history_mirrors_vs_reference_stream_goldens(case):
    """the host mirrors the reference GUI reads (gccNMFProcessor.py:211-229).  gccPHATHistory / tdoaHistory objects passed
    to the constructor are filled after every block; after the whole stream they hold what the reference's own
    SharedMemoryCircularBuffers held (goldens from the unmodified processor)."""
    from gcc_nmf_amd.realtime import GCCNMFProcessor, StreamingGCCNMF
    g = np.load(os.path.join(GOLD, 'rt_stream_%s.npz' % case))
    ws, hop, B, K, D, numBlocks, L, seed = [int(v) for v in g['params']]
    W = R.make_rt_dictionary(seed, ws // 2 + 1, K)
    Lh = g['gccPHATHistory'].shape[1]
    gcc, tdoa = R.CircularHistory((D, Lh)), R.CircularHistory((1, Lh))
    dev = GCCNMFProcessor(16000, ws, B // hop, {'Pretrained': {K: W}}, 'Pretrained', K, 0, float(g['d']), True, L, gccPHATHistory=gcc,
                          tdoaHistory=tdoa, numTDOAs=D, numTDOAHistory=Lh)
    dev.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
    s = StreamingGCCNMF(dev, hop, B)
    x = g['x']
    for b in range(numBlocks):
        s.process_block(x[:, b * B:(b + 1) * B])
        if dev.targetTDOAIndex != g['tdoa'][b]:
            assert g['loc_gap'][b] < NEAR_TIE
            pytest.skip('the track left the reference at a genuine near-tie of its own localisation spectrum (block %d)' % b)
    ref_t = g['tdoaHistory']
    assert np.array_equal(tdoa.getUnraveledArray(), ref_t)                        # every block's tracked index, in ring order
    got, ref = gcc.getUnraveledArray(), g['gccPHATHistory']
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.abs(got[ok] - ref[ok]).max() < 2e-4                                  # mean over F = 257..513 unit-modulus terms in float32


def test_spectrogram_and_mask_history_mirrors():
    """inputSpectrogramHistory / outputSpectrogramHistory / coefficientMaskHistories (gccNMFProcessor.py:211-217,228-229): the
    reference's expressions, incl. -mean(|X|) ** (1/3.0) and 1 - coefficientMask, on the device's X, Y and HMask."""
    from gcc_nmf_amd.realtime import GCCNMFProcessor
    ws, K, D, Tc, Ls = 512, 96, 40, 4, 10
    rng = np.random.RandomState(2)
    W = R.make_rt_dictionary(5, ws // 2 + 1, K)
    F = ws // 2 + 1
    hin, hout, hmask = R.CircularHistory((F, Ls)), R.CircularHistory((F, Ls)), {K: R.CircularHistory((K, Ls))}
    dev = GCCNMFProcessor(16000, ws, Tc, {'Pretrained': {K: W}}, 'Pretrained', K, 0, 0.1, False, 6, inputSpectrogramHistory=hin,
                          outputSpectrogramHistory=hout, coefficientMaskHistories=hmask, numTDOAs=D)
    ora = R.GCCNMFProcessorOracle(16000, ws, Tc, W, 0.1, D, localizationEnabled=False)
    for p in (dev, ora):
        p.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
    for call in range(2):
        frames = (rng.standard_normal((2, ws, Tc)) * 0.1).astype(np.float32)
        dev.processFrames(frames)
        ref, im = ora.processFrames(frames, return_intermediates=True)
        cols = slice(call * Tc, (call + 1) * Tc)
        want_in = -np.mean(np.abs(im['X']), axis=0) ** (1 / 3.0)
        assert np.abs(hin.values[:, cols] - want_in).max() < 1e-5 * np.abs(want_in).max()
        Y = im['tfMask'] * im['X']
        want_out = -np.nanmean(np.abs(Y), axis=0) ** (1 / 3.0)
        assert np.abs(hout.values[:, cols] - want_out).max() < 2e-3 * np.abs(want_out).max()       # soft mask through the arg-max
        d = dev.intermediates()
        assert np.array_equal(hmask[K].values[:, cols], (1 - d['HMask']).astype(np.float64))
        assert np.abs(hmask[K].values[:, cols] - (1 - im['HMask'])).mean() < 1e-3
    assert hin.index == 2 * Tc and hmask[K].index == 2 * Tc
    # separation off: the output history mirrors the input spectrogram (:213-214), the mask history is not touched (:207-212)
    dev.separationEnabled = False
    dev.processFrames(frames)
    assert np.array_equal(hout.values[:, 2 * Tc:3 * Tc], hin.values[:, 2 * Tc:3 * Tc]) and hmask[K].index == 2 * Tc


def test_output_delay_must_cover_the_synthesis_window():
    """outputDelayBlocks = 1 with the symmetric sqrt-hamming window would hand out partial overlap-add sums."""
    from gcc_nmf_amd.realtime import GCCNMFProcessor, StreamingGCCNMF, asymmetricWindows
    ws, hop, K, D = 512, 64, 64, 32
    W = R.make_rt_dictionary(2, ws // 2 + 1, K)
    sym = GCCNMFProcessor(16000, ws, 1, {'Pretrained': {K: W}}, 'Pretrained', K, 0, 0.1, False, 6, numTDOAs=D)
    with pytest.raises(ValueError, match='before it is complete'):
        StreamingGCCNMF(sym, hop, hop, outputDelayBlocks=1)
    StreamingGCCNMF(sym, hop, hop, outputDelayBlocks=2)                       # the reference's own hand-out, pinned by the goldens
    StreamingGCCNMF(sym, hop, hop, outputDelayBlocks=7)                       # 7 * 64 + 64 = 512: complete
    a, sy = asymmetricWindows(ws, 2 * hop)
    asym = GCCNMFProcessor(16000, ws, 1, {'Pretrained': {K: W}}, 'Pretrained', K, 0, 0.1, False, 6, numTDOAs=D, analysisWindow=a, synthesisWindow=sy)
    StreamingGCCNMF(asym, hop, hop, outputDelayBlocks=1)


def test_reset_invalidates_the_captured_graph():
    """reset() re-allocates every device buffer; the graph key carries the processor's generation, so a replay never
    touches freed memory even if the allocator hands the old addresses out again."""
    from gcc_nmf_amd.realtime import GCCNMFProcessor, StreamingGCCNMF
    ws, hop, K, D = 512, 64, 64, 32
    W = R.make_rt_dictionary(3, ws // 2 + 1, K)
    x = O.synthetic_mixture(9, numSamples=40 * hop, delays=(-3, 1, 4))
    p = GCCNMFProcessor(16000, ws, 1, {'Pretrained': {K: W}}, 'Pretrained', K, 0, 0.1, False, 6, numTDOAs=D)
    s = StreamingGCCNMF(p, hop, hop)
    first = [s.process_block(x[:, b * hop:(b + 1) * hop]) for b in range(20)]
    key0 = s._graph_key
    for _ in range(2):
        p.reset()
    s2 = StreamingGCCNMF(p, hop, hop)
    s2._pin_in, s2._pin_out, s2._ev_out, s2._graph, s2._graph_key = s._pin_in, s._pin_out, s._ev_out, s._graph, s._graph_key
    again = [s2.process_block(x[:, b * hop:(b + 1) * hop]) for b in range(20)]
    assert s2._graph_key != key0 and s2.capture_error is None
    assert all(np.array_equal(a, b) for a, b in zip(first, again))


# ---- low-latency extensions (BASELINE config 5; no reference code exists for them: oracle "parity unpinned") --------------------
@pytest.mark.parametrize('ws,K,D,Tc,n', [(512, 256, 64, 1, 1), (512, 1024, 64, 1, 3), (256, 96, 33, 4, 2)])
def test_coefficient_inference_and_asymmetric_windows_match_oracle(ws, K, D, Tc, n):
    from gcc_nmf_amd.realtime import GCCNMFProcessor, asymmetricWindows
    a, sy = asymmetricWindows(ws, ws // 4)
    W = R.make_rt_dictionary(21, ws // 2 + 1, K)
    dev = GCCNMFProcessor(16000, ws, Tc, {'Pretrained': {K: W}}, 'Pretrained', K, n, 0.1, False, 6, numTDOAs=D, analysisWindow=a,
                          synthesisWindow=sy)
    ora = R.GCCNMFProcessorOracle(16000, ws, Tc, W, 0.1, D, localizationEnabled=False, numHUpdates=n, analysisWindow=a, synthesisWindow=sy)
    rng = np.random.RandomState(8)
    compared = total = 0
    for params in [(9.6, 5.0, 2.0, 0.0), (20.0, 3.0, 1.0, 0.2)]:
        dev.setTargetTDOARange(*params)
        ora.setTargetTDOARange(*params)
        frames = (rng.standard_normal((2, ws, Tc)) * 0.1).astype(np.float32)
        out = dev.processFrames(frames)
        ora_c = copy.deepcopy(ora)
        ref, im = ora.processFrames(frames, return_intermediates=True)
        d = dev.intermediates()
        assert np.abs(d['X'] - im['X']).max() < 1e-5 * np.abs(im['X']).max()
        same = d['argmaxTDOA'] == im['argmaxTDOA']
        assert same.mean() > 0.995
        assert d['tfMask'].shape == (2, ws // 2 + 1, Tc)
        # the mask and output stages under the device's own arg-max, on every frame
        ref_c, im_c = ora_c.processFrames(frames, return_intermediates=True, argmax_override=d['argmaxTDOA'])
        assert np.abs(d['tfMask'] - im_c['tfMask']).max() < 2e-4
        assert np.abs(out - ref_c).max() < 2e-4 * np.abs(ref_c).max()
        # ... and against the oracle's own run on every frame where no atom flipped
        ok = same.all(axis=0)
        compared, total = compared + int(ok.sum()), total + ok.size
        assert maxabs(d['tfMask'][..., ok] - im['tfMask'][..., ok]) < 2e-4
        assert maxabs(out[..., ok] - ref[..., ok]) < 2e-4 * np.abs(ref).max()
    assert 2 * compared > total, (compared, total)


def test_low_latency_stream_is_the_identity_one_block_late_when_separation_is_off():
    from gcc_nmf_amd.realtime import GCCNMFProcessor, StreamingGCCNMF, asymmetricWindows
    ws, hop, K, D = 512, 64, 64, 32
    a, sy = asymmetricWindows(ws, 2 * hop)
    W = R.make_rt_dictionary(2, ws // 2 + 1, K)
    dev = GCCNMFProcessor(16000, ws, 1, {'Pretrained': {K: W}}, 'Pretrained', K, 2, 0.1, False, 6, numTDOAs=D, analysisWindow=a, synthesisWindow=sy)
    dev.separationEnabled = False
    x = (np.random.RandomState(4).standard_normal((2, 60 * hop)) * 0.05).astype(np.float32)
    y = StreamingGCCNMF(dev, hop, hop, outputDelayBlocks=1).process_stream(x)
    assert np.abs(y[:, 9 * hop:] - x[:, 8 * hop:-hop]).max() < 1e-5
    # and with separation on: the device stream against the oracle stream, same windows, delay and coefficient updates
    dev.separationEnabled = True
    dev.reset()
    dev.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
    ora = R.GCCNMFProcessorOracle(16000, ws, 1, W, 0.1, D, localizationEnabled=False, numHUpdates=2, analysisWindow=a, synthesisWindow=sy)
    ora.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
    ola = R.OverlapAddOracle(2, ws, hop, hop, 1, outputDelayBlocks=1)
    xs = O.synthetic_mixture(6, numSamples=60 * hop, delays=(-3, 1, 4))
    yd = StreamingGCCNMF(dev, hop, hop, outputDelayBlocks=1).process_stream(xs)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        yr = np.concatenate([ola.processFrames(xs[:, b * hop:(b + 1) * hop], ora.processFrames) for b in range(60)], axis=1)
    assert np.abs(yd - yr).max() < 5e-4 * np.abs(xs).max()


def test_graph_replay_equals_direct_launches():
    """process_block replays a captured HIP graph (upload, kernels, download); it must produce exactly what the direct launches do,
    also across a parameter change that forces a re-capture."""
    from gcc_nmf_amd.realtime import GCCNMFProcessor, StreamingGCCNMF
    ws, hop, K, D = 512, 64, 128, 64
    W = R.make_rt_dictionary(3, ws // 2 + 1, K)
    x = O.synthetic_mixture(9, numSamples=80 * hop, delays=(-3, 1, 4))
    outs = []
    for use_graph in (False, True):
        p = GCCNMFProcessor(16000, ws, 1, {'Pretrained': {K: W}}, 'Pretrained', K, 1, 0.1, True, 6, numTDOAs=D)
        p.setTargetTDOARange(9.6, 5.0, 2.0, 0.0)
        s = StreamingGCCNMF(p, hop, hop, use_graph=use_graph)
        ys = []
        for b in range(80):
            if b == 40:
                p.targetMode = 0                       # boxcar: a different launch argument -> re-capture
            ys.append(s.process_block(x[:, b * hop:(b + 1) * hop]))
        assert (s._graph is not None) == use_graph
        outs.append(np.concatenate(ys, axis=1))
    assert np.array_equal(outs[0], outs[1])
