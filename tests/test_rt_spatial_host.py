"""CPU: the online spatial filter of the real-time path (GCCNMF_RT_SEPARATION_SPATIAL, csrc/rt_spatial.hip) without a device.

  the stage layer    the separation word that reaches the C ABI (a recording stub, as in test_stage_words_host.py), the checks that come
                     before the library, the state helpers and the settings' validation
  the library        the argument rules of the carrier, decided before any HIP call (as in test_rt_host.py)
  the restatement    tests/rt_spatial_restatement.py: the consequences of the contract, and that the measured bar sees each of four planted
                     mistakes on every cell of tests/rt_spatial_cells.py where the mistake changes anything -- evaluated on
                     rt_checks.model32's Y and X, the float32 restatement of the call in front of the filter
  the condition      outside the rank-deficient cell every cell's bar is below 1e-4, so that an identity covariance fails
"""
import numpy as np
import pytest

import rt_checks as R
import rt_spatial_cells as SC
import rt_spatial_restatement as RS
import spatial_restatement as SR
from test_stage_words_host import StubLibrary, last, RT_POINTERS, RT_GEOMETRY, STREAM, BANK, MULTI, ROW8

ARG = 1
SEPARATION = 32                                              # separation_enabled's place in gccnmf_rt_process_block_ll's argument list


@pytest.fixture
def stub(monkeypatch):
    from gcc_nmf_amd import _hip
    lib = StubLibrary()
    monkeypatch.setattr(_hip, '_lib', lib)
    return lib


def rt_call(target_mode, separation=True, **mode):
    from gcc_nmf_amd import _hip
    _hip.rt_process_block(*RT_POINTERS, *RT_GEOMETRY, target_mode, separation, False, 6, 3, 1, stream=STREAM, **mode)


# ---- the stage layer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,word', [(dict(nl_row=True), ROW8), (dict(streams=3), BANK | 2 << 8), (dict(targets=3), MULTI | 2 << 21),
                                       (dict(streams=2, targets=8, localize='skip'), 2 | BANK | 1 << 8 | MULTI | 7 << 21),
                                       (dict(nl_row=True, frames=True), ROW8 | 1)], ids=lambda v: None if isinstance(v, int) else ' '.join(v))
def test_the_separation_word(stub, mode, word):
    from gcc_nmf_amd import _hip
    assert _hip.RT_SEPARATION_SPATIAL == SC.SPATIAL == 2
    target_mode = _hip.TARGET_MODE_MULTIPLE if 'targets' in mode else _hip.TARGET_MODE_WINDOW_FUNCTION
    for spatial, separation, want in ((True, True, 3), (False, True, 1), (True, False, 0), (False, False, 0), (True, 5, 3)):
        rt_call(target_mode, separation, spatial=spatial, **mode)
        args = last(stub, 'gccnmf_rt_process_block_ll')
        assert args[SEPARATION] == want and args[35] == word
        assert args[:SEPARATION] + args[SEPARATION + 1:35] + args[36:] == RT_POINTERS + RT_GEOMETRY + (target_mode, 0, 6, 3, 1, STREAM)
    rt_call(target_mode, **mode)                             # the keyword's default: the word every caller passed before
    assert last(stub, 'gccnmf_rt_process_block_ll')[SEPARATION] == 1


def test_the_filter_needs_a_row_with_word_7(stub):
    from gcc_nmf_amd import _hip
    for mode in ({}, dict(frames=True), dict(localize='skip')):
        with pytest.raises(ValueError):
            rt_call(_hip.TARGET_MODE_WINDOW_FUNCTION, spatial=True, **mode)
        with pytest.raises(ValueError):                      # ... whether or not the separation is on
            rt_call(_hip.TARGET_MODE_BOXCAR, False, spatial=True, **mode)
    assert stub.calls == []


def test_state_helpers_and_settings():
    from gcc_nmf_amd import _hip, realtime as rt
    assert _hip.rt_spatial_state_floats(257, 2, 1) == 4 * 2 * 257 and _hip.rt_spatial_state_floats(33, 8, 256) == 4 * 256 * 8 * 33
    assert _hip.rt_spatial_state_floats(33, 3) == 4 * 3 * 33
    for D, Lh, S, want in ((64, 128, 1, 8192), (33, 5, 1, 168), (33, 5, 3, 496), (1, 1, 1, 4), (3, 3, 3, 28), (64, 128, 256, 64 * 128 * 256)):
        assert _hip.rt_spatial_state_offset(D, Lh, S) == want and want % 4 == 0 and 0 <= want - S * D * Lh < 4
    assert _hip.check_spatial_filter(False, 16) == (False, 16.0) and _hip.check_spatial_filter(1, np.float32(1.0)) == (True, 1.0)
    assert _hip.check_spatial_filter(True, 1e6) == (True, 1e6)
    assert _hip.check_spatial_filter(False, _hip.DEFAULT_SPATIAL_FILTER_FRAMES)[1] == _hip.DEFAULT_SPATIAL_FILTER_FRAMES
    W = np.ones((513, 8), np.float32)
    for bad in (0, 0.5, -4, float('nan'), float('inf'), 1e39, None, '8', True, 1 - 1e-9):
        for enabled in (False, True):
            with pytest.raises(ValueError):
                _hip.check_spatial_filter(enabled, bad)
        with pytest.raises(ValueError):                      # the constructor checks before it looks for a device
            rt.GCCNMFProcessor(16000, 1024, 1, {'P': {8: W}}, 'P', 8, 0, 0.1, True, 6, spatialFilterFrames=bad)
        p = object.__new__(rt.GCCNMFProcessor)               # attributes set later are checked by the next call through the same helper
        p.spatialFilterEnabled, p.spatialFilterFrames = True, bad
        with pytest.raises(ValueError):
            p._spatial_word()
    p = object.__new__(rt.GCCNMFProcessor)
    p.spatialFilterEnabled, p.spatialFilterFrames = False, 8
    assert p._spatial_word() == 0.0                          # word 7 of the target row: 0 = off
    p.spatialFilterEnabled = True
    assert p._spatial_word() == 8.0 and p._spatial_word().dtype == np.float32
    bk = object.__new__(rt.StreamingGCCNMFBank)              # the bank's per-stream setter checks before it touches the device
    bk.numStreams, bk.device = 2, 'cpu'
    with pytest.raises(ValueError):
        rt.StreamingGCCNMFBank.setSpatialFilter.__wrapped__(bk, 0, True, 0.25)
    with pytest.raises(IndexError):
        rt.StreamingGCCNMFBank.setSpatialFilter.__wrapped__(bk, 2, True, 8)
    import inspect
    params = inspect.signature(rt.GCCNMFProcessor.__init__).parameters
    assert params['spatialFilterEnabled'].default is False and params['spatialFilterFrames'].default == _hip.DEFAULT_SPATIAL_FILTER_FRAMES


# ---- the library: every rule of the carrier is decided before any HIP call ----------------------------------------------------------------
P = 4096
POINTERS = ('block_in', 'block_out', 'in_ring', 'out_ring', 'X', 'Y', 'C', 'HMask', 'argmaxTDOA', 'tfMask', 'hist', 'hist_pos', 'target', 'gccphat',
            'W', 'cosT', 'sinT', 'window', 'synthesis_window', 'twiddle', 'colsumW', 'Hcoef', 'Rv')
INTS = dict(windowSize=1024, hopSize=256, blockSize=512, K=100, Kp=128, D=33, Dp=64, numTDOAHistory=16, target_mode=2, separation_enabled=3,
            localization_enabled=1, localization_window=6, frames_mode=0, numHUpdates=0, out_delay_blocks=2)


@pytest.fixture(scope='module')
def call():
    from gcc_nmf_amd import _hip
    fn = _hip.lib().gccnmf_rt_process_block_ll

    def call(**kw):
        ptrs = [kw.pop(k, P) for k in POINTERS]
        ints = dict(INTS)
        for k in list(kw):
            assert k in ints, k
            ints[k] = kw.pop(k)
        return fn(*ptrs, *[ints[k] for k in INTS], None)
    return call


def test_the_filter_bit_with_a_4_word_row_is_an_argument_error(call):
    for bits in (0, 1, 2, 4, 1 | 4):                         # streaming, frames mode, without / only the localisation
        for sep in (3, 2, 7, -1):                            # bit 1, with whatever else
            assert call(frames_mode=bits, separation_enabled=sep) == ARG, (bits, sep)


def test_the_filter_bit_with_a_row_that_has_word_7_still_checks_everything(call):
    layouts = ((ROW8, 2), (BANK | (2 << 8), 2), (MULTI | (2 << 21), 1), (BANK | (255 << 8) | MULTI | (7 << 21), 1), (ROW8 | 1, 0))
    for bits, mode in layouts:
        for bad in (dict(windowSize=1023), dict(Kp=100), dict(D=0), dict(localization_window=17), dict(out_delay_blocks=0), dict(X=0),
                    dict(hist=0), dict(numHUpdates=-1)):
            assert call(frames_mode=bits, target_mode=mode, **bad) == ARG, (hex(bits), bad)
        assert call(frames_mode=bits, target_mode=mode, hist=P + 4) == ARG          # the state behind hist is read as float4
        assert call(frames_mode=bits, target_mode=mode, hist=P + 8) == ARG
    assert call(frames_mode=ROW8 | BANK) == ARG and call(frames_mode=1 << 25) == ARG    # the frames_mode word keeps its rules


# ---- the restatement: consequences of the contract -------------------------------------------------------------------------------------------
def random_call(N, F, T, seed, multi=True):
    """Random masked spectra that add up to X (as the one-hot masks make them), X and a random state."""
    rng = np.random.RandomState(seed)
    X = ((rng.standard_normal((2, F, T)) + 1j * rng.standard_normal((2, F, T))) * 3).astype(np.complex64)
    if multi:
        m = rng.dirichlet(np.ones(N), size=(F, T)).transpose(2, 0, 1)[:, None]        # (N, 1, F, T)
        Y = (m * X[None]).astype(np.complex64)
        return Y, X, RS.random_state(N, F, seed + 1, 3.0)
    m = rng.rand(1, 1, F, T)
    return (m * X[None]).astype(np.complex64), X, RS.random_state(2, F, seed + 1, 3.0)


def test_the_outputs_of_multiple_mode_add_up_to_the_mixture():
    for N in (1, 2, 3, 8):
        Y, X, P = random_call(N, 19, 4, 10 + N)
        m = RS.measured_bar(Y, X, P, 4.0, True)
        assert np.abs(m['Y64'].sum(axis=0) - X).max() / m['scale_Y'] < 1e-12
        assert np.abs(m['Y32'].astype(np.complex128).sum(axis=0) - X).max() / m['scale_Y'] <= N * m['bar_Y'] + 2.0 ** -23
        if N == 1:                                           # one target returns the mixture, whatever the state
            assert np.abs(m['Y64'][0] - X).max() / m['scale_Y'] < 1e-12 and np.abs(m['Y32'][0] - X).max() / m['scale_Y'] <= m['bar_Y']


@pytest.mark.parametrize('multi', [False, True], ids=['single', 'multi'])
def test_swapping_the_input_channels_swaps_the_output_channels(multi):
    Y, X, P = random_call(3, 17, 3, 5, multi)
    Ps = P[..., [1, 0, 2, 3]] * np.array([1, 1, 1, -1], np.float32)                     # R -> its channel swap: p0 <-> p1, q -> conj q
    a, Pa = RS.rt_spatial(Y, X, P, 6.0, multi)
    b, Pb = RS.rt_spatial(Y[:, ::-1], X[::-1], Ps, 6.0, multi)
    assert np.abs(a - b[:, ::-1]).max() < 1e-12 * np.abs(X).max()
    assert np.array_equal(Pa[..., [1, 0, 2, 3]] * np.array([1, 1, 1, -1], np.float32), Pb)


@pytest.mark.parametrize('multi', [False, True], ids=['single', 'multi'])
def test_tau_1_has_no_memory_and_a_call_of_tc_frames_is_tc_calls_of_one(multi):
    Y, X, P = random_call(3, 17, 4, 7, multi)
    for dtype in (np.float64, np.float32):
        a, Pa = RS.rt_spatial(Y, X, P, 1.0, multi, dtype)
        b, Pb = RS.rt_spatial(Y, X, np.zeros_like(P), 1.0, multi, dtype)
        assert np.array_equal(a, b) and np.array_equal(Pa, Pb)
        c, Pc = RS.rt_spatial(Y, X, 100 * P, 7.0, multi, dtype)
        assert not np.array_equal(a, c)
        whole, Pw = RS.rt_spatial(Y, X, P, 5.0, multi, dtype)
        Pt, parts = P, []
        for t in range(X.shape[-1]):
            y, Pt = RS.rt_spatial(Y[..., t:t + 1], X[..., t:t + 1], Pt, 5.0, multi, dtype)
            parts.append(y)
        assert np.array_equal(np.concatenate(parts, axis=-1), whole) and np.array_equal(Pt, Pw)      # bit for bit


def test_identical_frames_with_tau_1_give_the_offline_covariances_of_one_frame():
    """R~ of the state then is the trace-normalised rank-1 covariance of the frame plus the loading: spatial_restatement.covariances of that
    frame, up to the one float32 rounding of the stored state (the offline sums are float64): 4 float32 ulps of the largest entry."""
    Y, X, P = random_call(3, 23, 1, 3)
    Tc = 4
    Yr, Xr = np.repeat(Y, Tc, axis=-1), np.repeat(X, Tc, axis=-1)
    out, Pn = RS.rt_spatial(Yr, Xr, P, 1.0, True)
    got = RS.loaded_covariances(Pn).astype(np.float32)
    want = SR.covariances(Y)
    assert np.abs(got.astype(np.float64) - want).max() <= 4 * 2.0 ** -23 * 2.0
    offline = SR.spatial_filter(Y, X, R=got)
    assert np.array_equal(out[..., -1], offline[..., 0])     # "exactly spatial_filter(E[..., t], X[..., t], R = R~)"


def test_a_non_finite_frame_leaves_the_state_and_only_its_own_output_non_finite():
    Y, X, P = random_call(2, 9, 3, 21, multi=False)
    Yn, Xn = Y.copy(), X.copy()
    Xn[0, :, 1], Yn[0, 0, :, 1] = np.nan, np.nan
    Xn[1, 4, 2] = np.inf
    for dtype in (np.float64, np.float32):
        out, Pn = RS.rt_spatial(Yn, Xn, P, 3.0, False, dtype)
        ref0, P0 = RS.rt_spatial(Y[..., :1], X[..., :1], P, 3.0, False, dtype)
        ref2, P2 = RS.rt_spatial(Y[..., 2:], X[..., 2:], P0, 3.0, False, dtype)     # frame 1 skipped entirely
        assert np.array_equal(out[..., 0], ref0[..., 0]) and not np.isfinite(out[0, 0, :, 1]).any()
        keep = np.arange(9) != 4
        assert np.array_equal(out[..., keep, 2], ref2[..., keep, 0]) and np.array_equal(Pn[:, keep], P2[:, keep])
        assert np.array_equal(Pn[:, 4], P0[:, 4]) and np.isfinite(Pn).all()          # the Inf bin of frame 2: its update skipped too


# ---- the bar: measured on every cell, small enough, and sensitive ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def front():
    """Every cell's inputs and the float32 restatement of the call in front of the filter (rt_checks.model32), computed once."""
    out = {}
    for sc in SC.CELLS:
        I = SC.make_inputs(sc)
        out[sc.name] = (I, R.model32(sc.c, {k: v for k, v in I.items() if k != 'spatial'}))
    return out


@pytest.mark.parametrize('sc', SC.CELLS, ids=repr)
def test_the_bar_is_small_and_sees_the_planted_mistakes(front, sc):
    I, O = front[sc.name]
    filtered = [s for s in range(sc.c.nS) if sc.filtered(s)]
    assert filtered == [0]
    for s in filtered:
        Y, X = SC.stream_io(sc, O, s)
        P, tau = I['spatial'][s], sc.taus()[s]
        m = RS.measured_bar(Y, X, P, tau, sc.c.multi)
        print('%s: float32 error Y %.3e (bar %.3e), state %.3e (bar %.3e)' % (sc.name, m['err_Y'], m['bar_Y'], m['err_P'], m['bar_P']))
        if not sc.rank_deficient:
            assert 0 < m['bar_Y'] < 1e-4 and 0 < m['bar_P'] < 1e-4
        dY, dP = RS.distance(m['Y32'], m['P32'], m)
        assert dY <= m['bar_Y'] and dP <= m['bar_P']         # sound: the float32 evaluation itself passes
        if not sc.rank_deficient:                            # an identity covariance (the loading alone) is far outside the bar
            ident = RS.rt_spatial(Y, X, P, tau, sc.c.multi, np.float32, bug='identity')[0]
            ok = np.isfinite(m['Y64'])
            d = np.abs(ident.astype(np.complex128) - m['Y64'])[ok].max() / m['scale_Y']
            assert d > 100 * m['bar_Y'] or sc.NC == 1, d
        for bug in RS.BUGS:
            if bug not in sc.applies:
                continue
            Yb, Pb = RS.rt_spatial(Y, X, P, tau, sc.c.multi, np.float32, bug=bug)
            if Pb.shape != m['P64'].shape:                   # the residual left out: one component's state
                Pb = np.concatenate([Pb, m['P32'][1:]])
            if np.array_equal(np.isfinite(Yb), np.isfinite(m['Y64'])):      # else caught already: non-finite elements in the wrong places
                dY, dP = RS.distance(Yb, Pb, m)
                assert dY > 10 * m['bar_Y'] or dP > 10 * m['bar_P'], (bug, dY, m['bar_Y'], dP, m['bar_P'])


def test_every_planted_mistake_is_seen_somewhere():
    seen = set(b for sc in SC.CELLS for b in sc.applies)
    assert seen == set(RS.BUGS)
