"""-m gpu: time-varying TDOA tracks in the offline path (GCCNMFEngine(tdoaTracking=True): the tracks mode of gccnmf_pick_tdoa_peaks and
the per-(target, frame) steering of gccnmf_target_scores_masks, csrc/gcc.hip) against the float64 NumPy restatement in
tests/tdoa_tracks_restatement.py, evaluated on the device's own angular spectrogram read back (the streaming tests' "device's own
decisions" convention).

The bar on the windowed mean is measured, not fixed: BAR_FACTOR = 4 x the largest distance of a float32 NumPy evaluation of the same
window sums from the float64 one, per input.  A frame may be left out of the exact comparison of the tracks only when the restatement's
own margin (tdoa_tracks_restatement.frame_margin) is below that bar, and at most 1 % of the frames of an input may be.  Each test prints
its figures before it asserts."""
import numpy as np
import pytest

import angular_nl_restatement as NL
import gcc_checks as C
import tdoa_tracks_restatement as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ERR_ARG = 1
FS, WS, HOP, D = 16000, 1024, 256, 128


def moving(seed, sources=False):
    from gcc_nmf_amd.synthetic import moving_source_mixture
    return moving_source_mixture(seed, returnSources=sources)


def mixture(name):
    return moving(int(name[-1])) if name.startswith('moving') else NL.load_mixture('dev1_female3_liverec_130ms_1m')[0]


def engine(n, **kw):
    from gcc_nmf_amd.engine import GCCNMFEngine
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    kw.setdefault('dictionarySize', 64)
    kw.setdefault('numIterations', 10)
    return GCCNMFEngine(n, sampleRate=FS, windowSize=WS, hopSize=HOP, numTDOAs=D, **kw)


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize('nl', [False, True], ids=['phat', 'nl'])
@pytest.mark.parametrize('name', ['moving1', 'moving2', 'dev1'])
def test_tracks_equal_the_restatement(name, nl):
    """L in {16, 48, 2T - 1} x S in {2, 3}: the device's tracks and per-frame status are the restatement's on the device's own ang, in
    every frame whose margin reaches the measured bar (at most 1 % may fall short; the L >= 2T - 1 tracks also equal the whole-file
    indexes)."""
    x = mixture(name)
    T = 1 + (x.shape[1] - WS) // HOP
    for S in (2, 3):
        for L in (16, 48, 2 * T - 1):
            e = engine(x.shape[1], numTargets=S, tdoaTracking=True, localizationWindowSize=L, gccPHATNLEnabled=nl)
            e.upload(x[None])
            e.stft()
            e.localize()
            torch.cuda.synchronize()
            ang = e.get_angular()[0][0]
            assert ang.shape == (D, T) and ang.dtype == np.float32
            bar, err, Abar = R.measured_bar(ang, L)
            want, wstatus = R.tracks_from_means(Abar, S)
            margin = np.array([R.frame_margin(Abar[:, t], S, bar) for t in range(T)])
            keep = margin >= bar
            got, gstatus = e.get_tdoa_tracks()[0], e.get_track_status()[0]
            differ = int((got != want).any(axis=0).sum())
            print('%s %s S = %d L = %d: windowed mean in [%.1f, %.1f], float32 NumPy error %.3g -> bar %.3g; smallest margin %.3g, frames left '
                  'out %d of %d, short frames %d, frames that differ %d' % (name, 'nl' if nl else 'phat', S, L, Abar.min(), Abar.max(), err, bar,
                                                                            margin.min(), int((~keep).sum()), T, int(wstatus.sum()), differ))
            assert bar > 0 and (~keep).sum() <= 0.01 * T, 'the input leaves too many frames to the bar'
            assert got.shape == (S, T) and gstatus.shape == (T,)
            assert np.array_equal(got[:, keep], want[:, keep]) and np.array_equal(gstatus[keep], wstatus[keep])
            if L == 2 * T - 1:
                idx = e.get_tdoa_indexes()[0]
                assert np.array_equal(got, np.repeat(idx[:, None], T, axis=1)) and not gstatus.any()
            # the padding of the device images stays zero
            assert not e.tracks[:, :, T:].any() and not e.track_status[:, T:].any()


def test_hand_built_spectrograms_through_the_library():
    """Short frames, leading frames, ties, truncated windows and files longer than one 256-frame step of the carry scan, through
    estimateTargetTDOATracksFromAngularSpectrogram: exactly the restatement; no complete frame anywhere is a ValueError."""
    from gcc_nmf_amd import gccNMFFunctions as G
    rng = np.random.RandomState(11)
    for Dn, T, S, L in [(12, 8, 2, 1), (12, 700, 2, 1), (33, 257, 3, 5), (64, 513, 2, 4), (128, 300, 4, 48), (200, 65, 1, 1000), (3, 5, 1, 2)]:
        A = np.zeros((Dn, T), np.float32)
        for t in range(T):
            n = rng.randint(0, S + 2) if t > 2 else 0                       # leading frames without peaks, then 0 .. S + 1 peaks a frame
            pos = rng.choice(np.arange(1, Dn - 1, 2), size=min(n, (Dn - 1) // 2), replace=False)
            A[pos, t] = rng.choice([1.0, 2.0, 3.0], size=len(pos))          # few heights: ties at the S boundary are common
        if L == 1 and T > 600:
            A[:, 200:520] = 0                                               # a gap longer than one scan step: the carry crosses it
        A[1, T - 1] = 4.0
        if S > 1:
            A[3 if Dn > 4 else 1, T - 1] = 5.0
        try:
            want, wstatus, _ = R.tdoa_tracks(A, S, L)
        except ValueError:
            want = None
        if want is None:
            with pytest.raises(ValueError, match='enough peaks'):
                G.estimateTargetTDOATracksFromAngularSpectrogram(A, 1.0, Dn, S, L)
            continue
        got = G.estimateTargetTDOATracksFromAngularSpectrogram(A.astype(np.float64), 1.0, Dn, S, L)
        print('D = %d T = %d S = %d L = %d: %d short frames' % (Dn, T, S, L, int(wstatus.sum())))
        assert got.dtype == np.int64 and np.array_equal(got, want), (Dn, T, S, L)
    with pytest.raises(ValueError, match='enough peaks'):
        G.estimateTargetTDOATracksFromAngularSpectrogram(np.zeros((16, 40)), 1.0, 16, 2, 8)


def test_malformed_mode_bits_are_argument_errors_and_write_nothing():
    from gcc_nmf_amd import _hip
    lib = _hip.lib()
    e = engine(32000, numTargets=2, tdoaTracking=True, localizationWindowSize=8)
    e.upload(moving(1)[None, :, :32000])
    e.stft()
    e.localize()
    torch.cuda.synchronize()
    g = e.g
    tracks = torch.full((2, g.Tp), -7, dtype=torch.int32, device='cuda')
    status = torch.full((g.Tp,), -7, dtype=torch.int32, device='cuda')
    call = lambda S, T=g.T, Dn=g.D: lib.gccnmf_pick_tdoa_peaks(e.ang.data_ptr(), Dn, T, S, 1, tracks.data_ptr(), status.data_ptr(), stream())
    for S in (2 | (8 << 9), 2 | 0x100, 0x100 | (8 << 9), -(1 << 31) | 2 | 0x100 | (8 << 9), -1):       # L without the bit, L = 0, S = 0, sign bit
        assert call(S) == ERR_ARG, hex(S & 0xffffffff)
    assert call(2 | 0x100 | (8 << 9), T=0) == ERR_ARG and call(2 | 0x100 | (8 << 9), T=1 << 21) == ERR_ARG
    assert call(2 | 0x100 | (8 << 9), Dn=2) == ERR_ARG and call(2 | 0x100 | (8 << 9), Dn=4097) == ERR_ARG
    scores = torch.full((g.Kp, 2 * g.Tp), -7.0, dtype=torch.float32, device='cuda')
    for S in (2 | 0x200, 2 | 0x300, 2 | (1 << 16), 0x100, -2):
        assert lib.gccnmf_target_scores_masks(e.CC.data_ptr(), e.trig.data_ptr(), e.tracks.data_ptr(), e.W0.data_ptr(), g.F, g.T, g.K, g.D, S, 1,
                                              e.ws_scores.data_ptr(), scores.data_ptr(), 0, stream()) == ERR_ARG, hex(S & 0xffffffff)
    torch.cuda.synchronize()
    assert (tracks == -7).all() and (status == -7).all() and (scores == -7).all()
    assert call(2 | 0x100 | (8 << 9)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(tracks[:, :g.T].cpu().numpy(), e.get_tdoa_tracks()[0]) and (tracks[:, g.T:] == -7).all()


@pytest.mark.parametrize('nl', [False, True], ids=['phat', 'nl'])
def test_scores_and_argmax_with_per_frame_indexes(nl):
    """G_i[k, t] = Re sum_f W[f, k] C[f, t] e^{-j 2 pi f tau_{i, t}} on the device's own C, W and tracks: within the existing score bound
    (tests/gcc_checks.py) of the float64 evaluation; the arg-max is numpy.nanargmax of the device's scores exactly, and the float64
    arg-max except where the float64 scores' two best targets are closer than the two bounds (the existing near-tie rule)."""
    x = moving(1)
    e = engine(x.shape[1], numTargets=2, tdoaTracking=True, localizationWindowSize=48, gccPHATNLEnabled=nl, numIterations=30)
    e.separate(x[None])
    g = e.g
    tracks = e.get_tdoa_tracks()[0]
    assert len(np.unique(tracks[0])) >= 2, 'the moving talker must move'
    Cd, Wd = e.get_C()[0], e.get_WH()[0][0]
    G, Gabs = R.target_scores(Cd, Wd, e.frequenciesInHz, e.tdoasInSeconds, tracks)
    scores = e.get_scores()[0]
    err = np.abs(scores - G)
    print('scores in [%.2f, %.2f]: largest distance from float64 %.3g, smallest bound %.3g, largest error / bound %.3g'
          % (G.min(), G.max(), err.max(), C.gemm_bound(Gabs, g.F).min(), (err / C.gemm_bound(Gabs, g.F)).max()))
    for i in range(2):
        C.check_gemm_like(scores[i], G[i], Gabs[i], g.F, what='scores, target %d' % i)
    # a frame after the jump really uses the other column: the fixed-index scores differ there
    fixed, _ = R.target_scores(Cd, Wd, e.frequenciesInHz, e.tdoasInSeconds, np.repeat(tracks[:, :1], g.T, axis=1))
    assert np.abs(fixed[0, :, -50:] - G[0, :, -50:]).max() > 100 * C.gemm_bound(Gabs, g.F)[0, :, -50:].max()
    am = e.get_argmax()[0]
    C.check_argmax(am, scores, what='arg-max of the device scores')
    flips = am != np.nanargmax(G, axis=0)
    gap = np.abs(G[0] - G[1])
    allowed = gap <= C.gemm_bound(Gabs[0], g.F) + C.gemm_bound(Gabs[1], g.F)
    print('arg-max: %d of %d positions differ from float64, all near-ties: %s' % (flips.sum(), flips.size, bool(np.all(allowed[flips]))))
    assert np.all(allowed[flips]) and flips.mean() < 5e-3


@pytest.mark.parametrize('reconstruction', ['direct', 'ratio'])
@pytest.mark.parametrize('name', ['moving1', 'dev1'])
def test_whole_file_window_is_the_static_path_bit_for_bit(name, reconstruction):
    x = mixture(name)
    T = 1 + (x.shape[1] - WS) // HOP
    S = 2 if name.startswith('moving') else 3
    kw = dict(numTargets=S, reconstruction=reconstruction)
    e0, e1 = engine(x.shape[1], **kw), engine(x.shape[1], tdoaTracking=True, localizationWindowSize=2 * T - 1, **kw)
    e2 = engine(x.shape[1], tdoaTracking=True, localizationWindowSize=10 * T, **kw)
    y0, y1, y2 = e0.separate(x[None]), e1.separate(x[None]), e2.separate(x[None])
    assert np.array_equal(e1.get_tdoa_tracks()[0], np.repeat(e0.get_tdoa_indexes()[0][:, None], T, axis=1))
    assert np.array_equal(e0.get_tdoa_indexes(), e1.get_tdoa_indexes())
    for e, y in ((e1, y1), (e2, y2)):
        assert np.array_equal(e.get_scores(), e0.get_scores()) and np.array_equal(e.get_argmax(), e0.get_argmax())
        assert np.array_equal(e.get_spec(), e0.get_spec()) and np.array_equal(y, y0)
    assert np.abs(y0).max() > 1e-3


def test_a_file_alone_in_a_batch_and_in_a_ragged_batch():
    """The same file alone, at both ends of a batch of 5 and in a ragged batch: identical tracks, status and spec.  (The blind KL-NMF
    of ONE file sums in another order than a batch's -- include/gccnmf_hip.h -- so every engine is handed the factors of the file alone;
    everything this feature touches runs per engine.)"""
    from gcc_nmf_amd.engine import GCCNMFEngine
    x = moving(1)
    n, n_short = x.shape[1], 64000
    others = [moving(s) for s in (2, 3, 4)]
    kw = dict(numTargets=2, tdoaTracking=True, localizationWindowSize=48)
    e1 = engine(n, **kw)
    e1.separate(x[None])
    tracks, status, spec = e1.get_tdoa_tracks()[0], e1.get_track_status()[0], e1.get_spec()[0]
    assert len(np.unique(tracks[0])) >= 2 and np.abs(spec).max() > 0

    def finish(e, rows):
        for k in rows:
            e.W[k].copy_(e1.W[0])
            e.H[k].copy_(e1.H[0])
        e.localize()
        e.masks()
        e.reconstruct()
        torch.cuda.synchronize()

    e5 = engine(n, batch=5, **kw)
    e5.upload(np.stack([x] + others + [x]))
    e5.stft()
    e5.klnmf()
    finish(e5, (0, 4))
    for k in (0, 4):
        assert np.array_equal(e5.get_tdoa_tracks()[k], tracks) and np.array_equal(e5.get_track_status()[k], status), k
        assert np.array_equal(e5.get_spec()[k], spec), k
    assert not np.array_equal(e5.get_tdoa_tracks()[1], tracks)
    files = [x, others[0][:, :n_short], others[1], x, others[2][:, :n_short]]
    r = GCCNMFEngine(lengths=[f.shape[1] for f in files], sampleRate=FS, windowSize=WS, hopSize=HOP, numTDOAs=D, dictionarySize=64,
                     numIterations=10, **kw)
    assert all(sub.tdoaTracking and sub.localizationWindowSize == 48 for sub in r.sub.values())
    r.upload(files)
    for sub in r.sub.values():
        sub.stft()
    r.klnmf()
    sub = r.sub[n]
    finish(sub, (r.file(0)[1], r.file(3)[1]))
    for i in (0, 3):
        k = r.file(i)[1]
        assert np.array_equal(sub.get_tdoa_tracks()[k], tracks) and np.array_equal(sub.get_spec()[k], spec), i
    # each file's windows end at its own T: a short file's tracks are those of an engine of its length
    short = r.sub[n_short]
    short.localize()
    torch.cuda.synchronize()
    es = engine(n_short, **kw)
    es.upload(files[1][None])
    es.stft()
    es.localize()
    got = r.get_tdoa_tracks()
    assert [t.shape for t in got] == [(2, 1 + (f.shape[1] - WS) // HOP) for f in files]
    assert np.array_equal(got[1], es.get_tdoa_tracks()[0]) and np.array_equal(r.get_track_status()[1], es.get_track_status()[0])


@pytest.mark.parametrize('seed', [1, 2])
def test_tracking_recovers_the_talker_who_changed_seat(seed):
    """THE test that fails without the feature.  Moving mixture, K = 64, 60 iterations, L = 48: after the jump the static path scores
    source 1 against the direction it has left; with tracking its second-half SDR is at least 3 dB higher (the float64 CPU pipeline
    gives +4.9 dB for both seeds), and the first-half SDRs of both sources stay within 0.5 dB of the static path's (CPU: 0.0).
    Left-channel image SDR per half, output delayed by windowSize / 2, 4000 samples left out around the ends and the jump.
    The float64 CPU pipeline (oracle + restatement): seed 1 static 1.6 -> tracked 6.5 dB, seed 2 static 1.3 -> 6.2 dB, first halves
    identical; the device's values are printed before the assertions (DESIGN section 4b records them)."""
    x, images = moving(seed, sources=True)
    n = x.shape[1]
    kw = dict(numTargets=2, dictionarySize=64, numIterations=60)
    e0, e1 = engine(n, **kw), engine(n, tdoaTracking=True, localizationWindowSize=48, **kw)
    y0, y1 = e0.separate(x[None])[0], e1.separate(x[None])[0]
    assert e0.get_tdoa_indexes()[0].tolist() == [56, 97]
    # targets are numbered from the left: target 0 is the moving talker (source 1, index 56 / 57 then 23), target 1 the static one (97)
    sdr = {}
    for label, y in (('static', y0), ('tracked', y1)):
        for src, target in ((0, 1), (1, 0)):
            sdr[label, src, 1] = R.image_sdr(y[target, 0], images[src], WS, 0, n // 2)
            sdr[label, src, 2] = R.image_sdr(y[target, 0], images[src], WS, n // 2, n - WS)
        print('seed %d %-7s src0 h1 %.2f h2 %.2f   src1 h1 %.2f h2 %.2f dB'
              % (seed, label, sdr[label, 0, 1], sdr[label, 0, 2], sdr[label, 1, 1], sdr[label, 1, 2]))
    tr = e1.get_tdoa_tracks()[0]
    print('seed %d tracks: moving talker %s -> %s, static talker %s; short frames %d'
          % (seed, np.unique(tr[0, :130]), np.unique(tr[0, 240:]), np.unique(tr[1]), int(e1.get_track_status().sum())))
    assert sdr['tracked', 1, 2] - sdr['static', 1, 2] >= 3.0
    for src in (0, 1):
        assert abs(sdr['tracked', src, 1] - sdr['static', src, 1]) <= 0.5, src


def test_dropin_functions_agree_with_the_engine():
    from gcc_nmf_amd import gccNMFFunctions as G
    x = moving(2)
    e = engine(x.shape[1], numTargets=2, tdoaTracking=True, localizationWindowSize=48)
    e.separate(x[None])
    ang, Cd, (W, H) = e.get_angular()[0][0], e.get_C()[0], e.get_WH()
    tracks = G.estimateTargetTDOATracksFromAngularSpectrogram(ang, 1.0, D, 2, 48)
    assert tracks.shape == (2, e.g.T) and np.array_equal(tracks, e.get_tdoa_tracks()[0])
    stereoH = np.array(np.hsplit(H[0], 2))
    Gt = G.getTargetTDOAGCCNMFs(Cd, 1.0, D, e.frequenciesInHz, tracks, W[0], stereoH)
    assert Gt.shape == (2, 64, e.g.T) and Gt.dtype == np.float32 and np.array_equal(Gt, e.get_scores()[0])
    # the 1-D form is what it was: constant 2-D tracks give its bits
    idx = [int(i) for i in e.get_tdoa_indexes()[0]]
    G1 = G.getTargetTDOAGCCNMFs(Cd, 1.0, D, e.frequenciesInHz, idx, W[0], stereoH)
    G2 = G.getTargetTDOAGCCNMFs(Cd, 1.0, D, e.frequenciesInHz, np.repeat(np.array(idx)[:, None], e.g.T, axis=1), W[0], stereoH)
    assert np.array_equal(G1, G2) and not np.array_equal(G1, Gt)
    masks = G.getTargetCoefficientMasks(Gt, 2)
    assert np.array_equal(np.argmax(masks, axis=0), e.get_argmax()[0])


def test_tracking_through_every_way_in():
    """separate_batches, separate_pcm16, a fixed dictionary and the ratio mask with tracking on: the same tracks and the waveforms of
    separate(); a file without enough peaks in any frame is the ValueError the static path raises."""
    x = moving(1)
    n = x.shape[1]
    kw = dict(numTargets=2, tdoaTracking=True, localizationWindowSize=48)
    e = engine(n, **kw)
    y = e.separate(x[None])
    tracks = e.get_tdoa_tracks()
    out = list(e.separate_batches([x[None], x[None], x[None]]))
    assert len(out) == 3 and all(np.array_equal(o, y) for o in out) and np.array_equal(e.get_tdoa_tracks(), tracks)
    pcm = np.round(x.T * 32768).astype(np.int16)
    p = e.separate_pcm16(pcm[None])
    assert p.shape == (1, 2, e.L, 2) and p.dtype == np.int16 and np.array_equal(e.get_tdoa_tracks(), tracks)
    W = e.get_WH()[0][0]
    ef = engine(n, dictionaryW=W, dictionarySize=None, reconstruction='ratio', **kw)
    yf = ef.separate(x[None])
    assert np.array_equal(ef.get_tdoa_tracks(), tracks) and np.isfinite(yf).all() and np.abs(yf).max() > 1e-3
    spec = ef.get_spec()[0]
    X = ef.get_X()[0]
    assert np.abs(spec.sum(axis=0) - X).max() <= 1e-5 * np.abs(X).max()          # the ratio targets still add up to the mixture
    silent = engine(n, **kw)
    with pytest.raises(ValueError, match='fewer than 2 angular-spectrum peaks'):
        silent.separate(np.zeros((1, 2, n), np.float32))
    assert (silent.get_track_status() == 3).all() and (silent.get_tdoa_tracks() == -1).all()
