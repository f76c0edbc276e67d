"""-m gpu: GCCNMFArrayEngine (gcc_nmf_amd/array.py).

M = 2 is the stereo engine: with pairTDOAs = the stereo TDOA grid every buffer holds the bits of GCCNMFEngine(reconstruction='ratio',
nmf_groups=1).  (The stereo engine takes its coherence from the STFT epilogue, which no test pins bit for bit to gccnmf_coherence; the
array engine's is gccnmf_coherence's arithmetic, so the stereo engine's CC is replaced by that call on its own X before the comparison,
and whether the epilogue's bits were the same is printed.)

M = 3 (odd: the STFT's spare signal slot, a spare spectrogram slot for odd S M) and M = 4 on the line LINE, M = 5 ... 8 on an unequally
spaced eight-microphone line (tests/stacked_pairs.py: no two pair vectors equal, mixtures chosen on the host by tests/test_array_host.py),
and one call at the corner of the envelope (M = 8, n_fft = 4096), stage by stage against the float64 restatement
tests/array_restatement.py, every stage fed the device's OWN previous stage, with the element-wise bounds of gcc_checks / fft_checks:
  angular spectrogram   gemm_bound at Kd = 2 P F (cos and sin products of every pair's F bins)
  its mean              check_mean;  peaks: check_peaks, exact
  scores                gemm_bound at Kd = P F;  arg-max: check_argmax, exact on the device's own scores
  W, H                  bit-equal to a direct gccnmf_klnmf call on the engine's V
  spec                  check_gemm_like at Kd = K relative to |X| (tests/test_gpu_array_stages.py states why)
  waveforms             the float64 inverse STFT of the device's spec at the frame bar of tests/test_gpu_fft_stages.py, overlap-added
                        (array_restatement.istft states the bar)"""
import numpy as np
import pytest

import array_restatement as A
import fft_checks as K
import gcc_checks as C
import stacked_pairs as SP

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

LINE = np.array([[0.0, 0, 0], [0.2, 0, 0], [0.5, 0, 0], [1.0, 0, 0]])
SOUND = 340.29
U = 2.0 ** -24


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32) if a.dtype != torch.uint8 else a,
                                                   b.contiguous().view(torch.int32) if b.dtype != torch.uint8 else b))


def test_two_channels_are_the_stereo_engine_bit_for_bit():
    from gcc_nmf_amd import _hip
    from gcc_nmf_amd.array import GCCNMFArrayEngine
    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_batch
    n, B = 4096, 2
    xs = synthetic_batch(3, B, numSamples=n)
    kw = dict(windowSize=256, hopSize=64, numTargets=2, dictionarySize=32, numIterations=5, batch=B)
    e = GCCNMFEngine(n, numTDOAs=128, reconstruction='ratio', nmf_groups=1, **kw)
    e.upload(xs)
    e.stft()
    e.klnmf()
    epilogue = e.CC.clone()
    _hip.coherence(e.X, e.g.F, e.g.T, B, e.CC)
    torch.cuda.synchronize()
    print('the STFT epilogue\'s coherence %s gccnmf_coherence of the same X bit for bit' % ('equals' if same_bits(epilogue, e.CC) else 'differs from'))
    e.localize()
    e.masks()
    e.reconstruct()
    e.istft()
    e.check_status()
    assert not e.status.cpu().numpy().any(), 'the inputs are chosen so that the stereo engine finds its peaks'
    a = GCCNMFArrayEngine(n, numChannels=2, pairTDOAs=e.tdoasInSeconds[None], **kw)
    y = a.separate(xs)
    assert (a.P, a.Fs, a.nsig_pitch) == (1, e.g.F, 4)
    for name, mine, theirs in (('X', a.X, e.X), ('V', a.V, e.V), ('CC', a.CC, e.CC), ('W', a.W, e.W), ('H', a.H, e.H), ('trig', a.trig, e.trig),
                               ('angular spectrogram', a.ang, e.ang), ('mean', a.mean_ang.view(torch.float32), e.mean_ang.view(torch.float32)),
                               ('indexes', a.tdoa_idx, e.tdoa_idx), ('scores', a.scores, e.scores), ('arg-max', a.argmax, e.argmax),
                               ('spec', a.spec, e.spec), ('waveforms', a._y, e.y.view(B, 4, -1))):
        assert same_bits(mine, theirs), name
    assert y.shape == (B, 2, 2, a.L) and np.array_equal(y, e.y.cpu().numpy())
    assert np.isfinite(y).all() and np.abs(y).max() > 0
    assert np.array_equal(a.get_spec(), e.get_spec()) and np.array_equal(a.get_scores(), e.get_scores())
    assert np.array_equal(a.get_C()[:, 0], e.get_C())


def run_stages(M, B, S, seed, line=LINE, n=4096, n_fft=256, hop=64, Kk=32, D=61, iters=5):
    from gcc_nmf_amd import _hip
    from gcc_nmf_amd.array import GCCNMFArrayEngine, azimuthDirections
    from gcc_nmf_amd.synthetic import array_mixture
    azimuths = [40, 90, 130][:max(S, 2)]
    xs = np.stack([array_mixture(seed + b, line[:M], azimuths, n, 16000) for b in range(B)])
    dirs = azimuthDirections(D)
    e = GCCNMFArrayEngine(n, numChannels=M, microphonePositions=line[:M], directions=dirs, speedOfSound=SOUND, windowSize=n_fft,
                          hopSize=hop, numTargets=S, dictionarySize=Kk, numIterations=iters, batch=B)
    P, F, T = e.P, e.F, e.T
    Fp = -(-F // 16) * 16
    assert (F, T, e.Fs, e.N) == (n_fft // 2 + 1, 1 + (n - n_fft) // hop, (P - 1) * Fp + F, M * T) and e.nsig_pitch == S * M + (S * M) % 2
    tau = A.pair_tdoas_from_geometry(line[:M], A.azimuth_directions(D), SOUND)
    assert np.array_equal(e.pairTDOAs, tau)
    y = e.separate(xs)
    what = 'M=%d batch=%d S=%d' % (M, B, S)
    w = np.hanning(n_fft).astype(np.float32)
    freqs = np.linspace(0, 8000.0, F)

    # X of every signal: the stereo STFT of consecutive signal pairs (the last one beside a silent spare when batch * M is odd)
    X = e.get_X()
    flat = np.concatenate([xs.reshape(B * M, n), np.zeros((1, n), np.float32)])
    Xf = X.reshape(B * M, F, T)
    for j in range(0, B * M, 2):
        ref, sumabs = K.stft64(flat[j:j + 2], w, n_fft, hop, T)
        bar = K.stft_bar(sumabs, n_fft)
        for c in range(min(2, B * M - j)):
            K.check_bar(Xf[j + c], ref[c], bar, '%s X of signal %d' % (what, j + c))
    assert not e._X[B * M:].cpu().numpy().any() or (B * M) % 2 == 0

    V, Cd = e.get_V(), e.get_C()
    Wd, Hd = e.get_WH()
    ang, mean = e.get_angular()
    idx, sc, am, spec = e.get_tdoa_indexes(), e.get_scores(), e.get_argmax(), e.get_spec()
    status = e.status.cpu().numpy()
    for b in range(B):
        ref_V, ref_C = A.features(X[b])
        assert np.abs(V[b] - ref_V).max() <= K.HYPOT_U * U * np.abs(ref_V).max(), what
        assert np.abs(Cd[b] - ref_C).max() <= (4 + 2 * K.HYPOT_U) * U * (1 + 1e-5) * np.sqrt(2), what
        ref_ang, absprod = A.angular(Cd[b], freqs, tau)
        C.report_gemm_like(ang[b], ref_ang, absprod, 2 * P * F, what='%s angular spectrogram of file %d' % (what, b))
        C.check_mean(mean[b], ang[b], '%s mean of file %d' % (what, b))
        C.check_peaks(idx[b], status[b], mean[b], S, '%s peaks of file %d' % (what, b))
        assert status[b] == 0, 'the mixtures are chosen so that every file has its peaks'
        ref_G, absG = A.scores(Cd[b], Wd[b], freqs, tau, idx[b])
        C.report_gemm_like(sc[b], ref_G, absG, P * F, what='%s scores of file %d' % (what, b))
        C.check_argmax(am[b], sc[b], '%s arg-max of file %d' % (what, b))
        ref_spec = A.ratio_one_hot(Wd[b], Hd[b], am[b], S, X[b])
        assert (A.denominators(Wd[b], Hd[b], M, argmax=am[b], S=S) > 0).all()
        C.report_gemm_like(spec[b], ref_spec, np.broadcast_to(np.abs(X[b])[None], ref_spec.shape), Kk, what='%s spec of file %d' % (what, b))
        slots = torch.view_as_complex(e.spec)[b, :, :F, :T].cpu().numpy()
        ref_y, bar = A.istft(slots, w, n_fft, hop, hop / float(n_fft) * 2)
        got_y = e._y[b].cpu().numpy()
        err = np.abs(got_y - ref_y)
        print('%s waveforms of file %d: worst share of the bar %.4f' % (what, b, (err / np.maximum(bar, 1e-300)).max()))
        assert (err <= bar).all(), '%s waveforms of file %d: worst share of the bar %.3g' % (what, b, (err / np.maximum(bar, 1e-300)).max())
        assert np.array_equal(got_y[:S * M].reshape(S, M, -1), y[b])
        if e.nsig_pitch > S * M:
            # (its waveform shares one complex transform with the last real slot: within the bar above, not exactly zero)
            assert not slots[S * M:].any(), 'the spare spectrogram slot stays zero'
    assert np.isfinite(y).all() and np.abs(y).max() > 0

    # W, H: a direct library call on the engine's V
    W2 = e.W0.unsqueeze(0).expand_as(e.W).contiguous()
    H2 = e.H0.unsqueeze(0).expand_as(e.H).contiguous()
    ws = torch.zeros_like(e.ws_nmf)
    _hip.klnmf(e.V, W2, H2, ws, F, e.N, Kk, B, iters, 0.0, 1e-16)
    torch.cuda.synchronize()
    assert same_bits(W2, e.W) and same_bits(H2, e.H), what
    return e


@pytest.mark.parametrize('M,B,S', [(4, 2, 3), (3, 1, 3), (3, 3, 2)], ids=['M4-b2-S3', 'M3-b1-S3', 'M3-b3-S2'])
def test_stage_by_stage_against_float64(M, B, S):
    run_stages(M, B, S, 10 * M + B)


@pytest.mark.parametrize('M,B,S', list(SP.ENGINE_CASES), ids=['M%d-b%d-S%d' % c for c in SP.ENGINE_CASES])
def test_five_to_eight_microphones_stage_by_stage_against_float64(M, B, S):
    """B M odd at (5, 1, 2): the STFT's spare signal slot; B M and S M odd at (7, 1, 3): the spare spectrogram slot stays zero; at M = 8
    the stacked calls run at Fs = 4017 bins."""
    e = run_stages(M, B, S, SP.ENGINE_CASES[(M, B, S)], line=SP.LINE8, **SP.ENGINE_SHAPE)
    assert e.P == M * (M - 1) // 2 and (M < 8 or e.Fs == 4017)
    assert e.get_tdoa_indexes().tolist() == [[13, 30, 43][:S]] * B, 'the talkers at 40, 90 and 130 degrees of a 61-point scan'


def test_the_corner_of_the_envelope_stage_by_stage_against_float64():
    """Eight microphones at the longest window: Fs = 57777 stacked bins (grid extent 57792 of 65535), three frames, K = 16, two iterations."""
    M, B, S = SP.CORNER_CASE
    e = run_stages(M, B, S, SP.CORNER_SEED, line=SP.LINE8, Kk=16, iters=2, **SP.CORNER_SHAPE)
    assert (e.F, e.T, e.Fs, e.P * e.Fp) == (2049, 3, 57777, 57792)
    assert e.get_tdoa_indexes().tolist() == [[13, 30]]


def test_the_line_array_finds_its_three_talkers():
    """The mixture of tests/test_array_host.py (4-microphone line, talkers at 40 / 90 / 130 degrees, 181 azimuths, 1 s at 16 kHz, n_fft
    1024): the device picks the indexes the float64 restatement picks there."""
    from gcc_nmf_amd.array import GCCNMFArrayEngine, azimuthDirections
    from gcc_nmf_amd.synthetic import array_mixture
    x = array_mixture(0, LINE, [40, 90, 130], 16000, 16000)
    e = GCCNMFArrayEngine(16000, numChannels=4, microphonePositions=LINE, directions=azimuthDirections(181), speedOfSound=SOUND,
                          numTargets=3, dictionarySize=16, numIterations=2)
    y = e.separate(x)
    assert e.get_tdoa_indexes().tolist() == [[40, 90, 130]]
    assert y.shape == (1, 3, 4, 256 * 58) and np.isfinite(y).all()
    assert e.Fs == 5 * 528 + 513 and e.Fs > 2049, 'the stacked calls run beyond the stereo envelope of 2049 bins'
