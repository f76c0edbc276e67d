"""-m gpu: the device-resident pipeline (GCCNMFEngine) against the committed reference goldens, the
live oracle, and size-independent properties at the benchmark shape."""
import numpy as np
import pytest

import gcc_checks
from conftest import golden, golden_wav, mask_flips
from oracle import gccnmf_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

# coefficient masks are exact except at genuine near-ties of the reference's own scores.  The goldens list every
# (k, t) whose top-2 relative gap is below 1e-2 (conftest.mask_flips); a flip anywhere else fails.  The device's W/H differ from
# the reference's by ~5e-6 relative after 100 iterations (summation order), so scores move by about that much: measured on
# MI355X the largest gap that ever flipped is 5.6e-5 (dev1 in the six-file batch, K=1024; 0-6 flips per 637k coefficients), printed by the tests below (-s).
# SURVEY 8(c) names 1e-5 (from 0 flips between an f32 and an f64 oracle run on dev1); that is below the reference's OWN noise floor:
# the same NumPy/OpenBLAS float32 expressions with 1 vs 8 BLAS threads (sgemm summation order only; oracle/mask_noise_floor.py,
# tests/golden/mask_noise_floor.json) differ by 1.6-2.1e-6 in W and flip 0-2 coefficients per mixture at K = 1024, the largest at a gap
# of 3.9e-5 (dev_B).  The device's drift is 2-3x that thread-order noise (different k-tiling), hence 1e-4 = 2.6x the reference's own
# largest self-flip; the kernels that divide V / (W.H) by rcp + Newton instead of IEEE change nothing here (scripts/mask_flips.py).
TIE_LIMIT = 1e-4


def live_gaps(G):
    """relative top-2 gap of oracle scores G (S, K, T) -> (K, T); inf with one target (nothing to flip to)"""
    srt = np.sort(np.asarray(G, np.float64), axis=0)
    if len(srt) < 2:
        return np.full(srt.shape[1:], np.inf)
    return (srt[-1] - srt[-2]) / np.maximum(np.abs(srt[-1]), 1e-300)


WAVS = ['dev_A_1_2_3_4', 'dev_B_1_8_9_16', 'dev_C_2_7_10_15', 'dev_D_13_14_15_16', 'dev_Sq1_Co_A']


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300)


def engine(n, **kw):
    from gcc_nmf_amd.engine import GCCNMFEngine
    return GCCNMFEngine(n, **kw)


def check_after_masks(spec, y, argmax, X, W, H, ref, windowSize, hopSize, spec_tol=1e-4, y_tol=1e-6):
    """The stages after the coefficient masks of one file, compared twice, both always:
    (a) under the device's own decisions and intermediates: the oracle's getTargetSpectrogramEstimates of the device's arg-max (one-hot),
        X, W and H against the device's spectrogram, and the oracle's inverse STFT of the device's spectrogram against its waveforms;
    (b) against the oracle's own run ``ref`` on every frame where no atom's target flipped -- and most frames must be compared.
    spec (S, 2, F, T), y (S, 2, L), argmax (K, T), X (2, F, T), W (F, K), H (K, 2T)."""
    S = spec.shape[0]
    onehot = np.stack([(argmax == i) for i in range(S)]).astype(np.float32)
    est = O.getTargetSpectrogramEstimates(onehot, X, W, np.array(np.hsplit(H, 2)))
    assert np.abs(spec - est).max() < spec_tol * np.abs(est).max()
    yc = O.getTargetSignalEstimates(spec, windowSize, hopSize, np.hanning)
    rms = np.sqrt(np.mean((y.astype(np.float64) - yc) ** 2))
    assert rms < y_tol, rms
    ok = ~(argmax != np.argmax(ref['M'], 0)).any(axis=0)
    assert 2 * ok.sum() > ok.size, (int(ok.sum()), ok.size)
    assert np.abs(spec[..., ok] - ref['S'][..., ok]).max() < spec_tol * np.abs(ref['S']).max()


@pytest.mark.parametrize('K', [128, 1024])
def test_dev1_against_reference_golden(dev1, K):
    """BASELINE configs 1/2: dev1 mixture, hop 256, K=128 / K=1024, 100 iterations: TDOA indexes
    bit-exact, waveform RMS <= 1e-4 against the unmodified reference's output."""
    x, sr = dev1
    g = golden('dev1_hop256_K%d' % K)
    e = engine(x.shape[1], sampleRate=sr, dictionarySize=K, numIterations=100)
    y = e.separate(x)[0]
    assert e.get_tdoa_indexes()[0].tolist() == [47, 72, 107] == list(g['idx'])
    sub = int(g['sub'])
    X = e.get_X()[0]
    assert np.abs(X[:, ::4, ::7] - g['X_sub']).max() < 1e-5 * np.abs(g['X_sub']).max()
    W, H = e.get_WH()
    assert rel(W[0][:, ::sub], g['W_sub']) < 1e-4 and rel(H[0][::sub, :], g['H_sub']) < 1e-4
    ang, meanA = e.get_angular()
    assert np.abs(meanA[0] - g['meanA']).max() < 1e-3
    flips, worst = mask_flips(e.get_argmax()[0], g)
    assert worst < TIE_LIMIT, (flips, worst)
    assert y.shape == (3, 2, 158976) and y.dtype == np.float32
    rms = np.sqrt(np.mean((y.astype(np.float64) - g['y']) ** 2))
    assert rms < 1e-6, rms                                  # bar: 1e-4; measured 7e-9 (K=128) / 1.2e-8 (K=1024)
    print('dev1 K=%d: W rel %.2e H rel %.2e mask flips %d (largest reference gap among them %.1e) waveform rms %.2e' %
          (K, rel(W[0][:, ::sub], g['W_sub']), rel(H[0][::sub, :], g['H_sub']), flips, worst, rms))


@pytest.mark.parametrize('K,launches', [(128, 'auto'), (128, 'fused'), (128, 'four'), (1024, 'auto')])
def test_all_reference_mixtures_batched(K, launches):
    """The five other reference mixtures as ONE batch of 5 (+ dev1), K = 128 and K = 1024: TDOA indexes exact for every file.
    Their sources sit within 4 TDOA bins of each other (d = 1 m assumed, real spacing 5 cm), which makes
    this the sharp test of the f32 angular spectrum.  K = 128 also with both short-dictionary fused launches forced (tuning keys 16 / 17 = 2:
    K1 + K2 on column tiles, K3 + K4a on bin slabs, csrc/direct.hip) and with neither: the same bars against the reference's outputs."""
    from gcc_nmf_amd import _hip
    lib = _hip.lib()
    names = ['dev1_female3_liverec_130ms_1m'] + WAVS
    xs = np.stack([golden_wav(w)[0] for w in names])
    e = engine(xs.shape[2], dictionarySize=K, numIterations=100, batch=len(names))
    try:
        if launches != 'auto':
            v = 2 if launches == 'fused' else 0
            assert lib.gccnmf_set_tuning(16, v) == 0 and lib.gccnmf_set_tuning(17, v) == 0
            assert lib.gccnmf_klnmf_plan(e.g.F, e.g.N, K, len(names), 0) == (6 if launches == 'fused' else 0)
        y = e.separate(xs)
    finally:
        lib.gccnmf_set_tuning(16, 1)
        lib.gccnmf_set_tuning(17, 1)
    idx = e.get_tdoa_indexes()
    for i, w in enumerate(names):
        g = golden('%s_hop256_K%d' % (w, K)) if i else golden('dev1_hop256_K%d' % K)
        assert idx[i].tolist() == list(g['idx']), w
        assert np.abs(e.get_angular()[1][i] - g['meanA']).max() < 1e-3
        flips, worst = mask_flips(e.get_argmax()[i], g)
        assert worst < TIE_LIMIT, (w, flips, worst)
        ref = g['y'][:, :, ::8] if 'y' in g.files else g['y_sub']
        rms = np.sqrt(np.mean((y[i][:, :, ::8].astype(np.float64) - ref) ** 2))
        assert rms < 1e-5, (w, rms)      # bar 1e-4; measured <= 2.0e-6 (a near-tie flip moves one atom of one frame)
        wh = ''
        if K == 1024:                    # the factors of EVERY reference mixture against the reference's own (oracle/make_golden_wh.py)
            gw = golden('wh_sub_K1024')
            W, H = e.get_WH()
            rw, rh = rel(W[i][:, ::16], gw[w + '_W']), rel(H[i][::16, ::2], gw[w + '_H'])
            assert rw < 1e-4 and rh < 1e-4, (w, rw, rh)      # SURVEY 8(c) bar; the reference against itself (1 vs 8 BLAS threads): 2e-6
            wh = ' W rel %.2e H rel %.2e' % (rw, rh)
        print('%s K=%d: mask flips %d (largest reference gap %.1e) waveform rms %.2e%s' % (w, K, flips, worst, rms, wh))


@pytest.mark.parametrize('K', [128, 1024])
def test_each_reference_mixture_alone_on_the_direct_path(K):
    """Every reference mixture processed ALONE -- the call the reference driver and the notebooks make, which round 4 moved to the
    direct-to-register kernels (csrc/direct.hip) -- against the reference's own outputs: TDOA indexes exact, masks exact outside the
    reference's near-ties, waveforms, and at K = 1024 the factors themselves."""
    names = ['dev1_female3_liverec_130ms_1m'] + WAVS
    for i, w in enumerate(names):
        x = golden_wav(w)[0]
        e = engine(x.shape[1], dictionarySize=K, numIterations=100, batch=1)
        y = e.separate(x)
        g = golden('%s_hop256_K%d' % (w, K)) if i else golden('dev1_hop256_K%d' % K)
        assert e.get_tdoa_indexes()[0].tolist() == list(g['idx']), w
        flips, worst = mask_flips(e.get_argmax()[0], g)
        assert worst < TIE_LIMIT, (w, flips, worst)
        ref = g['y'][:, :, ::8] if 'y' in g.files else g['y_sub']
        rms = np.sqrt(np.mean((y[0][:, :, ::8].astype(np.float64) - ref) ** 2))
        assert rms < 1e-5, (w, rms)
        wh = ''
        if K == 1024:
            gw = golden('wh_sub_K1024')
            W, H = e.get_WH()
            rw, rh = rel(W[0][:, ::16], gw[w + '_W']), rel(H[0][::16, ::2], gw[w + '_H'])
            assert rw < 1e-4 and rh < 1e-4, (w, rw, rh)
            wh = ' W rel %.2e H rel %.2e' % (rw, rh)
        print('%s alone, K=%d: mask flips %d (largest reference gap %.1e) waveform rms %.2e%s' % (w, K, flips, worst, rms, wh))


@pytest.mark.parametrize('K', [128, 1024])
def test_hop128_reference_default(dev1, K):
    x, sr = dev1
    g = golden('dev1_female3_liverec_130ms_1m_hop128_K%d' % K)
    e = engine(x.shape[1], sampleRate=sr, hopSize=128, dictionarySize=K, numIterations=100)
    y = e.separate(x)[0]
    assert e.get_tdoa_indexes()[0].tolist() == list(g['idx'])
    assert y.shape == (3, 2, 128 * 1242)
    flips, worst = mask_flips(e.get_argmax()[0], g)
    assert worst < TIE_LIMIT, (flips, worst)
    assert np.sqrt(np.mean((y[:, :, ::8].astype(np.float64) - g['y_sub']) ** 2)) < 1e-6


@pytest.fixture(params=[1, 2], ids=['tile-throughput', 'tile-small'])
def forced_tile(request):
    from gcc_nmf_amd import _hip
    lib = _hip.lib()
    assert lib.gccnmf_set_tuning(2, request.param) == 0
    yield request.param
    lib.gccnmf_set_tuning(2, 0)


def test_dev1_K1024_both_tiles(dev1, forced_tile):
    """Config 2 (single dev1 mixture, K = 1024) through each GEMM tile shape explicitly."""
    x, sr = dev1
    g = golden('dev1_hop256_K1024')
    e = engine(x.shape[1], sampleRate=sr, dictionarySize=1024, numIterations=100)
    y = e.separate(x)[0]
    assert e.get_tdoa_indexes()[0].tolist() == [47, 72, 107]
    flips, worst = mask_flips(e.get_argmax()[0], g)
    assert worst < TIE_LIMIT, (flips, worst)
    assert np.sqrt(np.mean((y.astype(np.float64) - g['y']) ** 2)) < 1e-6


def test_synthetic_against_oracle_stagewise():
    """Seeded synthetic input, every intermediate against the live oracle (ragged T: 9000 samples -> 32 frames)."""
    for n, K, it in [(9000, 24, 7), (30000, 200, 10)]:
        x = O.synthetic_mixture(3, numSamples=n)
        r = O.runGCCNMF(x, 16000, 1024, 256, 128, 1.0, 3, dictionarySize=K, numIterations=it, return_intermediates=True)
        e = engine(n, dictionarySize=K, numIterations=it)
        y = e.separate(x)[0]
        assert np.abs(e.get_X()[0] - r['X']).max() < 1e-5 * np.abs(r['X']).max()
        assert np.abs(e.get_V()[0] - r['V']).max() < 1e-5 * r['V'].max()
        # the coherence is a unit-modulus RATIO: where |X| sits at the f32 FFT noise floor (~1e-6 max|X|) its phase is
        # noise in both implementations, so check the kernel's arithmetic on the device's own X, and the oracle's C
        # only where both channels are well above that floor
        Xd = e.get_X()[0]
        C_from_Xd = Xd[0] * Xd[1].conj() / np.abs(Xd[0]) / np.abs(Xd[1])
        assert np.abs(e.get_C()[0] - C_from_Xd).max() < 1e-5
        strong = np.minimum(np.abs(r['X'][0]), np.abs(r['X'][1])) > 1e-2 * np.abs(r['X']).max()
        assert np.abs(e.get_C()[0] - r['C'])[strong].max() < 2e-3
        W, H = e.get_WH()
        assert rel(W[0], r['W']) < 1e-4 and rel(H[0], r['H']) < 1e-4
        ang, meanA = e.get_angular()
        # +-513 range; the difference is dominated by the noise-floor bins' phase (see above), not by the f32 GEMM
        assert np.abs(ang[0] - r['A']).max() < 5e-2 and np.abs(meanA[0] - r['meanA']).max() < 5e-3
        ang_same_C = np.dot(np.exp(np.outer(e.frequenciesInHz, -(2j * np.pi) * e.tdoasInSeconds)).T, e.get_C()[0].astype(np.complex128)).real
        assert np.abs(ang[0] - ang_same_C).max() < 1e-3              # the GEMM itself, on the device's own coherence
        assert e.get_tdoa_indexes()[0].tolist() == r['idx']
        assert np.abs(e.get_scores()[0] - r['G']).max() < 1e-4 * np.abs(r['G']).max()
        flipped = e.get_argmax()[0] != np.argmax(r['M'], 0)
        assert (live_gaps(r['G'])[flipped] < TIE_LIMIT).all(), (int(flipped.sum()), live_gaps(r['G'])[flipped].max())
        check_after_masks(e.get_spec()[0], y, e.get_argmax()[0], e.get_X()[0], W[0], H[0], r, 1024, 256)
        assert np.sqrt(np.mean((y.astype(np.float64) - r['y']) ** 2)) < 1e-6


# windowSize (F = 129 ... 2049), numTDOAs, numTargets and K off the n_fft = 1024 / 128 TDOAs / 3 targets path: every value twice
OFF_PATH = [  # (windowSize, hopSize, numTDOAs, numTargets, K)
    (256, 128, 33, 1, 64), (256, 128, 200, 4, 200), (512, 256, 200, 1, 200), (512, 256, 33, 4, 64),
    (2048, 512, 33, 4, 200), (2048, 512, 200, 1, 64), (4096, 1024, 200, 4, 64), (4096, 1024, 33, 1, 200),
]


@pytest.mark.parametrize('ws,hop,D,S,K', OFF_PATH, ids=['ws%d-hop%d-D%d-S%d-K%d' % c for c in OFF_PATH])
def test_engine_against_oracle_off_the_1024_path(ws, hop, D, S, K):
    """GCCNMFEngine against O.runGCCNMF (1.5 s, four sources, 10 iterations): TDOA indexes exact, W / H <= 1e-4, masks exact up to the
    oracle's near-ties, the localisation GEMM on the device's own coherence, the stages after the masks both ways (check_after_masks)."""
    n = 24000
    x = O.synthetic_mixture(17, numSamples=n, delays=(-30, -12, 5, 24))
    r = O.runGCCNMF(x, 16000, ws, hop, D, 1.0, S, dictionarySize=K, numIterations=10, return_intermediates=True)
    e = engine(n, windowSize=ws, hopSize=hop, numTDOAs=D, numTargets=S, dictionarySize=K, numIterations=10)
    y = e.separate(x)[0]
    assert e.get_tdoa_indexes()[0].tolist() == r['idx']
    W, H = e.get_WH()
    assert rel(W[0], r['W']) < 1e-4 and rel(H[0], r['H']) < 1e-4, (rel(W[0], r['W']), rel(H[0], r['H']))
    ang, meanA = e.get_angular()
    C = e.get_C()[0].astype(np.complex128)
    E = np.exp(np.outer(e.frequenciesInHz, -(2j * np.pi) * e.tdoasInSeconds))
    absA = np.dot(np.abs(E.real).T, np.abs(C.real)) + np.dot(np.abs(E.imag).T, np.abs(C.imag))
    gcc_checks.check_gemm_like(ang[0], np.dot(E.T, C).real, absA, 2 * (ws // 2 + 1), what='angular spectrogram')
    gcc_checks.check_mean(meanA[0], ang[0])
    G = e.get_scores()[0]
    assert G.shape == r['G'].shape == (S, K, r['X'].shape[2])
    am = e.get_argmax()[0]
    flipped = am != np.argmax(r['M'], 0)
    assert (live_gaps(r['G'])[flipped] < TIE_LIMIT).all(), (int(flipped.sum()), live_gaps(r['G'])[flipped].max())
    check_after_masks(e.get_spec()[0], y, am, e.get_X()[0], W[0], H[0], r, ws, hop)
    assert y.shape == r['y'].shape
    rms = np.sqrt(np.mean((y.astype(np.float64) - r['y']) ** 2))
    assert rms < 1e-5, rms


def test_benchmark_batch_against_oracle():
    """The bench workload itself (64 synthetic 10 s files, K = 1024, 100 iterations, throughput tile, two file groups): TDOA
    indexes of ALL 64 files against the oracle's localisation, and four files (first, last, two from the middle) through the
    oracle's whole pipeline: masks exact up to near-ties, waveforms <= 1e-6 RMS (bar 1e-4)."""
    from gcc_nmf_amd.synthetic import synthetic_batch
    xs = synthetic_batch(0, 64)
    e = engine(160000, dictionarySize=1024, numIterations=100, batch=64)
    y = e.separate(xs)
    idx = e.get_tdoa_indexes()
    freqs = np.linspace(0, 8000.0, 513)
    for b in range(64):
        X = O.computeComplexMixtureSpectrogram(xs[b], 1024, 256, np.hanning)
        meanA = np.mean(O.getAngularSpectrogram(O.spectralCoherence(X), freqs, 1.0, 128), axis=-1)
        assert idx[b].tolist() == [int(i) for i in O.estimateTargetTDOAIndexesFromAngularSpectrum(meanA, 1.0, 128, 3)], b
    am = e.get_argmax()
    for b in (0, 21, 42, 63):
        r = O.runGCCNMF(xs[b], 16000, 1024, 256, 128, 1.0, 3, dictionarySize=1024, numIterations=100, return_intermediates=True)
        flipped = am[b] != np.argmax(r['M'], 0)
        gaps = live_gaps(r['G'])[flipped]
        assert (gaps < TIE_LIMIT).all(), (b, int(flipped.sum()), gaps.max())
        rms = np.sqrt(np.mean((y[b].astype(np.float64) - r['y']) ** 2))
        assert rms < 1e-5, (b, rms)      # bar 1e-4; measured <= 1.7e-6
        print('bench file %d: mask flips %d (largest oracle gap %.1e) waveform rms %.2e' % (b, int(flipped.sum()), gaps.max() if len(gaps) else 0, rms))


def test_too_few_peaks_is_an_error():
    n = 9000
    x = np.zeros((2, n), np.float32)
    x[:] = np.random.RandomState(0).standard_normal(n).astype(np.float32) * 0.01   # identical channels: one peak only
    # 8 TDOAs have 6 interior bins and strict maxima cannot be adjacent: at most 3 peaks, 4 requested
    e = engine(n, dictionarySize=16, numIterations=2, numTDOAs=8, numTargets=4)
    with pytest.raises(ValueError):
        e.separate(x)
    with pytest.raises(ValueError):
        e.upload(np.full((2, n), np.nan, np.float32))
    with pytest.raises(ValueError):
        e.upload(np.zeros((2, n + 1), np.float32))


def test_zero_magnitude_bins_do_not_poison_the_batch():
    """|X| == 0 bins (a silent channel here; an exactly-cancelling Nyquist bin in practice) give the reference a 0/0 = NaN
    coherence.  The device path defines their coherence as 0: the silent file fails cleanly with 'too few peaks', its
    neighbour in the batch is untouched and nothing is NaN."""
    n = 20000
    good = O.synthetic_mixture(4, numSamples=n)
    bad = good.copy()
    bad[1] = 0
    e = engine(n, dictionarySize=32, numIterations=5, batch=2)
    with pytest.raises(ValueError, match=r'file\(s\) \[1\]'):
        e.separate(np.stack([good, bad]))
    assert np.isfinite(e.get_angular()[0]).all() and np.isfinite(e.get_C()).all()
    y0 = e.y[0].cpu().numpy()
    e2 = engine(n, dictionarySize=32, numIterations=5, batch=2)                # the clean file next to another clean file
    assert np.array_equal(e2.separate(np.stack([good, good]))[1], y0)


def test_benchmark_shape_properties():
    """BASELINE config 2/3 shape (F=513, T=622, K=1024) on a batch of 8: properties that need no oracle.
      - masks partition the coefficients: sum_i S[i,c] == (W.H_c) * X_c/|X_c|
      - KL divergence D(V || W.H) after 30 iterations is below the value after 5 (multiplicative updates descend)
      - unit-L2 atoms, non-negative factors, untouched zero padding
      - every file of the batch equals its own run in another batch: bit for bit when both runs use the same GEMM tile (the
        result does not depend on the batch position or size), and to 1e-6 of the signal RMS for the file ALONE (the direct
        latency path, and the small-batch tile sums each 16-deep k-tile in a different order than the LDS-DMA tile)."""
    from gcc_nmf_amd.synthetic import synthetic_batch
    xs = synthetic_batch(100, 8)
    e = engine(160000, dictionarySize=1024, numIterations=30, batch=8)
    y = e.separate(xs)
    g = e.g
    assert e.get_tdoa_indexes().tolist() == [[27, 59, 91]] * 8
    W = e.W[:, :g.F, :g.K]
    H = e.H[:, :g.K, :g.N]
    V = e.V[:, :g.F, :g.N]
    assert torch.all(W >= 0) and torch.all(H >= 0)
    assert torch.allclose(torch.linalg.norm(W, dim=1), torch.ones_like(W[:, 0]), atol=1e-5)
    assert not e.W[:, g.F:].any() and not e.H[:, :, g.N:].any() and not e.H[:, g.K:].any()
    WH = torch.bmm(W.double(), H.double())

    def kl(WH_):
        return (V.double() * torch.log(V.double() / WH_) - V.double() + WH_).sum(dim=(1, 2))
    kl30 = kl(WH)
    spec = torch.view_as_complex(e.spec)[:, :, :g.F, :g.T].reshape(8, 3, 2, g.F, g.T)
    X = torch.view_as_complex(e.X)[:, :, :g.F, :g.T]
    total = spec.sum(dim=1)                                       # (8, 2, F, T)
    expect = torch.stack([WH[:, :, :g.T], WH[:, :, g.T:]], dim=1) * (X / X.abs()).to(torch.complex128)
    err = (total.to(torch.complex128) - expect).abs().max().item()
    assert err < 1e-4 * expect.abs().max().item(), err
    assert np.isfinite(y).all() and y.shape == (8, 3, 2, 158976)

    e5 = engine(160000, dictionarySize=1024, numIterations=5, batch=8)
    e5.upload(xs)
    e5.run()
    W5, H5 = e5.W[:, :g.F, :g.K].double(), e5.H[:, :g.K, :g.N].double()
    kl5 = kl(torch.bmm(W5, H5))
    assert torch.all(kl30 < kl5), (kl30, kl5)

    e1 = engine(160000, dictionarySize=1024, numIterations=30, batch=1)
    y1 = e1.separate(xs[5])
    assert e1.get_tdoa_indexes().tolist() == [[27, 59, 91]]
    assert np.sqrt(np.mean((y1[0] - y[5]) ** 2)) < 1e-6 * np.sqrt(np.mean(y[5] ** 2))
    from gcc_nmf_amd import _hip
    lib = _hip.lib()
    e2 = engine(160000, dictionarySize=1024, numIterations=30, batch=2)
    for policy in (1, 2):                 # same GEMM tile for both batch sizes -> bit-identical
        assert lib.gccnmf_set_tuning(2, policy) == 0
        try:
            y8 = e.separate(xs)
            y2 = e2.separate(xs[4:6])
            y1 = e1.separate(xs[5])
        finally:
            lib.gccnmf_set_tuning(2, 0)
        assert np.array_equal(y2[1], y8[5]), policy
        if policy == 1:                   # forcing the throughput tile also switches the single-file latency path off
            assert np.array_equal(y1[0], y8[5])


def test_pcm16_ingest_and_egress(dev1, tmp_path):
    """int16 frames in, int16 frames out, conversions fused on the device -- against wavread / wavwrite
    semantics (gccNMF/wavfile.py) applied to the float path, and against the reference's own waveform golden."""
    from scipy.io import wavfile
    from conftest import GOLDEN
    import os
    sr, pcm = wavfile.read(os.path.join(GOLDEN, 'data', 'dev1_female3_liverec_130ms_1m_mix.wav'))
    assert pcm.dtype == np.int16 and pcm.shape == (160000, 2)
    e = engine(160000, dictionarySize=128, numIterations=100)
    out = e.separate_pcm16(pcm)[0]                                   # (3, L, 2) int16
    assert out.dtype == np.int16 and out.shape == (3, 158976, 2)
    y_float = e.y[0].cpu().numpy()                                    # the float waveforms of the same run
    assert np.array_equal(out.transpose(0, 2, 1), O.float2pcm(y_float))          # egress == float2pcm, exactly (no clipping here)
    x, _ = dev1
    e2 = engine(160000, dictionarySize=128, numIterations=100)
    assert np.array_equal(e2.separate(x)[0], y_float)                # ingest == pcm2float + float path, bit for bit
    g = golden('dev1_hop256_K128')
    assert np.abs(out.transpose(0, 2, 1).astype(int) - O.float2pcm(g['y']).astype(int)).max() <= 1   # vs the reference's output
    # clip protection: a block whose peak exceeds 1 is rescaled to 0.99 like wavwrite
    e.y.mul_(40.0)
    e.pack_pcm16()
    loud = e.pcm_out[0].cpu().numpy().transpose(0, 2, 1)
    yl = e.y[0].cpu().numpy()
    for i in range(3):
        m = np.max(np.abs(yl[i]))
        expect = O.float2pcm((yl[i] / m * 0.99).astype(np.float32)) if m >= 1 else O.float2pcm(yl[i])
        # exactly: fft.hip is built without fma contraction and the reference computes in float32 (tests/test_gpu_fft_stages.py shows it group by group)
        assert np.array_equal(loud[i], expect)


def test_nmf_file_groups_on_streams_are_bitwise_the_single_stream_result():
    """The engine runs KL-NMF per file group on separate streams (tail of one group's launches overlaps the head of
    another's); the mixtures are independent, so the result is bit for bit that of one launch over the whole batch, and a
    second run of the same engine (stream / event reuse) reproduces it."""
    from gcc_nmf_amd.synthetic import synthetic_batch
    xs = synthetic_batch(300, 32, numSamples=32000)
    kw = dict(dictionarySize=128, numIterations=10, batch=32)
    e1 = engine(32000, nmf_groups=1, **kw)
    y1 = e1.separate(xs)
    assert engine(32000, **kw).nmf_groups == 1          # K = 128: a half batch would no longer fuse / fill the chip like the whole
    # K = 1024: the library runs the call as ONE chained launch (round 6) -- one group; without chaining the engine splits the batch in two
    from gcc_nmf_amd import _hip
    assert engine(160000, dictionarySize=1024, numIterations=1, batch=32).nmf_groups == 1
    try:
        assert _hip.lib().gccnmf_set_tuning(21, 0) == 0
        assert engine(160000, dictionarySize=1024, numIterations=1, batch=32).nmf_groups == 2
    finally:
        _hip.lib().gccnmf_set_tuning(21, 1)
    for groups in (2, 4):
        eg = engine(32000, nmf_groups=groups, **kw)
        assert eg.nmf_groups == groups
        yg = eg.separate(xs)
        assert np.array_equal(yg, y1) and torch.equal(eg.W, e1.W) and torch.equal(eg.H, e1.H)
        assert np.array_equal(eg.separate(xs), y1)
    with pytest.raises(ValueError):
        engine(32000, nmf_groups=5, **kw)


@pytest.mark.parametrize('K', [512, 1024])
def test_narrow_items_in_the_one_shot_gemms_are_bitwise(K):
    """Tuning key 9 in the whole pipeline at a batch whose one-shot GEMMs end in a small partial round (9 files: reconstruction
    9 x 60 = 540 tiles -> 8 files + 1 file as half-height tiles; the score GEMM at K = 512: 270 tiles, all half-height; key 9 = 2: the
    score GEMM's tiles as narrow halves): scores, masks, spectrogram estimates and waveforms bit for bit those of the full-tiles-only form."""
    from gcc_nmf_amd import _hip
    from gcc_nmf_amd.synthetic import synthetic_batch
    lib = _hip.lib()
    xs = synthetic_batch(40, 9)
    outs = []
    try:
        for narrow in (0, 1, 2):
            assert lib.gccnmf_set_tuning(9, narrow) == 0
            e = engine(160000, dictionarySize=K, numIterations=3, batch=9)
            y = e.separate(xs)
            outs.append((y, e.get_scores(), e.get_argmax(), e.get_spec(), e.get_WH()))
    finally:
        lib.gccnmf_set_tuning(9, 1)
    for other in outs[1:]:
        for a, b in zip(outs[0][:4], other[:4]):
            assert np.array_equal(a, b)
        assert np.array_equal(outs[0][4][0], other[4][0]) and np.array_equal(outs[0][4][1], other[4][1])


def test_separate_batches_overlaps_transfers_and_matches_separate():
    """The pipelined host-to-host path (pinned staging, copy streams) returns, batch by batch and in order, exactly what
    ``separate`` returns; the engine is usable as before afterwards; bad input surfaces as the reference's error."""
    from gcc_nmf_amd.synthetic import synthetic_batch
    e = engine(32000, dictionarySize=64, numIterations=8, batch=4)
    batches = [synthetic_batch(400 + 4 * i, 4, numSamples=32000) for i in range(5)]
    expect = [e.separate(b) for b in batches]
    got = list(e.separate_batches(iter(batches)))
    assert len(got) == 5
    for a, b in zip(got, expect):
        assert np.array_equal(a, b)
    assert np.array_equal(e.separate(batches[2]), expect[2])
    assert list(e.separate_batches([])) == []
    bad = batches[1].copy()
    bad[0, 0, 5] = np.nan
    with pytest.raises(ValueError):
        list(e.separate_batches([batches[0], bad]))
    assert np.array_equal(e.separate(batches[0]), expect[0])


def test_klnmf_repeats_are_bitwise_identical():
    """Race detector for the hand-synchronised GEMM main loop (LDS-DMA, inline-asm fragment reads, LDS-counter split barrier):
    the same KL-NMF run repeated on the throughput tile gives bit-identical factors every time, as does the single-file
    latency path."""
    from gcc_nmf_amd.synthetic import synthetic_batch
    xs = synthetic_batch(500, 16)
    e = engine(160000, dictionarySize=1024, numIterations=8, batch=16)
    e.upload(xs)
    e.stft()
    e.klnmf()
    W0, H0 = e.W.clone(), e.H.clone()
    assert torch.isfinite(W0).all() and torch.isfinite(H0).all()
    for _ in range(12):
        e.klnmf()
        assert torch.equal(e.W, W0) and torch.equal(e.H, H0)
    e1 = engine(160000, dictionarySize=1024, numIterations=8, batch=1)
    e1.upload(xs[3])
    e1.stft()
    e1.klnmf()
    W1 = e1.W.clone()
    for _ in range(12):
        e1.klnmf()
        assert torch.equal(e1.W, W1)


def test_pcm16_egress_reports_non_finite_waveforms():
    """A NaN / Inf in a separated waveform must not become arbitrary PCM silently: the peak image flags it."""
    n = 20000
    x = O.synthetic_mixture(4, numSamples=n)
    e = engine(n, dictionarySize=16, numIterations=3)
    e.separate(x)
    e.pack_pcm16()
    e.check_pcm_finite()
    clean = e.pcm_out.cpu().numpy().copy()
    e.y[0, 1, 0, 77] = float('nan')
    e.y[0, 2, 1, 5] = float('inf')
    e.pack_pcm16()
    with pytest.raises(ValueError, match='non-finite'):
        e.check_pcm_finite()
    out = e.pcm_out.cpu().numpy()
    assert out[0, 1, 77, 0] == 0 and out[0, 2, 5, 1] == 32767                 # NaN -> 0, +Inf clips
    assert np.array_equal(out[0, 0], clean[0, 0])                             # the other groups are untouched
    mask = np.ones_like(out[0, 1], bool)
    mask[77, 0] = False
    assert np.array_equal(out[0, 1][mask], clean[0, 1][mask])                 # no rescale of a group with a NaN peak


def test_unmodified_reference_driver_on_hardware(tmp_path):
    """gccNMF/runGCCNMF.py, byte for byte unchanged, executed as __main__ on top of this package with the REAL HIP functions
    (dropin.run_reference_driver), when a reference checkout is staged on the box (GCCNMF_REFERENCE_ROOT, default
    oracle/_ref/reference_checkout: git-ignored scratch, see scripts/stage_reference.sh).  Its three output wav files against
    the reference's own output for its default parameters (hop 128, K = 128, 100 iterations): <= 1 LSB."""
    import os
    import sys
    import time
    from scipy.io import wavfile
    from conftest import REPO
    root = os.environ.get('GCCNMF_REFERENCE_ROOT', os.path.join(REPO, 'oracle', '_ref', 'reference_checkout'))
    if not os.path.exists(os.path.join(root, 'gccNMF', 'runGCCNMF.py')):
        pytest.skip('no reference checkout staged on this box')
    pytest.importorskip('matplotlib')
    from gcc_nmf_amd import dropin
    saved = {k: sys.modules.get(k) for k in list(dropin._ALIASES) + ['gccNMFPlotting', 'gccNMF', 'gccNMF.gccNMFPlotting']}
    try:
        t0 = time.perf_counter()
        out = dropin.run_reference_driver(root, str(tmp_path))
        dt = time.perf_counter() - t0
    finally:
        dropin.uninstall()
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    g = golden('dev1_female3_liverec_130ms_1m_hop128_K128')
    worst, beyond, total = 0, 0, 0
    for i in range(3):
        sr, pcm = wavfile.read(os.path.join(out, 'dev1_female3_liverec_130ms_1m_sim_%d.wav' % (i + 1)))
        assert sr == 16000 and pcm.shape == (158976, 2) and pcm.dtype == np.int16
        expect = (g['y_sub'][i] * 32768).clip(-32768, 32767).astype(np.int16)       # float2pcm of the reference's own output
        d = np.abs(pcm.T[:, ::8].astype(int) - expect)
        worst, beyond, total = max(worst, int(d.max())), beyond + int((d > 1).sum()), total + d.size
    print('unmodified runGCCNMF.py on the HIP functions: %.2f s wall (plots included); int16 outputs vs the reference: worst %d LSB, '
          '%d of %d samples beyond 1 LSB' % (dt, worst, beyond, total))
    # truncation to int16 turns any float difference into <= 1 LSB; a near-tie coefficient flip moves one atom of one frame
    # and can reach a few LSB on a handful of samples (measured on MI355X: worst 2 LSB)
    assert worst <= 4 and beyond <= 1e-4 * total


@pytest.mark.parametrize('n,hop,K,batch', [(160000, 256, 64, 3), (52000, 128, 32, 2), (33000, 256, 16, 1), (9000, 256, 16, 1)])
def test_fused_istft_overlap_add_is_bitwise_the_two_kernel_form(n, hop, K, batch):
    """The one-pass inverse STFT + overlap-add (no frame buffer) against frames kernel + overlap-add kernel: same bits (the FFT
    butterflies are explicitly rounded, the accumulation order is the reference's), including the first / last hops of the stream and
    frame counts that are not a multiple of the 32 hops a workgroup owns.  The engine picks the form by launch size."""
    from gcc_nmf_amd.synthetic import synthetic_batch
    xs = synthetic_batch(40, batch, numSamples=n)
    e = engine(n, hopSize=hop, dictionarySize=K, numIterations=3, batch=batch)
    e.fused_istft = True
    e.separate(xs)
    y_fused = e.y.clone()
    e.y.zero_()
    e.istft(keep_frames=True)
    assert torch.equal(e.y, y_fused)
    assert torch.isfinite(y_fused).all() and y_fused.abs().max() > 0


@pytest.mark.parametrize('K,iters,expect_ragged', [(1024, 6, True), (256, 5, True), (128, 8, False)])
def test_ragged_batch_is_bitwise_the_equal_length_batches(K, iters, expect_ragged):
    """Mixtures of different lengths in one batch (the reference separates a file of any length, runGCCNMF.py:30-36): 5 s, 10 s and 15 s
    files interleaved, KL-NMF over all of them in ONE chained launch whose lists hold each file's own column tiles
    (gccnmf_klnmf_ragged).  Every file gets bit for bit the factors, masks and waveforms it gets in a batch of files of its own length;
    K = 128 has no chained form -- the engine then runs one KL-NMF call per length, same bits."""
    from gcc_nmf_amd.engine import GCCNMFEngine, RaggedGCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_mixture
    lengths = [80000, 160000, 240000] * 8 + [160000]
    xs = [synthetic_mixture(900 + i, numSamples=n) for i, n in enumerate(lengths)]
    kw = dict(dictionarySize=K, numIterations=iters)
    e = GCCNMFEngine(lengths=lengths, **kw)
    assert isinstance(e, RaggedGCCNMFEngine) and e.batch == 25 and e.frames[:3] == [309, 622, 934]
    ys = e.separate(xs)
    assert e.ragged_klnmf_used is expect_ragged
    assert np.array_equal(e.separate(xs)[7], ys[7])                        # a second run of the same engine reproduces it
    from gcc_nmf_amd import _hip
    lib = _hip.lib()
    for n in sorted(set(lengths)):
        idx = [i for i, m in enumerate(lengths) if m == n]
        ref = engine(n, batch=len(idx), **kw)
        try:
            # an equal-length batch of 8 or 9 files would by itself take the small-batch kernels (other tiles, other summation order); on the
            # tiles a batch at scale takes -- the ones the ragged launch runs -- it is bit for bit the same (tuning key 2 = 1: any size on them)
            assert K <= 128 or lib.gccnmf_set_tuning(2, 1) == 0
            yr = ref.separate(np.stack([xs[i] for i in idx]))
        finally:
            lib.gccnmf_set_tuning(2, 0)
        sub = e.sub[n]
        assert torch.equal(sub.W, ref.W) and torch.equal(sub.H, ref.H), n
        assert torch.isfinite(sub.W).all() and torch.equal(sub.argmax, ref.argmax)
        for k, i in enumerate(idx):
            assert ys[i].shape == (3, 2, 256 * (sub.g.T - 1)) and np.array_equal(ys[i], yr[k]), (n, i)
    # and against the oracle, one file of the shortest length
    r = O.runGCCNMF(xs[0], 16000, 1024, 256, 128, 1.0, 3, dictionarySize=K, numIterations=iters, return_intermediates=True)
    sub, k = e.file(0)
    assert sub.get_tdoa_indexes()[k].tolist() == r['idx']
    assert rel(sub.get_WH()[0][k], r['W']) < 1e-4 and rel(sub.get_WH()[1][k], r['H']) < 1e-4
    assert np.sqrt(np.mean((ys[0].astype(np.float64) - r['y']) ** 2)) < 1e-5


def test_a_failed_chained_launch_is_loud_and_the_engine_falls_back():
    """Fault injection (lab build, tuning key 25): every consumer of a chained launch that has to wait gives up at once.  The library flags it, turns
    the factors into NaN (never plausible garbage) and reports it (gccnmf_klnmf_chain_status); GCCNMFEngine.separate() then switches the process to
    the plain launches, repeats the batch with a warning, and returns exactly the plain result; an explicit check raises."""
    from gcc_nmf_amd import _hip, HipLibraryError
    from gcc_nmf_amd.synthetic import synthetic_batch
    lib = _hip.lib()
    if lib.gccnmf_set_tuning(25, 1) != 0:
        pytest.skip('key 25 (fault injection into the chained hand-over) exists in experiment builds only: make EXPERIMENTS=1')
    xs = synthetic_batch(800, 24, numSamples=96000)
    try:
        assert lib.gccnmf_set_tuning(25, 0) == 0 and lib.gccnmf_set_tuning(21, 0) == 0
        e = engine(96000, dictionarySize=1024, numIterations=5, batch=24)
        y_plain = e.separate(xs)
        assert lib.gccnmf_set_tuning(21, 8) == 0 and lib.gccnmf_set_tuning(25, 1) == 0
        e = engine(96000, dictionarySize=1024, numIterations=5, batch=24)
        assert e.lib.gccnmf_klnmf_plan(e.g.F, e.g.N, 1024, 24, 0) & 8
        e.upload(xs)
        e.run()
        assert e.chain_failed() & 1
        assert torch.isnan(e.W).all() and torch.isnan(e.H).all()
        with pytest.raises(HipLibraryError, match='did not hand over cleanly'):
            e.check_status()
        with pytest.warns(RuntimeWarning, match='falls back to the plain launches'):
            y = e.separate(xs)
        assert np.array_equal(y, y_plain)
        assert lib.gccnmf_klnmf_plan(e.g.F, e.g.N, 1024, 24, 0) & 8 == 0          # the process now runs plain launches
    finally:
        lib.gccnmf_set_tuning(25, 0)
        lib.gccnmf_set_tuning(21, 1)
