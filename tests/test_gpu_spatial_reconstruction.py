"""-m gpu: spatial (multichannel Wiener) reconstruction (gccnmf_reconstruct with GCCNMF_RECONSTRUCT_RATIO and
GCCNMF_RECONSTRUCT_SPATIAL_BATCH, csrc/spatial.hip) against the float64 restatement tests/spatial_restatement.py of the SAME float32
inputs: the ratio-mode spec and X as the device holds them.

The bar is measured, not fixed: per case it is 4 x the largest distance of a float32 NumPy evaluation of the same
formulas from the float64 one (inputs rounded to float32 once, float64 only for the covariance sums and R~), distances relative to
max|X|; the factor covers the other association order of the 2 x 2 products and the reciprocal.  Every element is compared.
Measured on an MI355X: see the print of each test (-s) and DESIGN 4c."""
import hashlib

import numpy as np
import pytest

import spatial_restatement as SR
from conftest import golden
from oracle import gccnmf_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

RATIO, SPATIAL = 0x100, 1 << 16


@pytest.fixture(scope='module')
def lib():
    from gcc_nmf_amd import _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib()


def synthetic(F, T, K, S, seed):
    """float32 factors as tests/test_gpu_ratio_reconstruction.py builds them, with an X that has a structure between the channels."""
    rng = np.random.RandomState(seed)
    X = (rng.uniform(0.5, 2.0, (2, F, T)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (2, F, T)))).astype(np.complex64)
    W = rng.uniform(0.01, 1.0, (F, K)).astype(np.float32)
    W[F - 1] *= np.float32(100)
    W[:, K - 1] *= np.float32(100)
    H = rng.uniform(0.01, 1.0, (K, 2 * T)).astype(np.float32)
    am = rng.randint(0, S, (K, T)).astype(np.uint8)
    return W, H, am, X


def complex_of(t):
    a = t.cpu().numpy()
    return a[..., 0] + 1j * a[..., 1]


def device_stages(lib, files, S, masks=None):
    """files: [(W, H, argmax, X)] of one shape, as ONE batch through the C ABI.  The ratio call, a copy of its spec, then the spatial call
    on the same inputs with spec and the covariance workspace prefilled with a sentinel.  -> (ratio spec, spatial spec) as
    (B, S, 2, F, T) complex64, covariances (B, S, F, 4); the spatial call's padding (rows >= F, frames >= T) must be zeros."""
    from gcc_nmf_amd import _hip
    from gcc_nmf_amd.engine import Geometry
    B = len(files)
    F, K = files[0][0].shape
    T = files[0][3].shape[2]
    g = Geometry(F, T, K)
    Wp, Hp = np.zeros((B, g.Fp, g.Kp), np.float32), np.zeros((B, g.Kp, g.Np), np.float32)
    Ap, Xp = np.zeros((B, g.Kp, g.Tp), np.uint8), np.zeros((B, 2, g.Fp, g.Tp, 2), np.float32)
    for j, (W, H, am, X) in enumerate(files):
        Wp[j, :F, :K], Hp[j, :K, :2 * T], Ap[j, :K, :T] = W, H, am
        Xp[j, :, :F, :T, 0], Xp[j, :, :F, :T, 1] = X.real, X.imag
    d = lambda a: torch.from_numpy(a).cuda()
    dW, dH, dA, dX = d(Wp), d(Hp), d(Ap), d(Xp)
    dM = None
    if masks is not None:
        Mp = np.zeros((B, S, g.Kp, g.Tp), np.float32)
        Mp[:, :, :K, :T] = masks
        dM = d(Mp)
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: 0 if t is None else t.data_ptr()
    spec = torch.full((B, 2 * S, g.Fp, g.Tp, 2), float('nan'), dtype=torch.float32, device='cuda')
    assert lib.gccnmf_reconstruct(p(dW), p(dH), 0 if masks is not None else p(dA), p(dM), p(dX), 0, F, T, K, S | RATIO, B, 0, p(spec),
                                  stream) == 0
    ratio = complex_of(spec).reshape(B, S, 2, g.Fp, g.Tp)[:, :, :, :F, :T].astype(np.complex64)
    spec.fill_(float('nan'))
    cov = torch.full((_hip.reconstruct_spatial_workspace_floats(B, S, g.Fp),), -7.0, dtype=torch.float32, device='cuda')
    assert lib.gccnmf_reconstruct(p(dW), p(dH), 0 if masks is not None else p(dA), p(dM), p(dX), 0, F, T, K, S | RATIO, B | SPATIAL,
                                  p(cov), p(spec), stream) == 0
    torch.cuda.synchronize()
    sp = complex_of(spec).reshape(B, S, 2, g.Fp, g.Tp)
    assert (sp[:, :, :, F:, :] == 0).all() and (sp[:, :, :, :, T:] == 0).all(), 'output padding must be written as zeros'
    return ratio, sp[:, :, :, :F, :T].astype(np.complex64), cov.cpu().numpy().reshape(B, S, g.Fp, 4)[:, :, :F]


def check_against_restatement(E, X, got, what):
    """Every element of the device's spatial output against the float64 restatement of the device's own ratio spec, under the measured bar."""
    bar, err32, ref = SR.measured_bar(E, X)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), '%s: NaN where the definition has none, or the reverse' % what
    ok = np.isfinite(ref)
    scale = float(np.abs(X[np.isfinite(X)]).max())
    dist = float(np.abs(got[ok] - ref[ok]).max()) / scale if ok.any() else 0.0
    print('%s: float32 evaluation %.3g, bar %.3g, device %.3g of max|X| (%.2f of the bar)' % (what, err32, bar, dist, dist / bar if bar else 0))
    assert dist <= bar, (what, dist, bar)
    return bar, ref


CASES = [(513, 130, 64, 3), (201, 37, 50, 2), (513, 70, 64, 1), (513, 130, 128, 8), (33, 1, 16, 2)]


@pytest.mark.parametrize('shape', CASES)
def test_stage_against_the_restatement(lib, shape):
    F, T, K, S = shape
    W, H, am, X = synthetic(F, T, K, S, 400 + F + S)
    ratio, got, cov = device_stages(lib, [(W, H, am, X)], S)
    what = 'F=%d T=%d K=%d S=%d' % shape
    # R~: the device adds the frames in another (fixed) order in float64, then rounds to float32 once: at most one ulp of an entry of
    # magnitude below 4 (p_c / n <= 2, plus the loading)
    assert np.abs(cov[0].astype(np.float64) - SR.covariances(ratio[0])).max() <= 2.0 ** -22
    bar, ref = check_against_restatement(ratio[0], X, got[0], what)
    total = float(np.abs(got[0].astype(np.complex128).sum(axis=0) - X).max() / np.abs(X).max())
    print('%s: sum of the targets against the mixture %.3g of max|X|' % (what, total))
    assert total <= bar, 'the targets add up to the mixture within the same measured bar'
    if S == 1:
        assert float(np.abs(got[0, 0] - X).max() / np.abs(X).max()) <= bar, 'one target returns the mixture'


@pytest.fixture(scope='module')
def reference_factors():
    g = golden('dev1_hop256_K128')
    W, H, am = g['W_sub'].astype(np.float32), g['H_sub'].astype(np.float32), g['argmax'].astype(np.uint8)
    assert W.shape == (513, 128) and H.shape == (128, 1244) and am.shape == (128, 622)
    rng = np.random.RandomState(11)
    X = (rng.randn(2, 513, 622) + 1j * rng.randn(2, 513, 622)).astype(np.complex64)
    return W, H, am, X


def test_stage_on_the_reference_factors(lib, reference_factors):
    W, H, am, X = reference_factors
    ratio, got, _ = device_stages(lib, [(W, H, am, X)], 3)
    assert np.array_equal(ratio[0], device_stages(lib, [(W, H, am, X)], 3)[0][0])
    check_against_restatement(ratio[0], X, got[0], 'dev1 golden factors F=513 T=622 K=128 S=3')


def test_channel_swap(lib):
    """Swapping the channels of H and X swaps the channels of the output: the stated roundings are symmetric, so bit for bit."""
    F, T, K, S = 201, 37, 50, 3
    W, H, am, X = synthetic(F, T, K, S, 77)
    Hs = np.concatenate([H[:, T:], H[:, :T]], axis=1)
    _, got, _ = device_stages(lib, [(W, H, am, X)], S)
    _, swapped, _ = device_stages(lib, [(W, Hs, am, X[::-1].copy())], S)
    assert np.array_equal(swapped[0][:, ::-1], got[0])


def test_stage_does_not_depend_on_the_batch(lib):
    """The same file's operands alone and at positions 0 and 4 of a batch of 5, through the C ABI: the same bits."""
    F, T, K, S = 513, 150, 64, 3
    files = [synthetic(F, T, K, S, 300 + b) for b in range(5)]
    files[4] = files[0]
    _, alone, cov1 = device_stages(lib, files[:1], S)
    _, five, cov5 = device_stages(lib, files, S)
    assert np.isfinite(five).all()
    assert np.array_equal(five[0], alone[0]) and np.array_equal(five[4], alone[0])
    assert np.array_equal(cov5[0], cov1[0]) and np.array_equal(cov5[4], cov1[0])
    assert not np.array_equal(five[1], alone[0])


def test_edges(lib):
    """A target silent in one bin (R = I), an all-zero (f, t) (zero outputs), a NaN coefficient (a whole frame of a channel: it reaches every
    bin; test_nan_stays_in_its_bin has the NaN that stays in one bin)."""
    F, T, K, S = 201, 70, 48, 3
    W, H, am, X = synthetic(F, T, K, S, 91)
    am[:] = (np.arange(K) % S)[:, None]               # atom k belongs to target k mod S in every frame
    W[17, 1::S] = 0                                   # bin 17: target 1's numerator is 0 in every frame
    H[:, 5] = H[:, T + 5] = 0                         # frame 5: both channels' coefficients are 0 -> den = 0 -> every estimate 0
    ratio, got, cov = device_stages(lib, [(W, H, am, X)], S)
    assert (ratio[0][1, :, 17, :] == 0).all() and (ratio[0][:, :, :, 5] == 0).all()
    lam1 = np.float32(1 + SR.LOADING)
    assert np.array_equal(cov[0][1, 17], np.array([lam1, lam1, 0, 0], np.float32)), 'n = 0: R = I'
    assert (got[0][:, :, :, 5] == 0).all(), 'sum_j v_j = 0: zero for every target'
    assert (got[0][1, :, 17, :] == 0).all()
    assert np.isfinite(got[0]).all()
    check_against_restatement(ratio[0], X, got[0], 'edges: silent target, silent frame')

    H[3, 9] = np.nan                                  # channel 0, frame 9, an atom of target 0
    ratio, got, _ = device_stages(lib, [(W, H, am, X)], S)
    ref = SR.spatial_filter(ratio[0], X)
    assert np.isnan(ratio[0][:, 0, :, 9]).all() and np.isfinite(ratio[0][:, 1]).all()
    # the ratio stage makes channel 0 of frame 9 NaN in every bin and target: every covariance of the file is NaN, and so is the output
    assert np.isnan(ref).sum() > 0 and np.array_equal(np.isnan(got[0]), np.isnan(ref))
    assert (got[0][:, :, :, 5] == 0).all(), 'the zero rule comes first: frame 5 stays 0'
    check_against_restatement(ratio[0], X, got[0], 'edges: NaN coefficient')


def test_nan_stays_in_its_bin(lib):
    """One NaN element of X: the ratio stage makes that (channel, bin, frame) NaN for every target, so the covariances of that bin are
    NaN and the bin is NaN in every frame, target and channel (but for a frame under the zero rule); every other bin stays finite."""
    F, T, K, S = 201, 70, 48, 3
    W, H, am, X = synthetic(F, T, K, S, 93)
    H[:, 5] = H[:, T + 5] = 0                         # frame 5: every estimate 0
    X[0, 23, 30] = np.nan
    ratio, got, cov = device_stages(lib, [(W, H, am, X)], S)
    hit = np.isnan(ratio[0])
    assert hit[:, 0, 23, 30].all() and hit.sum() == S, 'the ratio stage: that element of channel 0, every target'
    assert np.isnan(cov[0][:, 23]).all() and np.isfinite(np.delete(cov[0], 23, axis=1)).all()
    frames = np.arange(T) != 5
    assert np.isnan(got[0][:, :, 23, frames]).all() and (got[0][:, :, 23, 5] == 0).all()
    assert np.isfinite(np.delete(got[0], 23, axis=2)).all(), 'the other bins stay finite'
    check_against_restatement(ratio[0], X, got[0], 'edges: NaN in one element of X')


def test_nearly_silent_frame(lib):
    """A frame with |X| ~ 1e-10: the determinant of the unscaled form (~ 1e-43) is subnormal, which is why the kernel works on the
    powers scaled by 2^-e.  The frame is finite and, relative to ITS OWN max|X|, within 4 x the distance of the (scaled) float32
    evaluation from float64 in that frame; the whole file is within its bar as everywhere else."""
    F, T, K, S = 201, 70, 48, 3
    W, H, am, X = synthetic(F, T, K, S, 95)
    X[:, :, 11] *= np.float32(1e-10)
    ratio, got, _ = device_stages(lib, [(W, H, am, X)], S)
    assert np.isfinite(got[0]).all()
    check_against_restatement(ratio[0], X, got[0], 'nearly silent frame, whole file')
    ref, f32 = SR.spatial_filter(ratio[0], X), SR.spatial_filter(ratio[0], X, np.float32)
    quiet = float(np.abs(X[:, :, 11]).max())
    assert 1e-11 < quiet < 1e-9
    err = float(np.abs(f32[..., 11] - ref[..., 11]).max()) / quiet
    dist = float(np.abs(got[0][..., 11] - ref[..., 11]).max()) / quiet
    print('nearly silent frame: float32 evaluation %.3g, bar %.3g, device %.3g of the frame\'s max|X|' % (err, SR.BAR_FACTOR * err, dist))
    assert dist <= SR.BAR_FACTOR * err
    literal = SR.spatial_filter(ratio[0], X, np.float32, scaled=False)
    assert not np.isfinite(literal[..., 11]).all() or float(np.abs(literal[..., 11] - ref[..., 11]).max()) / quiet > SR.BAR_FACTOR * err, \
        'the unscaled float32 form does not survive this frame'


# ---- the engine ------------------------------------------------------------------------------------------------------------------

def engine(n, **kw):
    from gcc_nmf_amd.engine import GCCNMFEngine
    return GCCNMFEngine(n, **kw)


def sha(e):
    torch.cuda.synchronize()
    return hashlib.sha256(e.spec.cpu().numpy().tobytes()).hexdigest()


def waveforms(spec, hop=256, ws=1024):
    flat = spec.reshape((-1,) + spec.shape[-2:])
    y = np.array([O.istft(s.astype(np.complex64), hop, ws, np.hanning) for s in flat]).astype(np.float64) * (hop / float(ws) * 2)
    return y.reshape(spec.shape[:-2] + (-1,))


def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def test_engine_modes_on_dev1(lib, dev1):
    """'direct' and 'ratio' are what engines built without the new keyword value produce (SHA-256 of spec); 'spatial' is the restatement
    of the ratio spec; its targets add up to the mixture; the drop-in function gives the engine's bits."""
    from gcc_nmf_amd import gccNMFFunctions as G
    x, sr = dev1
    kw = dict(sampleRate=sr, dictionarySize=128, numIterations=100)
    e0 = engine(x.shape[1], **kw)
    y0 = e0.separate(x)[0]
    er = engine(x.shape[1], reconstruction='ratio', **kw)
    er.separate(x)
    es = engine(x.shape[1], reconstruction='spatial', **kw)
    ys = es.separate(x)[0]
    assert es.ws_rec is None and es.ws_cov is not None
    for a, b in zip(tuple(es.get_WH()) + (es.get_argmax(), es.get_X()), tuple(e0.get_WH()) + (e0.get_argmax(), e0.get_X())):
        assert np.array_equal(a, b), 'everything up to the masks is shared'
    direct_sha, ratio_sha, spatial_sha = sha(e0), sha(er), sha(es)
    assert len({direct_sha, ratio_sha, spatial_sha}) == 3
    # one engine through all three modes: the bits of each mode's own engine
    e0.reconstruction = 'ratio'
    e0.reconstruct()
    assert sha(e0) == ratio_sha
    e0.reconstruction = 'spatial'
    e0.reconstruct()
    assert sha(e0) == spatial_sha
    e0.reconstruction = 'direct'
    e0.reconstruct()
    assert sha(e0) == direct_sha
    ed = engine(x.shape[1], reconstruction='direct', **kw)         # a second engine that never saw the other modes
    yd = ed.separate(x)[0]
    assert sha(ed) == direct_sha and np.array_equal(yd, y0)
    e0.istft()
    torch.cuda.synchronize()
    assert np.array_equal(e0.y.cpu().numpy()[0], y0)

    E, X, spec = er.get_spec()[0], es.get_X()[0], es.get_spec()[0]
    bar, ref = check_against_restatement(E, X, spec, 'engine on dev1')
    total = float(np.abs(spec.astype(np.complex128).sum(axis=0) - X).max() / np.abs(X).max())
    print('engine on dev1: sum of the targets against the mixture %.3g of max|X| (bar %.3g)' % (total, bar))
    assert total <= bar
    assert ys.shape == y0.shape and np.isfinite(ys).all()
    r_y = rms(ys - waveforms(spec))
    print('engine on dev1: waveforms against the oracle inverse STFT of get_spec() %.3g rms' % r_y)
    assert r_y < 1e-4                                          # the waveform bar of the ratio mode's test (full scale 1)

    W, H = es.get_WH()
    W, H, scores = W[0], H[0], es.get_scores()[0]
    stereoH = np.array(np.hsplit(H, 2))
    # resident mode: the masks come back with the arg-max image they were expanded from, so the ratio stage takes its one-hot form, as
    # in the engine (in the default mode every mask array is a soft mask: den = W.H_c, an ulp away)
    G.set_resident(True)
    try:
        masks = G.getTargetCoefficientMasks(scores, 3)
        est = G.getTargetSpectrogramEstimates(masks, X, W, stereoH, reconstruction='spatial')
    finally:
        G.set_resident(False)
    assert est.shape == spec.shape and np.array_equal(est, spec), 'the drop-in function runs the same two stages on the same operands'
    soft = (0.9 * masks + 0.05).astype(np.float32)
    soft_ratio = G.getTargetSpectrogramEstimates(soft, X, W, stereoH, reconstruction='ratio')
    soft_spatial = G.getTargetSpectrogramEstimates(soft, X, W, stereoH, reconstruction='spatial')
    check_against_restatement(soft_ratio, X, soft_spatial, 'drop-in, soft masks')


def test_engine_with_tracks_and_with_a_dictionary(dev1):
    x, sr = dev1
    e = engine(x.shape[1], sampleRate=sr, dictionarySize=128, numIterations=100)
    e.separate(x)
    W = e.get_WH()[0][0]
    T = e.g.T
    for kw in (dict(dictionarySize=128, tdoaTracking=True, localizationWindowSize=2 * T - 1), dict(dictionaryW=W)):
        es = engine(x.shape[1], sampleRate=sr, numIterations=100, reconstruction='spatial', **kw)
        y = es.separate(x)[0]
        spec = es.get_spec()[0]
        assert y.shape == (3, 2, 256 * (T - 1)) and np.isfinite(y).all() and np.isfinite(spec).all()
        assert rms(y - waveforms(spec)) < 1e-4
        er = engine(x.shape[1], sampleRate=sr, numIterations=100, reconstruction='ratio', **kw)
        er.separate(x)
        check_against_restatement(er.get_spec()[0], es.get_X()[0], spec, 'engine, %s' % sorted(kw)[0])


def test_batch_independence(lib, dev1):
    """A file alone, at positions 0 and 4 of a batch of 5 and in a ragged batch: bit-identical spec and waveforms.  KL-NMF picks its GEMM
    tile by launch size, so the runs are made under tuning key 2 = 1, as in tests/test_gpu_ratio_reconstruction.py."""
    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_batch
    x, sr = dev1
    n = x.shape[1]
    kw = dict(sampleRate=sr, dictionarySize=128, numIterations=30, reconstruction='spatial')
    others = synthetic_batch(3, 3, numSamples=n)
    assert lib.gccnmf_set_tuning(2, 1) == 0
    try:
        e1 = engine(n, **kw)
        y1 = e1.separate(x)[0]
        alone = e1.get_spec()[0]
        e5 = engine(n, batch=5, **kw)
        y5 = e5.separate(np.concatenate([x[None], others, x[None]]))
        five = e5.get_spec()
        assert np.array_equal(e5.get_WH()[1][0], e1.get_WH()[1][0]), 'the factors themselves differ: nothing to compare downstream'
        rg = GCCNMFEngine(lengths=[160000, 80000, 160000], **kw)
        yr = rg.separate([x, others[0][:, :80000], others[1]])
        sub, k = rg.file(0)
        assert sub.reconstruction == 'spatial'
        ragged = sub.get_spec()[k]
    finally:
        lib.gccnmf_set_tuning(2, 0)
    assert np.isfinite(alone).all()
    assert np.array_equal(five[0], alone) and np.array_equal(five[4], alone) and np.array_equal(ragged, alone)
    assert np.array_equal(y5[0], y1) and np.array_equal(y5[4], y1) and np.array_equal(yr[0], y1)
