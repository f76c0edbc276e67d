"""-m gpu: EM refinement of the spatial reconstruction (gccnmf_reconstruct with GCCNMF_RECONSTRUCT_SPATIAL_ITERATIONS(n) on S,
csrc/spatial_em.hip) against the float64 restatement tests/spatial_em_restatement.py of the SAME float32 inputs: the ratio-mode spec
and X as the device holds them.

The bar is measured, not fixed, as in tests/test_gpu_spatial_reconstruction.py: per case it is 4 x the largest distance
of a float32 NumPy evaluation of the same formulas from the float64 one (inputs rounded to float32 once, float64 only for the frame
sums and R~, the frames added in another order), distances relative to max|X|.  It rests on a condition that measured_bar asserts:
the zero pattern of the powers and the NaN pattern are the same in both evaluations.  Every element is compared.
Measured on an MI355X: see the print of each test (-s) and DESIGN 4h."""
import hashlib

import numpy as np
import pytest

import spatial_em_restatement as EM
import spatial_restatement as SR
from oracle import gccnmf_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

RATIO, SPATIAL = 0x100, 1 << 16
ITER = lambda n: n << 20
SENTINEL = -7.0


@pytest.fixture(scope='module')
def lib():
    from gcc_nmf_amd import _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib()


def synthetic(F, T, K, S, seed):
    """float32 factors as tests/test_gpu_spatial_reconstruction.py builds them."""
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


def device_stages(lib, files, S, n, word=None):
    """files: [(W, H, argmax, X)] of one shape, as ONE batch through the C ABI.  The ratio call, a copy of its spec, then the spatial
    call with n iterations on the same inputs, spec prefilled with NaN and the workspace with a sentinel.  -> (ratio spec, output spec)
    as (B, S, 2, F, T) complex64, covariances (B, S, F, 4), the powers region (B, S, Fp, Tp) as the call left it."""
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
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    spec = torch.full((B, 2 * S, g.Fp, g.Tp, 2), float('nan'), dtype=torch.float32, device='cuda')
    assert lib.gccnmf_reconstruct(p(dW), p(dH), p(dA), 0, p(dX), 0, F, T, K, S | RATIO, B, 0, p(spec), stream) == 0
    ratio = complex_of(spec).reshape(B, S, 2, g.Fp, g.Tp)[:, :, :, :F, :T].astype(np.complex64)
    spec.fill_(float('nan'))
    ncov = _hip.reconstruct_spatial_workspace_floats(B, S, g.Fp)
    total = _hip.reconstruct_spatial_em_workspace_floats(B, S, g.Fp, g.Tp)
    assert total == ncov + B * S * g.Fp * g.Tp and _hip.reconstruct_workspace_floats('spatial', T, K, S, B, g.Fp, iterations=max(n, 1)) == total
    ws = torch.full((total,), SENTINEL, dtype=torch.float32, device='cuda')
    word = (S | RATIO | ITER(n)) if word is None else word
    assert lib.gccnmf_reconstruct(p(dW), p(dH), p(dA), 0, p(dX), 0, F, T, K, word, B | SPATIAL, p(ws), p(spec), stream) == 0
    torch.cuda.synchronize()
    sp = complex_of(spec).reshape(B, S, 2, g.Fp, g.Tp)
    assert (sp[:, :, :, F:, :] == 0).all() and (sp[:, :, :, :, T:] == 0).all(), 'output padding must be written as zeros'
    host = ws.cpu().numpy()
    return (ratio, sp[:, :, :, :F, :T].astype(np.complex64), host[:ncov].reshape(B, S, g.Fp, 4)[:, :, :F],
            host[ncov:].reshape(B, S, g.Fp, g.Tp))


def check_against_restatement(E, X, n, got, what):
    """Every element of the device's output against the float64 restatement of the device's own ratio spec, under the measured bar."""
    bar, err32, ref = EM.measured_bar(E, X, n)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), '%s: NaN where the definition has none, or the reverse' % what
    ok = np.isfinite(ref)
    scale = float(np.abs(X[np.isfinite(X)]).max())
    dist = float(np.abs(got[ok] - ref[ok]).max()) / scale if ok.any() else 0.0
    print('%s: float32 evaluation %.3g, bar %.3g, device %.3g of max|X| (%.2f of the bar)' % (what, err32, bar, dist, dist / bar if bar else 0))
    assert dist <= bar, (what, dist, bar)
    return bar, ref


CASES = [(33, 1, 16, 2, 1), (33, 1, 16, 2, 3), (201, 37, 50, 2, 2), (513, 130, 64, 3, 1), (513, 130, 64, 3, 5), (513, 130, 128, 8, 2),
         (513, 70, 64, 1, 3)]


@pytest.mark.parametrize('case', CASES)
def test_stage_against_the_restatement(lib, case):
    F, T, K, S, n = case
    W, H, am, X = synthetic(F, T, K, S, 400 + F + S)
    ratio, got, cov, powers = device_stages(lib, [(W, H, am, X)], S, n)
    what = 'F=%d T=%d K=%d S=%d n=%d' % case
    bar, ref = check_against_restatement(ratio[0], X, n, got[0], what)
    v, R = EM.refine(ratio[0], X, n)
    # the workspace on return: the final powers (frames < T of rows < F; the odd frame beside T - 1 is written as 0, nothing else is
    # touched) and the final R~, both within the bar's own scale of the float64 recursion
    assert np.array_equal(EM.refine(ratio[0], X, n, np.float32)[0] == 0, powers[0][:, :F, :T] == 0), 'the device skips the frames the definition skips'
    assert np.abs(powers[0][:, :F, :T] - v).max() <= 1e-3 * np.abs(v).max() and np.abs(cov[0] - R).max() <= 1e-3
    assert (powers[0][:, F:] == SENTINEL).all() and (powers[0][:, :, T + T % 2:] == SENTINEL).all()
    if T % 2:
        assert (powers[0][:, :F, T] == 0).all()
    total = float(np.abs(got[0].astype(np.complex128).sum(axis=0) - X).max() / np.abs(X).max())
    print('%s: sum of the targets against the mixture %.3g of max|X|' % (what, total))
    assert total <= bar, 'the targets add up to the mixture within the same measured bar'
    if S == 1:
        assert float(np.abs(got[0, 0] - X).max() / np.abs(X).max()) <= bar, 'one target returns the mixture'
    else:
        assert np.abs(got[0] - SR.spatial_filter(ratio[0], X)).max() > 10 * bar * np.abs(X).max(), 'the iterations ran'


def test_nan_stays_in_its_bin(lib):
    """One NaN element of X (as in tests/test_gpu_spatial_reconstruction.py): that bin is NaN in every frame, target and channel but
    for a frame under the zero rule; every other bin stays finite through the iterations."""
    F, T, K, S, n = 201, 70, 48, 3, 2
    W, H, am, X = synthetic(F, T, K, S, 93)
    H[:, 5] = H[:, T + 5] = 0                         # frame 5: every estimate 0
    X[0, 23, 30] = np.nan
    ratio, got, cov, powers = device_stages(lib, [(W, H, am, X)], S, n)
    assert np.isnan(cov[0][:, 23]).all() and np.isfinite(np.delete(cov[0], 23, axis=1)).all()
    frames = np.arange(T) != 5
    assert np.isnan(got[0][:, :, 23, frames]).all() and (got[0][:, :, 23, 5] == 0).all()
    assert np.isfinite(np.delete(got[0], 23, axis=2)).all(), 'the other bins stay finite'
    assert (powers[0][:, :F, 5] == 0).all()
    check_against_restatement(ratio[0], X, n, got[0], 'NaN in one element of X, n=2')


def test_nearly_silent_frame(lib):
    """A frame with |X| ~ 1e-10: finite, within the whole file's bar, and within 4 x the float32 evaluation's own distance relative to
    THAT frame's max|X| -- the scaling by 2^-e carries through the iterations."""
    F, T, K, S, n = 201, 70, 48, 3, 2
    W, H, am, X = synthetic(F, T, K, S, 95)
    X[:, :, 11] *= np.float32(1e-10)
    ratio, got, _, _ = device_stages(lib, [(W, H, am, X)], S, n)
    assert np.isfinite(got[0]).all()
    check_against_restatement(ratio[0], X, n, got[0], 'nearly silent frame, whole file, n=2')
    ref, f32 = EM.spatial_em(ratio[0], X, n), EM.spatial_em(ratio[0], X, n, np.float32)
    quiet = float(np.abs(X[:, :, 11]).max())
    assert 1e-11 < quiet < 1e-9
    err = float(np.abs(f32[..., 11] - ref[..., 11]).max()) / quiet
    dist = float(np.abs(got[0][..., 11] - ref[..., 11]).max()) / quiet
    print('nearly silent frame: float32 evaluation %.3g, bar %.3g, device %.3g of the frame\'s max|X|' % (err, EM.BAR_FACTOR * err, dist))
    assert dist <= EM.BAR_FACTOR * err


def test_stage_does_not_depend_on_the_batch(lib):
    """The same file's operands alone and at positions 0 and 2 of a batch of 3, through the C ABI: the same bits."""
    F, T, K, S, n = 513, 150, 64, 3, 3
    files = [synthetic(F, T, K, S, 300 + b) for b in range(3)]
    files[2] = files[0]
    _, alone, cov1, pw1 = device_stages(lib, files[:1], S, n)
    _, three, cov3, pw3 = device_stages(lib, files, S, n)
    assert np.isfinite(three).all()
    assert np.array_equal(three[0], alone[0]) and np.array_equal(three[2], alone[0])
    assert np.array_equal(cov3[0], cov1[0]) and np.array_equal(cov3[2], cov1[0])
    assert np.array_equal(pw3[0], pw1[0]) and np.array_equal(pw3[2], pw1[0])
    assert not np.array_equal(three[1], alone[0])


def test_without_the_iteration_bits_nothing_changes(lib):
    """ITERATIONS(0) is no bit at all: the spec of the spatial mode (SHA-256 against a call with the covariance workspace alone, the
    one tests/test_gpu_spatial_reconstruction.py checks), and the powers region of a larger workspace is not touched."""
    from gcc_nmf_amd import _hip
    F, T, K, S = 201, 70, 48, 3
    f = synthetic(F, T, K, S, 97)
    _, got, cov, powers = device_stages(lib, [f], S, 0)
    assert (powers == SENTINEL).all(), 'n = 0 does not touch the powers'
    _, again, cov2, _ = device_stages(lib, [f], S, 0, word=S | RATIO | ITER(0))
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    assert sha(again) == sha(got) and sha(cov2) == sha(cov)
    from test_gpu_spatial_reconstruction import device_stages as spatial_stages
    _, today, cov0 = spatial_stages(lib, [f], S)
    assert sha(today) == sha(got) and sha(cov0) == sha(cov)
    _, one, _, _ = device_stages(lib, [f], S, 1)
    assert sha(one) != sha(got)


# ---- the engine ------------------------------------------------------------------------------------------------------------------

def waveforms(spec, hop=256, ws=1024):
    flat = spec.reshape((-1,) + spec.shape[-2:])
    y = np.array([O.istft(s.astype(np.complex64), hop, ws, np.hanning) for s in flat]).astype(np.float64) * (hop / float(ws) * 2)
    return y.reshape(spec.shape[:-2] + (-1,))


def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def test_engine_and_dropin_on_dev1(lib, dev1):
    """One engine run on the committed dev1 mixture with spatialIterations=2: get_spec() against the restatement of the ratio spec, the
    waveforms against the oracle's inverse STFT; an engine whose attribute is raised later reallocates and gives the same bits; the
    drop-in function with soft masks."""
    from gcc_nmf_amd import gccNMFFunctions as G
    from gcc_nmf_amd.engine import GCCNMFEngine
    x, sr = dev1
    kw = dict(sampleRate=sr, dictionarySize=128, numIterations=30, reconstruction='spatial')
    e = GCCNMFEngine(x.shape[1], spatialIterations=2, **kw)
    y = e.separate(x)[0]
    g = e.g
    assert e.ws_cov.numel() == 4 * 3 * g.Fp + 3 * g.Fp * g.Tp
    spec, X = e.get_spec()[0], e.get_X()[0]
    e0 = GCCNMFEngine(x.shape[1], **kw)
    e0.separate(x)
    assert e0.spatialIterations == 0 and e0.ws_cov.numel() == 4 * 3 * g.Fp
    spec0 = e0.get_spec()[0]
    e0.reconstruction = 'ratio'
    e0.reconstruct()
    E = e0.get_spec()[0]
    bar, ref = check_against_restatement(E, X, 2, spec, 'engine on dev1, n=2')
    assert np.abs(spec - spec0).max() > 10 * bar * np.abs(X).max()
    total = float(np.abs(spec.astype(np.complex128).sum(axis=0) - X).max() / np.abs(X).max())
    print('engine on dev1: sum of the targets against the mixture %.3g of max|X| (bar %.3g)' % (total, bar))
    assert total <= bar
    r_y = rms(y - waveforms(spec))
    print('engine on dev1: waveforms against the oracle inverse STFT of get_spec() %.3g rms' % r_y)
    assert y.shape == (3, 2, 256 * (g.T - 1)) and r_y < 1e-4       # the waveform bar of the other modes' tests (full scale 1)
    # raised later: the workspace grows at the next reconstruct(), and the bits are those of the engine built with the keyword
    e0.reconstruction, e0.spatialIterations = 'spatial', 2
    e0.reconstruct()
    assert e0.ws_cov.numel() == e.ws_cov.numel() and np.array_equal(e0.get_spec()[0], spec)
    e0.spatialIterations = 0
    e0.reconstruct()
    assert np.array_equal(e0.get_spec()[0], spec0)

    W, H = e.get_WH()
    W, H, scores = W[0], H[0], e.get_scores()[0]
    stereoH = np.array(np.hsplit(H, 2))
    masks = G.getTargetCoefficientMasks(scores, 3)
    soft = (0.9 * masks + 0.05).astype(np.float32)
    soft_ratio = G.getTargetSpectrogramEstimates(soft, X, W, stereoH, reconstruction='ratio')
    soft_em = G.getTargetSpectrogramEstimates(soft, X, W, stereoH, reconstruction='spatial', spatialIterations=2)
    check_against_restatement(soft_ratio, X, 2, soft_em, 'drop-in, soft masks, n=2')


def ratio_spec_of(e):
    """The ratio-mode spec of an engine that has run: the input of its spatial stage."""
    mode, n = e.reconstruction, e.spatialIterations
    e.spatialIterations, e.reconstruction = 0, 'ratio'
    e.reconstruct()
    E = e.get_spec()
    e.reconstruction, e.spatialIterations = mode, n
    return E


@pytest.mark.parametrize('variant', ['auto', 'lengths', 'enhancement'])
def test_engine_variants_take_the_keyword(dev1, variant):
    """numTargets='auto' (the empty slots stay exactly zero), lengths= (every length's engine gets the keyword) and the enhancement engine
    (S = 2) with spatialIterations=2: get_spec() against the restatement of the engine's own ratio spec."""
    from gcc_nmf_amd.engine import GCCNMFEngine, GCCNMFEnhancementEngine
    x, sr = dev1
    n = x.shape[1]
    kw = dict(sampleRate=sr, dictionarySize=64, numIterations=30, reconstruction='spatial', spatialIterations=2)
    if variant == 'auto':
        from gcc_nmf_amd.synthetic import synthetic_mixture
        two = synthetic_mixture(0, 32000, 16000, delays=(-20, 27))      # the two-talker file of tests/test_gpu_source_count.py
        e = GCCNMFEngine(32000, numTargets='auto', maxTargets=4, **dict(kw, sampleRate=16000))
        y = e.separate(two)[0]
        count = int(e.get_num_sources()[0])
        spec = e.get_spec()[0]
        assert count == 2, 'the case needs an empty slot'
        assert (spec[count:] == 0).all() and (y[count:] == 0).all(), 'an empty slot stays exactly zero'
        g = e.g
        cov = e.ws_cov[:4 * 4 * g.Fp].cpu().numpy().reshape(4, g.Fp, 4)[count:, :g.F]
        lam1 = np.float32(1 + SR.LOADING)
        assert (cov == np.array([lam1, lam1, 0, 0], np.float32)).all(), 'and keeps R~ = (1 + lambda) I'
    elif variant == 'lengths':
        rg = GCCNMFEngine(lengths=[n, n // 2], **kw)
        rg.separate([x, x[:, :n // 2]])
        assert rg.spatialIterations == 2
        e, k = rg.file(1)
        assert k == 0 and e.spatialIterations == 2 and e.g.T < 622
        spec = e.get_spec()[0]
    else:
        e = GCCNMFEnhancementEngine(n, **kw)
        y = e.separate(x)[0]
        spec = e.get_spec()[0]
        assert spec.shape[0] == 2 and y.shape[0] == 2 and np.isfinite(y).all()
    E, X = ratio_spec_of(e)[0], e.get_X()[0]
    assert np.isfinite(spec).all()
    bar, _ = check_against_restatement(E, X, 2, spec, 'engine, %s, n=2' % variant)
    assert np.abs(spec.astype(np.complex128).sum(axis=0) - X).max() <= bar * np.abs(X).max()
    assert np.abs(spec - SR.spatial_filter(E, X)).max() > 10 * bar * np.abs(X).max(), 'the iterations ran'
