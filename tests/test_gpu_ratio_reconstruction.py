"""-m gpu: ratio-mask (Wiener-like) reconstruction (gccnmf_reconstruct with GCCNMF_RECONSTRUCT_RATIO, csrc/ratio.hip) against the
float64 restatement tests/ratio_restatement.py of the SAME float32 inputs, with itself (partition of the mixture, S = 1, batch
independence) and with the direct mode (everything up to the masks is shared).

Bounds, u = 2^-24 (f32 unit roundoff), elementwise and relative to |X| (the quotient num_i / den is at most 1):
  one-hot form   |S - ref| <= (2K + 5) u |X|   num_i and den are sums of K non-negative f32 products (relative error <= K u each, no
                                               cancellation), one quotient, one product
  soft form      |S - ref| <= (3K + 5) u |X|   the mask products add one rounding per term
  partition      |sum_i S_i - X| <= (3S + 2) u |X|   S quotients, S - 1 additions in den, S products, the rest slack
Measured on an MI355X: see the print of each test (-s)."""
import numpy as np
import pytest

import ratio_restatement as R
from conftest import golden
from oracle import gccnmf_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

RATIO = 0x100
U = 2.0 ** -24


@pytest.fixture(scope='module')
def lib():
    from gcc_nmf_amd import _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib()


def device_ratio(lib, W, H, X, S, argmax=None, masks=None):
    """One file through the C ABI: zero-padded operands, NaN-filled output, no workspace, no |X|.  -> (S, 2, F, T) complex64; the
    padding of the output (rows >= F, frames >= T) must have been written as zeros."""
    from gcc_nmf_amd.engine import Geometry
    F, K = W.shape
    T = X.shape[2]
    g = Geometry(F, T, K)
    Wp = np.zeros((g.Fp, g.Kp), np.float32)
    Wp[:F, :K] = W
    Hp = np.zeros((g.Kp, g.Np), np.float32)
    Hp[:K, :2 * T] = H
    Xp = np.zeros((2, g.Fp, g.Tp, 2), np.float32)
    Xp[:, :F, :T, 0], Xp[:, :F, :T, 1] = X.real, X.imag
    d = lambda a: torch.from_numpy(a).cuda()
    dW, dH, dX = d(Wp), d(Hp), d(Xp)
    dA = dM = None
    if masks is None:
        Ap = np.zeros((g.Kp, g.Tp), np.uint8)
        Ap[:K, :T] = argmax
        dA = d(Ap)
    else:
        Mp = np.full((S, g.Kp, g.Tp), np.float32(7.0))          # the padding of a caller's mask buffer is not the library's: garbage
        Mp[:, :K, :T] = masks
        dM = d(Mp)
    spec = torch.full((2 * S, g.Fp, g.Tp, 2), float('nan'), dtype=torch.float32, device='cuda')
    p = lambda t: 0 if t is None else t.data_ptr()
    rc = lib.gccnmf_reconstruct(p(dW), p(dH), p(dA), p(dM), p(dX), 0, F, T, K, S | RATIO, 1, 0, p(spec),
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    sp = spec.cpu().numpy()
    sp = (sp[..., 0] + 1j * sp[..., 1]).reshape(S, 2, g.Fp, g.Tp)
    assert (sp[:, :, F:, :] == 0).all() and (sp[:, :, :, T:] == 0).all(), 'output padding must be written as zeros'
    return sp[:, :, :F, :T].astype(np.complex64)


def worst(err, X, bound):
    """largest |err| / (bound u |X|) over the elements; <= 1 passes"""
    return float((np.abs(err) / (bound * U * np.abs(X)[None])).max())


def synthetic(F, T, K, S, seed):
    """float32 factors as tests/test_gpu_gcc_stages.py builds them: |X| in [0.5, 2]; W, H in [0.01, 1] with W's last row and last atom
    x100 (the VALU tail row / the last reduction index: a kernel that drops or misplaces them is far outside the bound)."""
    rng = np.random.RandomState(seed)
    X = (rng.uniform(0.5, 2.0, (2, F, T)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (2, F, T)))).astype(np.complex64)
    W = rng.uniform(0.01, 1.0, (F, K)).astype(np.float32)
    W[F - 1] *= np.float32(100)
    W[:, K - 1] *= np.float32(100)
    H = rng.uniform(0.01, 1.0, (K, 2 * T)).astype(np.float32)
    am = rng.randint(0, S, (K, T)).astype(np.uint8)
    masks = rng.uniform(0.0, 1.0, (S, K, T)).astype(np.float32)
    return W, H, am, masks, X


def check_one_hot(lib, W, H, am, S, X, what):
    K = W.shape[1]
    ref = R.ratio_one_hot(W, H, am, S, X)
    den = R.denominators(W, H, argmax=am, S=S)
    assert (den > 0).all(), '%s: den > 0 everywhere here, nothing is excluded (min %.3g)' % (what, den.min())
    sp = device_ratio(lib, W, H, X, S, argmax=am)
    w4 = worst(sp - ref, X, 2 * K + 5)
    w5 = worst(sp.astype(np.complex128).sum(axis=0)[None] - X[None], X, 3 * S + 2)
    print('%s: one-hot error %.3g of the (2K+5)u|X| bound (%.3g u|X|), partition %.3g of the (3S+2)u|X| bound (%.3g u|X|)'
          % (what, w4, w4 * (2 * K + 5), w5, w5 * (3 * S + 2)))
    assert w4 <= 1, (what, w4)
    assert w5 <= 1, (what, w5)
    return sp


def check_soft(lib, W, H, masks, X, what):
    S, K = masks.shape[0], W.shape[1]
    ref = R.ratio_soft(W, H, masks, X)
    assert (R.denominators(W, H, masks=masks) > 0).all()
    sp = device_ratio(lib, W, H, X, S, masks=masks)
    w6 = worst(sp - ref, X, 3 * K + 5)
    print('%s: soft error %.3g of the (3K+5)u|X| bound (%.3g u|X|)' % (what, w6, w6 * (3 * K + 5)))
    assert w6 <= 1, (what, w6)
    return sp


@pytest.fixture(scope='module')
def reference_factors():
    g = golden('dev1_hop256_K128')
    W, H, am = g['W_sub'].astype(np.float32), g['H_sub'].astype(np.float32), g['argmax'].astype(np.uint8)
    assert W.shape == (513, 128) and H.shape == (128, 1244) and am.shape == (128, 622)
    rng = np.random.RandomState(11)
    X = (rng.randn(2, 513, 622) + 1j * rng.randn(2, 513, 622)).astype(np.complex64)
    return W, H, am, X


def test_one_hot_on_the_reference_factors(lib, reference_factors):
    """Checks 4 and 5 on the reference's own W, H and arg-max (K = 128, F = 513: the VALU tail row, T = 622: a partial frame tile)."""
    W, H, am, X = reference_factors
    check_one_hot(lib, W, H, am, 3, X, 'dev1 golden factors')


@pytest.mark.parametrize('S', [1, 3, 8])
def test_one_hot_K1024(lib, S):
    W, H, am, _, X = synthetic(513, 130, 1024, S, 100 + S)
    sp = check_one_hot(lib, W, H, am, S, X, 'synthetic K=1024 S=%d' % S)
    if S == 1:
        assert np.array_equal(sp[0], X), 'one target: the quotient is exactly 1, S = X bit for bit'


def test_one_hot_odd_shape(lib):
    """F = 201 (no tail row: the last bin tile is padded), T = 37 (less than one frame tile), K = 50 (not a multiple of the k chunk)."""
    W, H, am, _, X = synthetic(201, 37, 50, 3, 7)
    check_one_hot(lib, W, H, am, 3, X, 'odd shape F=201 T=37 K=50')


def test_one_target_returns_the_mixture(lib, reference_factors):
    W, H, am, X = reference_factors
    sp = device_ratio(lib, W, H, X, 1, argmax=np.zeros_like(am))
    assert np.array_equal(sp[0], X)


@pytest.mark.parametrize('shape', [(513, 622, 128, 3), (513, 130, 1024, 3), (513, 130, 1024, 8), (201, 37, 50, 3), (513, 70, 64, 1)])
def test_soft_masks(lib, reference_factors, shape):
    """Check 6: random masks in [0, 1], den = W.H_c."""
    F, T, K, S = shape
    if (F, T, K) == (513, 622, 128):
        W, H, _, X = reference_factors
        masks = np.random.RandomState(3).uniform(0.0, 1.0, (S, K, T)).astype(np.float32)
    else:
        W, H, _, masks, X = synthetic(F, T, K, S, 200 + K + S)
    check_soft(lib, W, H, masks, X, 'soft F=%d T=%d K=%d S=%d' % shape)


@pytest.mark.parametrize('form', ['one-hot', 'soft'])
def test_zero_denominator_and_nan(lib, form):
    """Check 7: a frame whose coefficients are all zero gives exactly 0 for every target; a NaN coefficient gives NaN in that frame of that
    channel and nowhere else; every other element stays within its bound."""
    F, T, K, S = 513, 100, 128, 3
    W, H, am, masks, X = synthetic(F, T, K, S, 31)
    H[:, 5] = 0                  # channel 0, frame 5
    H[:, T + 70] = 0             # channel 1, frame 70
    H[17, 64] = np.nan           # channel 0, frame 64 (first frame of the second tile)
    H[K - 1, T + 99] = np.nan    # channel 1, last frame, last atom
    if form == 'one-hot':
        ref = R.ratio_one_hot(W, H, am, S, X)
        sp = device_ratio(lib, W, H, X, S, argmax=am)
        bound = 2 * K + 5
    else:
        ref = R.ratio_soft(W, H, masks, X)
        sp = device_ratio(lib, W, H, X, S, masks=masks)
        bound = 3 * K + 5
    assert (sp[:, 0, :, 5] == 0).all() and (sp[:, 1, :, 70] == 0).all()
    assert np.isnan(sp[:, 0, :, 64]).all() and np.isnan(sp[:, 1, :, 99]).all()
    special = np.zeros((2, T), bool)
    special[0, [5, 64]] = special[1, [70, 99]] = True
    ok = ~special
    assert np.isfinite(sp[:, ok[:, None, :].repeat(F, 1)]).all()
    err = np.where(ok[None, :, None, :], sp - ref, 0)
    assert worst(err, X, bound) <= 1


# ---- the engine ------------------------------------------------------------------------------------------------------------------

def engine(n, **kw):
    from gcc_nmf_amd.engine import GCCNMFEngine
    return GCCNMFEngine(n, **kw)


def state(e):
    W, H = e.get_WH()
    return dict(idx=e.get_tdoa_indexes(), W=W, H=H, argmax=e.get_argmax(), X=e.get_X(), spec=e.get_spec())


def waveforms(spec, hop=256, ws=1024):
    """(..., F, T) complex -> float64 waveforms through the CPU oracle's inverse STFT, with the gain of getTargetSignalEstimates"""
    flat = spec.reshape((-1,) + spec.shape[-2:])
    y = np.array([O.istft(s.astype(np.complex64), hop, ws, np.hanning) for s in flat]).astype(np.float64) * (hop / float(ws) * 2)
    return y.reshape(spec.shape[:-2] + (-1,))


def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def test_engine_end_to_end_both_modes(lib, dev1):
    """Check 8: dev1, K = 128, hop 256.  The mode changes only the last two stages."""
    x, sr = dev1
    kw = dict(sampleRate=sr, dictionarySize=128, numIterations=100)
    e0 = engine(x.shape[1], **kw)
    y0 = e0.separate(x)[0]
    s0 = state(e0)
    ed = engine(x.shape[1], reconstruction='direct', **kw)
    yd = ed.separate(x)[0]
    sd = state(ed)
    er = engine(x.shape[1], reconstruction='ratio', **kw)
    yr = er.separate(x)[0]
    sr_ = state(er)
    for k in ('idx', 'W', 'H', 'argmax', 'X'):
        assert np.array_equal(sd[k], s0[k]) and np.array_equal(sr_[k], s0[k]), k
    assert np.array_equal(sd['spec'], s0['spec']) and np.array_equal(yd, y0), 'the direct mode is what an engine without the keyword does'
    assert er.ws_rec is None, 'no masked-H workspace in ratio mode'
    W, H, am, X = sr_['W'][0], sr_['H'][0], sr_['argmax'][0], sr_['X'][0]
    den = R.denominators(W, H, argmax=am, S=3)
    assert (den > 0).all(), den.min()
    ref = R.ratio_one_hot(W, H, am, 3, X)
    w4 = worst(sr_['spec'][0] - ref, X, 2 * 128 + 5)
    r_y = rms(yr - waveforms(ref))
    r_sum = rms(yr.astype(np.float64).sum(axis=0) - waveforms(X))
    print('engine ratio mode on dev1: spec %.3g of the bound, waveform rms vs restatement %.3g, sum of targets vs mixture rms %.3g'
          % (w4, r_y, r_sum))
    assert w4 <= 1
    assert r_y < 1e-4
    assert r_sum < 1e-4


def test_batch_independence(lib, dev1):
    """Check 9: file 0's ratio spec alone == in a batch of 5 == in a ragged batch, bit for bit.  KL-NMF picks its GEMM tile by launch size
    and a file's factors are bit for bit the same across batch sizes when both runs use the same tile (tests/test_gpu_pipeline.py), so the
    three runs are made under tuning key 2 = 1, as there; the ratio kernel itself has one tile shape."""
    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_batch
    x, sr = dev1
    n = x.shape[1]
    assert n == 160000
    kw = dict(sampleRate=sr, dictionarySize=128, numIterations=30, reconstruction='ratio')
    others = synthetic_batch(3, 4, numSamples=n)
    assert lib.gccnmf_set_tuning(2, 1) == 0
    try:
        e1 = engine(n, **kw)
        e1.separate(x)
        alone = e1.get_spec()[0]
        e5 = engine(n, batch=5, **kw)
        e5.separate(np.concatenate([x[None], others]))
        in_five = e5.get_spec()[0]
        assert np.array_equal(e5.get_WH()[1][0], e1.get_WH()[1][0]), 'the factors themselves differ: nothing to compare downstream'
        rg = GCCNMFEngine(lengths=[160000, 80000, 160000], **kw)
        rg.separate([x, others[0][:, :80000], others[1]])
        sub, k = rg.file(0)
        assert sub.reconstruction == 'ratio'
        in_ragged = sub.get_spec()[k]
    finally:
        lib.gccnmf_set_tuning(2, 0)
    assert np.array_equal(in_five, alone, equal_nan=True)
    assert np.array_equal(in_ragged, alone, equal_nan=True)


def test_reconstruct_stage_does_not_depend_on_the_batch(lib):
    """The same file's operands at positions 0 and 3 of a batch of 5 and alone, through the C ABI: the same bits, one-hot and soft."""
    from gcc_nmf_amd.engine import Geometry
    F, T, K, S, B = 513, 150, 128, 3, 5
    g = Geometry(F, T, K)
    files = [synthetic(F, T, K, S, 300 + b) for b in range(B)]
    files[3] = files[0]
    d = lambda a: torch.from_numpy(a).cuda()

    def images(sel):
        n = len(sel)
        Wp, Hp = np.zeros((n, g.Fp, g.Kp), np.float32), np.zeros((n, g.Kp, g.Np), np.float32)
        Ap, Mp = np.zeros((n, g.Kp, g.Tp), np.uint8), np.zeros((n, S, g.Kp, g.Tp), np.float32)
        Xp = np.zeros((n, 2, g.Fp, g.Tp, 2), np.float32)
        for j, b in enumerate(sel):
            W, H, am, masks, X = files[b]
            Wp[j, :F, :K], Hp[j, :K, :2 * T], Ap[j, :K, :T], Mp[j, :, :K, :T] = W, H, am, masks
            Xp[j, :, :F, :T, 0], Xp[j, :, :F, :T, 1] = X.real, X.imag
        return d(Wp), d(Hp), d(Ap), d(Mp), d(Xp)

    def run(sel, soft):
        W, H, A, M, X = images(sel)
        spec = torch.full((len(sel), 2 * S, g.Fp, g.Tp, 2), float('nan'), dtype=torch.float32, device='cuda')
        assert lib.gccnmf_reconstruct(W.data_ptr(), H.data_ptr(), 0 if soft else A.data_ptr(), M.data_ptr() if soft else 0, X.data_ptr(), 0,
                                      F, T, K, S | RATIO, len(sel), 0, spec.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        return spec.cpu().numpy()

    for soft in (False, True):
        alone = run([0], soft)
        five = run(list(range(B)), soft)
        assert np.isfinite(five).all()
        assert np.array_equal(five[0], alone[0]) and np.array_equal(five[3], alone[0]), soft
        assert not np.array_equal(five[1], alone[0])


def test_fixed_dictionary_ratio(dev1):
    """Check 9, second half: a pre-trained dictionary with the ratio mode; the targets add up to the mixture."""
    x, sr = dev1
    e = engine(x.shape[1], sampleRate=sr, dictionarySize=128, numIterations=100)
    e.separate(x)
    W = e.get_WH()[0][0]
    ef = engine(x.shape[1], sampleRate=sr, numIterations=100, dictionaryW=W, reconstruction='ratio')
    ef.separate(x)
    Wf, Hf = ef.get_WH()
    assert np.array_equal(Wf[0], W)
    X, spec, am = ef.get_X()[0], ef.get_spec()[0], ef.get_argmax()[0]
    assert (R.denominators(W, Hf[0], argmax=am, S=3) > 0).all()
    w5 = worst(spec.astype(np.complex128).sum(axis=0)[None] - X[None], X, 3 * 3 + 2)
    print('fixed dictionary, ratio mode: partition %.3g of the bound' % w5)
    assert w5 <= 1
    assert worst(spec - R.ratio_one_hot(W, Hf[0], am, 3, X), X, 2 * 128 + 5) <= 1


def test_dropin_function(dev1):
    """Check 10: getTargetSpectrogramEstimates(..., reconstruction='ratio') takes the remembered arg-max image (one-hot form) for masks
    that came from getTargetCoefficientMasks, and the soft form for any other mask array."""
    from gcc_nmf_amd import gccNMFFunctions as G
    x, sr = dev1
    e = engine(x.shape[1], sampleRate=sr, dictionarySize=128, numIterations=100, reconstruction='ratio')
    e.separate(x)
    W, H = e.get_WH()
    W, H, X, scores, spec = W[0], H[0], e.get_X()[0], e.get_scores()[0], e.get_spec()[0]
    stereoH = np.array(np.hsplit(H, 2))
    masks = G.getTargetCoefficientMasks(scores, 3)
    assert np.array_equal(np.argmax(masks, 0), e.get_argmax()[0])
    est = G.getTargetSpectrogramEstimates(masks, X, W, stereoH, reconstruction='ratio')
    assert est.shape == spec.shape
    w = worst(est - spec, X, 2 * 128 + 5)
    print('drop-in one-hot vs engine: %.3g of the bound' % w)
    assert w <= 1
    soft = (0.9 * masks + 0.05).astype(np.float32)
    est_soft = G.getTargetSpectrogramEstimates(soft, X, W, stereoH, reconstruction='ratio')
    ws = worst(est_soft - R.ratio_soft(W, H, soft, X), X, 3 * 128 + 5)
    print('drop-in soft vs restatement: %.3g of the bound' % ws)
    assert ws <= 1
    # positional use is the reference's signature and the direct mode
    direct = G.getTargetSpectrogramEstimates(masks, X, W, stereoH)
    ref = O.getTargetSpectrogramEstimates(masks.astype(np.float32), X, W, stereoH)
    assert np.abs(direct - ref).max() < 1e-4 * np.abs(ref).max()
