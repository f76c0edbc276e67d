"""-m gpu: offline speech enhancement -- the full-grid atom TDOA arg-max and the talker / noise masks (csrc/atom_tdoa.hip, two modes
of gccnmf_target_scores_masks), through the C ABI wrappers of gcc_nmf_amd._hip, against the float64 restatement
tests/atom_tdoa_restatement.py of the SAME float32 inputs; then the engine and the reference-style functions end to end.

Index check, no exclusions: with S64 the float64 scores and Sabs[k, t] = max_d sum_f |W| |G|, the device's index d^ of every (k, t)
must satisfy S64[k, d^, t] >= max_d S64[k, :, t] - 1e-5 Sabs[k, t], and atom_score must lie within the same bound of S64[k, d^, t].
Where the float64 top-two gap reaches the bound this forces equality; elsewhere only a genuine near-tie passes.  1e-5 is 8 x the
1.3e-6 Sabs a float32 evaluation in NumPy's order erred by on the 1024-point synthetic mixture (about sqrt(F) 2^-24).  The kernel's own
error is printed by every case (-s).

Window masks: within 1e-6 absolute of float64 (expf and powf are within a few ulp; the error of p = (dist / eps)^beta enters
m = exp(-p) as m p delta with m p <= 1 / e).  Boxcar masks and the uint8 image are exact."""
import ctypes

import numpy as np
import pytest

import atom_tdoa_restatement as A
import ratio_restatement as R
from oracle import gccnmf_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ERR_ARG, ERR_UNSUPPORTED = 1, 3
BAR = 1e-5
U = 2.0 ** -24


@pytest.fixture(scope='module')
def hip():
    from gcc_nmf_amd import _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    _hip.lib()
    return _hip


def geometry(F, T, K, D):
    from gcc_nmf_amd.engine import Geometry
    return Geometry(F, T, K, D)


def tables(F, D, sampleRate=16000):
    """(cos, sin) (F, D) float32 exactly as the engine builds them."""
    from gcc_nmf_amd.engine import steering_tables
    tdoas = np.linspace(-1.0 / 340.29, 1.0 / 340.29, D)
    trig = steering_tables(np.linspace(0, sampleRate / 2.0, F), tdoas, F, D)
    return trig[0].copy(), trig[1].copy()


def phase_coherence(F, T, seed, sampleRate=16000):
    """unit-modulus coherence of a talker at tau0 plus phase noise, complex64 (F, T)"""
    rng = np.random.default_rng(seed)
    f = np.linspace(0, sampleRate / 2.0, F)[:, None]
    tau0 = 0.4 / 340.29
    ph = -2 * np.pi * f * tau0 + rng.normal(0, 0.8, (F, T))
    return np.exp(1j * ph).astype(np.complex64)


def stft_coherence(n_fft, T, batch):
    """PHAT coherence of synthetic_mixture(0 .. batch - 1) through the library's own STFT: (batch, F, T) complex64"""
    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_mixture
    hop = n_fft // 4
    n = n_fft + hop * (T - 1)
    e = GCCNMFEngine(n, windowSize=n_fft, hopSize=hop, dictionarySize=16, numIterations=1, batch=batch)
    e.upload(np.stack([synthetic_mixture(b, numSamples=n) for b in range(batch)]))
    e.stft()
    assert e.g.T == T
    return e.get_C()


def dictionary(F, K, seed):
    """random non-negative atoms, every second one limited to a band of the spectrum"""
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.01, 1.0, (F, K)).astype(np.float32)
    for k in range(1, K, 2):
        lo = int(rng.integers(0, F - F // 4))
        keep = np.zeros(F, bool)
        keep[lo:lo + max(2, F // 4)] = True
        W[~keep, k] = 0
    return W


def device_atom_tdoa(hip, C, cos, sin, W, D=None, want_score=True):
    """C (B, F, T) complex64, cos / sin (F, D), W (B, F, K) through the wrapper: zero-padded operands, outputs filled with 0xFFFF / NaN.
    -> (index (B, K, T) int64, score (B, K, T) float32 or None); the padding of both must have been written as zeros."""
    B, F, T = C.shape
    K = W.shape[2]
    D = cos.shape[1] if D is None else D
    g = geometry(F, T, K, D)
    CC = np.zeros((B, 2, g.Fp, g.Tp), np.float32)
    CC[:, 0, :F, :T], CC[:, 1, :F, :T] = C.real, C.imag
    trig = np.zeros((2, g.Fp, g.Dp), np.float32)
    trig[0, :F, :cos.shape[1]], trig[1, :F, :cos.shape[1]] = cos, sin
    Wp = np.zeros((B, g.Fp, g.Kp), np.float32)
    Wp[:, :F, :K] = W
    d = lambda a: torch.from_numpy(a).cuda()
    dC, dT, dW = d(CC), d(trig), d(Wp)
    idx = torch.full((B, g.Kp, g.Tp), -1, dtype=torch.int16, device='cuda')
    score = torch.full((B, g.Kp, g.Tp), float('nan'), dtype=torch.float32, device='cuda') if want_score else None
    hip.atom_tdoa_indexes(dC, dT, dW, F, T, K, D, B, idx, score)
    torch.cuda.synchronize()
    i = idx.cpu().numpy().view(np.uint16).astype(np.int64)
    assert (i[:, K:, :] == 0).all() and (i[:, :, T:] == 0).all(), 'index padding must be written as zeros'
    s = None
    if want_score:
        s = score.cpu().numpy()
        assert (s[:, K:, :] == 0).all() and (s[:, :, T:] == 0).all(), 'score padding must be written as zeros'
        s = s[:, :K, :T]
    return i[:, :K, :T], s, idx


def check_indexes(idx, score, C, cos, sin, W, what):
    """the index check of the module docstring on one file; returns the float64 scores"""
    ref, S64, Sabs = A.atom_tdoa(C, cos, sin, W)
    assert idx.min() >= 0 and idx.max() < cos.shape[1], what
    got = np.take_along_axis(S64, idx[:, None, :], axis=1)[:, 0, :]
    short = (S64.max(axis=1) - got) / Sabs
    err = np.abs(score.astype(np.float64) - got) / Sabs
    top2 = np.sort(S64, axis=1)[:, -2:, :]
    near = ((top2[:, 1] - top2[:, 0]) < BAR * Sabs).mean()
    print('%s: chosen score below the float64 maximum by at most %.3g Sabs, atom_score error %.3g Sabs, %d of %d indexes differ from the '
          'float64 arg-max, %.3f %% of positions have a float64 top-two gap below the bar'
          % (what, short.max(), err.max(), int((idx != ref).sum()), idx.size, 100 * near))
    assert short.max() <= BAR, what
    assert err.max() <= BAR, what
    return S64


CASES = [(33, 1, 16, 64, 1), (33, 5, 40, 33, 1), (129, 67, 128, 128, 3), (513, 70, 144, 200, 2), (65, 9, 64, 1024, 1),
         (513, 130, 1024, 128, 1)]

_inputs = {}


def inputs(case):
    """(C, cos, sin, W) of a case, built once"""
    if case not in _inputs:
        F, T, K, D, B = case
        C = stft_coherence(2 * (F - 1), T, B) if F in (129, 513) else np.stack([phase_coherence(F, T, 10 + b) for b in range(B)])
        cos, sin = tables(F, D)
        W = np.stack([dictionary(F, K, 100 + b) for b in range(B)])
        _inputs[case] = (C, cos, sin, W)
    return _inputs[case]


@pytest.mark.parametrize('case', CASES, ids=['x'.join(str(v) for v in c) for c in CASES])
def test_indexes_and_scores(hip, case):
    C, cos, sin, W = inputs(case)
    idx, score, _ = device_atom_tdoa(hip, C, cos, sin, W)
    for b in range(case[4]):
        check_indexes(idx[b], score[b], C[b], cos, sin, W[b], 'F, T, K, D = %s file %d' % (case[:4], b))
    idx2, _, _ = device_atom_tdoa(hip, C, cos, sin, W, want_score=False)
    assert np.array_equal(idx, idx2), 'the index image does not depend on whether the score is asked for'


def test_batch_independence(hip):
    C, cos, sin, W = inputs(CASES[2])
    idx, score, _ = device_atom_tdoa(hip, C, cos, sin, W)
    one_i, one_s, _ = device_atom_tdoa(hip, C[1:2], cos, sin, W[1:2])
    assert np.array_equal(idx[1], one_i[0]) and np.array_equal(score[1], one_s[0])


def test_rules(hip):
    """silent frame -> 0; identical TDOA columns -> the lower index; a NaN coherence entry -> 0 for that frame only"""
    F, T, K, D, _ = CASES[1]
    C, cos, sin, W = inputs(CASES[1])
    base, base_s, _ = device_atom_tdoa(hip, C, cos, sin, W)
    silent = C.copy()
    silent[0, :, 2] = 0
    idx, _, _ = device_atom_tdoa(hip, silent, cos, sin, W)
    assert (idx[0][:, 2] == 0).all() and np.array_equal(np.delete(idx, 2, axis=2), np.delete(base, 2, axis=2))
    # the most frequent winner gets an identical twin at a LOWER index (column 0) and at a HIGHER one (column D - 1)
    win = int(np.bincount(base.ravel()).argmax())
    assert 0 < win < D - 1
    cos2, sin2 = cos.copy(), sin.copy()
    cos2[:, 0], sin2[:, 0], cos2[:, D - 1], sin2[:, D - 1] = cos[:, win], sin[:, win], cos[:, win], sin[:, win]
    twin, _, _ = device_atom_tdoa(hip, C, cos2, sin2, W)
    assert not (twin == win).any() and not (twin == D - 1).any() and (twin == 0).sum() >= (base == win).sum(), \
        'of identical columns the lowest index wins'
    ref = A.atom_tdoa(C[0], cos2, sin2, W[0])[0]
    assert ((twin[0] == 0) == (ref == 0)).mean() > 0.99
    nan = C.copy()
    nan[0, 7, 1] = np.nan
    idx, score, _ = device_atom_tdoa(hip, nan, cos, sin, W)
    assert (idx[0][:, 1] == 0).all() and np.isnan(score[0][:, 1]).all()
    assert np.array_equal(np.delete(idx, 1, axis=2), np.delete(base, 1, axis=2))
    assert np.array_equal(np.delete(score, 1, axis=2), np.delete(base_s, 1, axis=2))


def device_masks(hip, idx_dev, target, T, K, B, window, eps, beta, nf, per_frame):
    g = geometry(2, T, K, 1)
    image = torch.full((B, g.Kp, g.Tp), 77, dtype=torch.uint8, device='cuda')
    masks = torch.full((B, 2, g.Kp, g.Tp), float('nan'), dtype=torch.float32, device='cuda')
    if per_frame:
        tg = torch.full((B, g.Tp), -5, dtype=torch.int32, device='cuda')
        tg[:, :T] = torch.from_numpy(np.asarray(target, np.int32)).cuda()
    else:
        tg = torch.from_numpy(np.asarray(target, np.int32)).cuda()
    hip.enhancement_masks(idx_dev, tg, T, K, B, image, masks, window=window, eps=eps, beta=beta, noise_floor=nf, per_frame=per_frame)
    torch.cuda.synchronize()
    im, m = image.cpu().numpy(), masks.cpu().numpy()
    assert (im[:, K:, :] == 0).all() and (im[:, :, T:] == 0).all() and (m[:, :, K:, :] == 0).all() and (m[:, :, :, T:] == 0).all()
    return im[:, :K, :T], m[:, :, :K, :T]


@pytest.mark.parametrize('window,eps,beta,nf', [(0, 4.0, 2.0, 0.0), (0, 2.5, 1.0, 0.1), (1, 5.0, 2.0, 0.0), (1, 2.0, 1.0, 0.05), (1, 3.0, 2.5, 0.3)])
def test_masks_from_the_device_index_image(hip, window, eps, beta, nf):
    case = CASES[2]
    F, T, K, D, B = case
    C, cos, sin, W = inputs(case)
    idx, _, idx_dev = device_atom_tdoa(hip, C, cos, sin, W, want_score=False)
    target = np.array([60, 61, 3], np.int32)
    im, m = device_masks(hip, idx_dev, target, T, K, B, window, eps, beta, nf, False)
    for b in range(B):
        ref_im, ref_m = A.masks(idx[b], target[b], window, eps, beta, nf)
        assert np.array_equal(im[b], ref_im)
        if window:
            err = np.abs(m[b] - ref_m).max()
            print('window masks eps %g beta %g nf %g file %d: max error %.3g' % (eps, beta, nf, b, err))
            assert err <= 1e-6
        else:
            assert np.array_equal(m[b], ref_m.astype(np.float32))
    assert np.array_equal(m[:, 1], np.float32(1) - m[:, 0]), 'noise = 1 - talker exactly'
    im2, m2 = device_masks(hip, idx_dev, np.repeat(target[:, None], T, axis=1), T, K, B, window, eps, beta, nf, True)
    assert np.array_equal(im2, im) and np.array_equal(m2, m), 'a constant track gives the bits of the per-file target'
    # a moving target: every frame against its own index
    moving = (np.arange(T)[None, :] + target[:, None]) % D
    im3, m3 = device_masks(hip, idx_dev, moving, T, K, B, window, eps, beta, nf, True)
    ref_im, ref_m = A.masks(idx[0], moving[0][None, :], window, eps, beta, nf)
    assert np.array_equal(im3[0], ref_im) and np.abs(m3[0] - ref_m).max() <= 1e-6
    # image only / masks only
    g = geometry(2, T, K, 1)
    only = torch.full((B, g.Kp, g.Tp), 77, dtype=torch.uint8, device='cuda')
    hip.enhancement_masks(idx_dev, torch.from_numpy(target).cuda(), T, K, B, only, None, window=window, eps=eps, beta=beta, noise_floor=nf)
    assert np.array_equal(only.cpu().numpy()[:, :K, :T], im)


def test_error_codes(hip):
    lib = hip.lib()
    F, T, K, D = 33, 5, 40, 33
    g = geometry(F, T, K, 1025)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device='cuda')
    CC, trig, W = z(2, g.Fp, g.Tp), z(2, g.Fp, 1088), z(g.Fp, g.Kp)
    out = torch.full((g.Kp, g.Tp), -1, dtype=torch.int16, device='cuda')
    s = torch.cuda.current_stream().cuda_stream
    call = lambda cc, tr, w, o, Dn=D, Fn=F, Tn=T, Kn=K, Bn=1, word=hip.GCCNMF_SCORES_ATOM_TDOA: lib.gccnmf_target_scores_masks(
        cc, tr, 0, w, Fn, Tn, Kn, Dn, word, Bn, 0, 0, o, s)
    p = lambda t: t.data_ptr()
    assert call(p(CC), p(trig), p(W), p(out), Dn=1025) == ERR_UNSUPPORTED
    for args in ((0, p(trig), p(W), p(out)), (p(CC), 0, p(W), p(out)), (p(CC), p(trig), 0, p(out)), (p(CC), p(trig), p(W), 0)):
        assert call(*args) == ERR_ARG
    for kw in (dict(Dn=0), dict(Fn=1), dict(Tn=0), dict(Kn=0), dict(Bn=0), dict(Kn=-3), dict(word=hip.GCCNMF_SCORES_ATOM_TDOA | 2)):
        assert call(p(CC), p(trig), p(W), p(out), **kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert (out == -1).all(), 'a rejected call launches nothing'
    assert call(p(CC), p(trig), p(W), p(out), Dn=1024) == 0
    torch.cuda.synchronize()
    assert (out == 0).all()
    # the masks mode
    params = (ctypes.c_float * 3)(4.0, 2.0, 0.0)
    tg = torch.zeros((1,), dtype=torch.int32, device='cuda')
    image = torch.full((g.Kp, g.Tp), 77, dtype=torch.uint8, device='cuda')
    word = hip.GCCNMF_SCORES_ENHANCEMENT_MASKS
    mcall = lambda a, pr, t, im, m=0, w=word, Tn=T, Kn=K, Bn=1: lib.gccnmf_target_scores_masks(a, pr, t, 0, 0, Tn, Kn, 0, w, Bn, 0, m, im, s)
    ok = (p(out), ctypes.addressof(params), p(tg), p(image))
    for i in range(4):
        bad = list(ok)
        bad[i] = 0
        assert mcall(*bad) == ERR_ARG, i                          # (both outputs null when i == 3)
    for kw in (dict(w=word | 2), dict(Tn=0), dict(Kn=0), dict(Bn=0)):
        assert mcall(*ok, **kw) == ERR_ARG, kw
    for bad in ((0.0, 2.0, 0.0), (4.0, -1.0, 0.0), (4.0, 2.0, -0.1), (float('nan'), 2.0, 0.0), (4.0, float('inf'), 0.0)):
        held = (ctypes.c_float * 3)(*bad)
        assert mcall(p(out), ctypes.addressof(held), p(tg), p(image)) == ERR_ARG, bad
    torch.cuda.synchronize()
    assert (image == 77).all()
    assert mcall(*ok) == 0


# ---- the engine and the reference-style functions ---------------------------------------------------------------------------------

def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def waveforms(spec, hop, ws):
    flat = spec.reshape((-1,) + spec.shape[-2:])
    y = np.array([O.istft(s.astype(np.complex64), hop, ws, np.hanning) for s in flat]).astype(np.float64) * (hop / float(ws) * 2)
    return y.reshape(spec.shape[:-2] + (-1,))


@pytest.mark.parametrize('mode,reconstruction', [('boxcar', 'direct'), ('boxcar', 'ratio'), ('window', 'ratio')])
def test_engine_end_to_end(hip, mode, reconstruction):
    """n_fft = 256, K = 32, two 1 s files: engine == the chain of reference-style functions bit for bit, both within the bars of
    tests/test_gpu_ratio_reconstruction.py of the float64 restatement fed the device's W, H and index image."""
    from gcc_nmf_amd import gccNMFFunctions as G
    from gcc_nmf_amd.engine import GCCNMFEnhancementEngine
    from gcc_nmf_amd.synthetic import speech_in_noise_mixture
    n, ws, hop, K, D, eps = 16000, 256, 64, 32, 128, 4.0
    xs = np.stack([speech_in_noise_mixture(b, 0.0, numSamples=n)[0] for b in range(2)])
    e = GCCNMFEnhancementEngine(n, windowSize=ws, hopSize=hop, dictionarySize=K, numIterations=30, batch=2, targetMode=mode,
                                targetTDOAEpsilon=eps, reconstruction=reconstruction)
    y = e.separate(xs)
    T, F = e.g.T, e.g.F
    assert y.shape == (2, 2, 2, hop * (T - 1)) and y.dtype == np.float32
    atoms, tdoa, (W, H), Cd, X, spec = e.get_atom_tdoa_indexes(), e.get_tdoa_indexes(), e.get_WH(), e.get_C(), e.get_X(), e.get_spec()
    assert atoms.shape == (2, K, T) and tdoa.shape == (2, 1)
    window = 1 if mode == 'window' else 0
    G.set_resident(reconstruction == 'ratio' and not window)      # the one-hot ratio form needs the image behind the boxcar masks
    try:
        for b in range(2):
            a = G.getAtomTDOAIndexes(Cd[b], 1.0, D, e.frequenciesInHz, W[b])
            assert a.shape == (K, T) and np.array_equal(a, atoms[b])
            m = G.getEnhancementCoefficientMasks(a, int(tdoa[b, 0]), mode, eps)
            assert m.shape == (2, K, T) and m.dtype == np.float32 and np.array_equal(m, e.get_enhancement_masks()[b])
            ref_im, ref_m = A.masks(atoms[b], int(tdoa[b, 0]), window, eps)
            assert np.abs(m - ref_m).max() <= 1e-6
            stereoH = np.array(np.hsplit(H[b], 2))
            S = G.getTargetSpectrogramEstimates(m, X[b], W[b], stereoH, reconstruction=reconstruction)
            assert np.array_equal(S, spec[b])
            yb = G.getTargetSignalEstimates(S, ws, hop, np.hanning)
            assert np.array_equal(yb, y[b])
            if reconstruction == 'ratio':
                ref = R.ratio_soft(W[b], H[b], m, X[b]) if window else R.ratio_one_hot(W[b], H[b], ref_im, 2, X[b])
                bound = (3 * K + 5) if window else (2 * K + 5)
                w = float((np.abs(spec[b] - ref) / (bound * U * np.abs(X[b])[None])).max())
                r_y, r_sum = rms(y[b] - waveforms(ref, hop, ws)), rms(y[b].astype(np.float64).sum(axis=0) - waveforms(X[b], hop, ws))
                print('file %d %s: spec %.3g of the bound, waveform rms %.3g, talker + noise vs mixture rms %.3g' % (b, mode, w, r_y, r_sum))
                assert w <= 1 and r_y < 1e-4 and r_sum < 1e-4
    finally:
        G.set_resident(False)
    if mode == 'boxcar' and reconstruction == 'direct':
        pcm = np.round(xs.transpose(0, 2, 1) * 32768).astype(np.int16)
        out = e.separate_pcm16(pcm)
        assert out.shape == (2, 2, hop * (T - 1), 2) and out.dtype == np.int16
        assert np.array_equal(list(e.separate_batches([xs, xs]))[1], y)
        fixed = GCCNMFEnhancementEngine(n, windowSize=ws, hopSize=hop, dictionarySize=K, numIterations=30, batch=2, targetMode=mode,
                                        targetTDOAEpsilon=eps, targetTDOAIndex=[int(v) for v in tdoa[:, 0]])
        assert np.array_equal(fixed.separate(xs), y), 'a given target index skips the pick and changes nothing else'
        tracked = GCCNMFEnhancementEngine(n, windowSize=ws, hopSize=hop, dictionarySize=K, numIterations=30, batch=2, targetMode=mode,
                                          targetTDOAEpsilon=eps, tdoaTracking=True, localizationWindowSize=2 * T)
        assert np.array_equal(tracked.separate(xs), y), 'a window of the whole file is the static pick'
        assert tracked.get_tdoa_tracks().shape == (2, 1, T)
