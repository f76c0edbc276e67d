"""-m gpu: GCC-NONLIN localisation offline (csrc/angular_nl.hip behind gccnmf_angular_spectrogram's packed alpha, the engines and the
named functions) against the float64 NumPy restatement in tests/angular_nl_restatement.py.

The bar.  It is not a constant: for every input the same formulas are evaluated in float32 NumPy (tables rounded to float32 once, as
the package does) and the bar is BAR_FACTOR = 4 x that evaluation's largest distance from float64, the factor covering a different
summation order and the device's v_sqrt_f32 / v_exp_f32 / v_rcp_f32 (each within 1 ulp).  Measured on the six committed mixtures
(alpha = 2, values between 35 and 264): float32 error 7.6e-4 .. 1.0e-3 on A, so a bar of 3.0e-3 .. 4.1e-3 -- the scale of the existing
PHAT bar (1e-3 absolute on +-360) -- and 1.2e-5 .. 1.6e-5 on the time mean, a bar of 4.8e-5 .. 6.4e-5 against a narrowest peak margin
of 3.5e-3 (dev_D).  Each test prints its figures before it asserts."""
import numpy as np
import pytest

import angular_nl_restatement as NL
from oracle import gccnmf_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ERR_ARG = 1
CANARY = 12345.0


@pytest.fixture(scope='module')
def lib():
    from gcc_nmf_amd import _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def device_nl(lib, Cs, freqs, tdoas, alpha, canary=True):
    """gccnmf_angular_spectrogram with GCC-NONLIN on a batch of (F, T) complex64 coherences -> (ang image [B][Dp][Tp], mean [B][Dp]).
    ang is zero-filled (the padding must stay zero) with a canary behind the buffer."""
    from gcc_nmf_amd import _hip
    from gcc_nmf_amd.engine import Geometry, steering_tables
    B, (F, T), D = len(Cs), Cs[0].shape, len(tdoas)
    g = Geometry(F, T, 1, D)
    CC = np.zeros((B, 2, g.Fp, g.Tp), np.float32)
    for b, C in enumerate(Cs):
        CC[b, 0, :F, :T], CC[b, 1, :F, :T] = C.real, C.imag
    dCC = torch.from_numpy(CC).cuda()
    trig = torch.from_numpy(steering_tables(freqs, tdoas, g.Fp, g.Dp)).cuda()
    n = B * g.Dp * g.Tp
    buf = torch.zeros(n + 64, dtype=torch.float32, device='cuda')
    buf[n:] = CANARY
    mean = torch.full((B * g.Dp + 8,), CANARY, dtype=torch.float64, device='cuda')
    Dw, Bw = _hip.angular_nl_words(D, B, alpha)
    assert lib.gccnmf_angular_spectrogram(dCC.data_ptr(), trig.data_ptr(), F, T, Dw, Bw, buf.data_ptr(), mean.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    out, m = buf.cpu().numpy(), mean.cpu().numpy()
    assert np.all(out[n:] == CANARY) and np.all(m[B * g.Dp:] == CANARY), 'wrote past the buffer'
    ang = out[:n].reshape(B, g.Dp, g.Tp)
    assert not ang[:, D:].any() and not ang[:, :, T:].any(), 'padding rows / columns of ang must stay zero'
    return ang, m[:B * g.Dp].reshape(B, g.Dp)


def random_coherence(F, T, seed):
    """Unit-modulus coherence with a few zero-magnitude bins (offline convention: 0) and a few bins that match a grid delay exactly."""
    rng = np.random.RandomState(seed)
    C = np.exp(1j * rng.uniform(-np.pi, np.pi, (F, T)))
    C[rng.rand(F, T) < 0.02] = 0
    return C.astype(np.complex64)


def check_against_restatement(ang, mean, b, C, freqs, tdoas, alpha, what):
    D, (F, T) = len(tdoas), C.shape
    barA, barM, A64, eA, eM = NL.measured_bar(C, freqs, tdoas, alpha)
    dA = float(np.abs(ang[b, :D, :T].astype(np.float64) - A64).max())
    dM = float(np.abs(mean[b, :D] - A64.mean(axis=-1)).max())
    print('%s: A in [%.2f, %.2f]; float32 NumPy error %.3g -> bar %.3g, device %.3g; mean: error %.3g -> bar %.3g, device %.3g'
          % (what, A64.min(), A64.max(), eA, barA, dA, eM, barM, dM))
    assert barA > 0 and dA <= barA, (what, dA, barA)
    assert dM <= barM, (what, dM, barM)
    # the mean is the float64 mean of the device's own float32 values
    assert np.abs(mean[b, :D] - ang[b, :D, :T].astype(np.float64).mean(axis=-1)).max() < 1e-9 * F
    return A64


@pytest.mark.parametrize('name', list(NL.MIXTURES))
def test_six_mixtures_spectrogram_mean_and_indexes(lib, name):
    """Checks 1 and 2 on the committed mixtures: A within the measured bar, the time mean within its bar, the TDOA indexes EXACTLY the
    restatement's (and the issue's lists)."""
    S, want, _ = NL.MIXTURES[name]
    C, freqs, sr = NL.mixture_coherence(name)
    tdoas = O.getTDOAsInSeconds(1.0, 128)
    ang, mean = device_nl(lib, [C], freqs, tdoas, 2.0)
    A64 = check_against_restatement(ang, mean, 0, C, freqs, tdoas, 2.0, name)
    assert NL.pick_peaks(A64.mean(axis=-1), S) == want
    dm = torch.from_numpy(mean[0].copy()).cuda()
    idx = torch.full((S,), -7, dtype=torch.int32, device='cuda')
    st = torch.full((1,), -7, dtype=torch.int32, device='cuda')
    assert lib.gccnmf_pick_tdoa_peaks(dm.data_ptr(), 128, 128, S, 1, idx.data_ptr(), st.data_ptr(), stream()) == 0
    assert int(st.cpu()[0]) == 0 and idx.cpu().numpy().tolist() == want


# shapes off the 1024 path: n_fft 256 and 512; D in {3, 64, 128, 200}; T in {1, 63, 64, 65, 622}; batch 1, 3 and 64; alpha in {0.5, 2, 8}
SHAPES = [
    # F, D, T, batch, alpha
    (129, 3, 1, 1, 2.0), (129, 64, 63, 3, 0.5), (129, 128, 64, 1, 8.0), (129, 200, 65, 3, 2.0), (129, 128, 622, 1, 0.5),
    (257, 3, 65, 3, 8.0), (257, 64, 1, 64, 2.0), (257, 128, 63, 1, 2.0), (257, 200, 64, 1, 0.5), (257, 64, 622, 3, 8.0),
    (257, 128, 65, 64, 2.0), (129, 200, 63, 64, 8.0), (513, 128, 622, 1, 8.0), (513, 128, 622, 3, 0.5),
]


@pytest.mark.parametrize('F,D,T,batch,alpha', SHAPES, ids=['F%d-D%d-T%d-b%d-a%g' % s for s in SHAPES])
def test_shapes_off_the_1024_path(lib, F, D, T, batch, alpha):
    freqs, tdoas = O.getFrequenciesInHz(16000, F), O.getTDOAsInSeconds(1.0, D)
    Cs = [random_coherence(F, T, 7919 * F + 31 * D + T + b) for b in range(batch)]
    # an exact grid delay in one frame of the first file: re = 1 at that tau for every f
    Cs[0][:, T // 2] = np.exp(2j * np.pi * freqs * tdoas[D // 2]).astype(np.complex64)
    ang, mean = device_nl(lib, Cs, freqs, tdoas, alpha)
    for b in sorted({0, batch // 2, batch - 1}):
        A64 = check_against_restatement(ang, mean, b, Cs[b], freqs, tdoas, alpha, 'file %d of %d' % (b, batch))
        assert np.all(ang[b, :D, :T] >= 0) and np.all(ang[b, :D, :T] <= F + 1e-3)
    # at the matched delay 1 - re <= 4 * 2^-24 per bin (two rounded table entries, two rounded parts of C), so 1 - phi <= alpha sqrt(.)
    assert abs(float(ang[0, D // 2, T // 2]) - F) <= F * alpha * 5e-4


def test_a_file_alone_and_in_a_batch_agree_bit_for_bit(lib):
    """Check 3: one file alone takes the 2 x 2 block, the batch of 5 the 4 x 4 block at this shape; every output is summed in the same
    order either way."""
    F, D, T = 513, 128, 622
    freqs, tdoas = O.getFrequenciesInHz(16000, F), O.getTDOAsInSeconds(1.0, D)
    file = random_coherence(F, T, 1)
    batch = [file] + [random_coherence(F, T, 10 + b) for b in range(3)] + [file]
    alone, mean1 = device_nl(lib, [file], freqs, tdoas, 2.0)
    five, mean5 = device_nl(lib, batch, freqs, tdoas, 2.0)
    for pos in (0, 4):
        assert np.array_equal(five[pos], alone[0]) and np.array_equal(mean5[pos, :D], mean1[0, :D]), pos
    assert not np.array_equal(five[1], alone[0])
    # ... and the small shapes, where both launches take the same block
    F, D, T = 129, 64, 65
    freqs, tdoas = O.getFrequenciesInHz(16000, F), O.getTDOAsInSeconds(1.0, D)
    file = random_coherence(F, T, 2)
    alone, _ = device_nl(lib, [file], freqs, tdoas, 0.5)
    five, _ = device_nl(lib, [file] + [random_coherence(F, T, 20 + b) for b in range(3)] + [file], freqs, tdoas, 0.5)
    assert np.array_equal(five[0], alone[0]) and np.array_equal(five[4], alone[0])


def test_argument_errors_and_phat_unchanged(lib):
    """alpha bits that are not a positive normal float are GCCNMF_ERR_ARG with real device pointers too; both halves zero is PHAT."""
    from gcc_nmf_amd import _hip
    from gcc_nmf_amd.engine import Geometry, steering_tables
    F, D, T = 129, 64, 10
    g = Geometry(F, T, 1, D)
    freqs, tdoas = O.getFrequenciesInHz(16000, F), O.getTDOAsInSeconds(1.0, D)
    C = random_coherence(F, T, 3)
    CC = np.zeros((1, 2, g.Fp, g.Tp), np.float32)
    CC[0, 0, :F, :T], CC[0, 1, :F, :T] = C.real, C.imag
    dCC, trig = torch.from_numpy(CC).cuda(), torch.from_numpy(steering_tables(freqs, tdoas, g.Fp, g.Dp)).cuda()
    ang = torch.zeros((1, g.Dp, g.Tp), dtype=torch.float32, device='cuda')
    for Dw, Bw in ((D | (0xbf80 << 16) - (1 << 32), 1), (D | (0x7f80 << 16), 1), (D | (0x7fc0 << 16), 1), (D, 1 | (1 << 16))):
        assert lib.gccnmf_angular_spectrogram(dCC.data_ptr(), trig.data_ptr(), F, T, Dw, Bw, ang.data_ptr(), 0, stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert not ang.cpu().numpy().any()
    assert lib.gccnmf_angular_spectrogram(dCC.data_ptr(), trig.data_ptr(), F, T, D, 1, ang.data_ptr(), 0, stream()) == 0
    torch.cuda.synchronize()
    phat = O.getAngularSpectrogram(C.astype(np.complex128), freqs, 1.0, D)
    assert np.abs(ang.cpu().numpy()[0, :D, :T] - phat).max() < 1e-3


def test_engine_indexes_and_waveforms(dev1):
    """Check 4: NL on dev1 finds [47, 72, 107] and returns the default engine's waveforms bit for bit (only localisation differs and the
    indexes coincide); on dev_Sq1_Co_A it finds [60, 64, 68] where the default finds [60, 63, 68]; a ragged engine with NL on gives each
    file the indexes of an equal-length batch."""
    from gcc_nmf_amd.engine import GCCNMFEngine
    x, sr = dev1
    kw = dict(sampleRate=sr, dictionarySize=64, numIterations=10)
    e0, e1 = GCCNMFEngine(x.shape[1], **kw), GCCNMFEngine(x.shape[1], gccPHATNLEnabled=True, **kw)
    assert (e1.gccPHATNLEnabled, e1.gccPHATNLAlpha, e0.gccPHATNLEnabled) == (True, 2.0, False)
    y0, y1 = e0.separate(x[None]), e1.separate(x[None])
    assert e0.get_tdoa_indexes()[0].tolist() == [47, 72, 107] == e1.get_tdoa_indexes()[0].tolist()
    assert np.array_equal(y0, y1)
    assert not np.array_equal(e0.get_angular()[0], e1.get_angular()[0])
    xs, sr = NL.load_mixture('dev_Sq1_Co_A')
    s0, s1 = GCCNMFEngine(xs.shape[1], **kw), GCCNMFEngine(xs.shape[1], gccPHATNLEnabled=True, gccPHATNLAlpha=2.0, **kw)
    s0.separate(xs[None])
    s1.separate(xs[None])
    assert s0.get_tdoa_indexes()[0].tolist() == [60, 63, 68] and s1.get_tdoa_indexes()[0].tolist() == [60, 64, 68]
    # ragged: two lengths, two files each; every file as in the equal-length batch of its length
    n_a, n_b = 60000, 48000
    files = [x[:, :n_a], xs[:, :n_b], xs[:, 20000:20000 + n_a], x[:, 30000:30000 + n_b]]
    r = GCCNMFEngine(lengths=[f.shape[1] for f in files], gccPHATNLEnabled=True, gccPHATNLAlpha=2.0, **kw)
    assert all(sub.gccPHATNLEnabled and sub.gccPHATNLAlpha == 2.0 for sub in r.sub.values())
    r.separate(files)
    for n, members in ((n_a, [0, 2]), (n_b, [1, 3])):
        eq = GCCNMFEngine(n, batch=2, gccPHATNLEnabled=True, **kw)
        eq.separate(np.stack([files[i] for i in members]))
        sub = r.sub[n]
        assert np.array_equal(sub.get_tdoa_indexes(), eq.get_tdoa_indexes()), n
        assert np.array_equal(sub.get_angular()[0], eq.get_angular()[0]), n


def test_named_functions(lib):
    """Check 5: getAngularSpectrogram(..., gccPHATNLEnabled=True) is float64 (D, T) within the bar of check 1; getTargetTDOAEstimates
    with NL returns the restatement's indexes."""
    from gcc_nmf_amd import gccNMFFunctions as G
    name = 'dev_Sq1_Co_A'
    S, want, phat = NL.MIXTURES[name]
    x, sr = NL.load_mixture(name)
    X = O.computeComplexMixtureSpectrogram(x, 1024, 256, np.hanning).astype(np.complex64)
    C = NL.offline_coherence(X).astype(np.complex64)
    freqs, tdoas = O.getFrequenciesInHz(sr, 513), O.getTDOAsInSeconds(1.0, 128)
    A = G.getAngularSpectrogram(C, freqs, 1.0, 128, gccPHATNLEnabled=True, gccPHATNLAlpha=2.0)
    barA, barM, A64, eA, eM = NL.measured_bar(C, freqs, tdoas, 2.0)
    d = float(np.abs(A - A64).max())
    print('getAngularSpectrogram NL: float32 NumPy error %.3g -> bar %.3g, device %.3g' % (eA, barA, d))
    assert A.dtype == np.float64 and A.shape == (128, C.shape[1]) and d <= barA
    assert np.array_equal(G.getAngularSpectrogram(C, freqs, 1.0, 128), G.getAngularSpectrogram(C, freqs, 1.0, 128, False, 2.0))
    idx, meanA = G.getTargetTDOAEstimates(X, sr, 1.0, 128, S, gccPHATNLEnabled=True)
    assert [int(i) for i in idx] == want == NL.pick_peaks(A64.mean(axis=-1), S)
    assert [int(i) for i in G.getTargetTDOAEstimates(X, sr, 1.0, 128, S)[0]] == phat
    assert meanA.dtype == np.float64 and meanA.shape == (128,)
