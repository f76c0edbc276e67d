"""-m gpu: GCCNMFArrayEngine(reconstruction='spatial') (gcc_nmf_amd/array.py).

M = 2 is the stereo engine: with pairTDOAs = the stereo TDOA grid, spec, the covariances and the waveforms hold the bits of
GCCNMFEngine(reconstruction='spatial', nmf_groups=1) (the recipe of tests/test_gpu_array_engine.py, including its replacement of the
stereo engine's CC by gccnmf_coherence of its own X).

M = 3, 4 on the line LINE and M = 8 on the eight-microphone line of tests/stacked_pairs.py, on the small shapes of that file's
run_stages: the spatial stage by array_spatial_checks.check_cell on the device's OWN ratio estimates (gccnmf_array_reconstruct on the
engine's W, H, arg-max and X reproduces them) -- bit for bit the float32 restatement, within bar_filter_M of float64 -- and the
waveforms against the float64 inverse STFT of the device's spec at the bar of array_restatement.istft.

check_cell holds every live frame to two float64 checks: bar_filter_M per element where every pivot's guard holds, and
array_spatial_checks.normwise_filter -- a bound from the backward error of the solve and the condition of Sigma_w, with the residual
of the sum of the targets -- wherever its eta is below 1/2, whatever the guards say.  At (8, 2, 3) Sigma_w is well conditioned (pivots
>= 5e-4 against a perturbation near 4e-6), but the running bound of bar_filter_M grows by 1 / d_k at each of the five small pivots
three talkers leave at eight microphones, and its guard fails in about 70 % of the elements (197464 of 280576): a weakness of that
bar, not of the problem; the normwise bar holds all of them.  Asserted in all three cases: at most 0.1 % of the non-zero elements
without any float64 check.

reconstruction='ratio' gives buffers bit-equal to an engine built without the keyword; 'direct' raises."""
import numpy as np
import pytest

import array_restatement as A
import array_spatial_checks as C
import array_spatial_restatement as AS
import stacked_pairs as SP

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

LINE = np.array([[0.0, 0, 0], [0.2, 0, 0], [0.5, 0, 0], [1.0, 0, 0]])
SOUND = 340.29


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
    e = GCCNMFEngine(n, numTDOAs=128, reconstruction='spatial', nmf_groups=1, **kw)
    e.upload(xs)
    e.stft()
    e.klnmf()
    _hip.coherence(e.X, e.g.F, e.g.T, B, e.CC)
    e.localize()
    e.masks()
    e.reconstruct()
    e.istft()
    e.check_status()
    assert not e.status.cpu().numpy().any(), 'the inputs are chosen so that the stereo engine finds its peaks'
    a = GCCNMFArrayEngine(n, numChannels=2, pairTDOAs=e.tdoasInSeconds[None], reconstruction='spatial', **kw)
    y = a.separate(xs)
    F, Fp = a.F, a.Fp
    for name, mine, theirs in (('arg-max', a.argmax, e.argmax), ('spec', a.spec, e.spec), ('waveforms', a._y, e.y.view(B, 4, -1)),
                               ('cov', a.cov[:, :, :F], e.ws_cov[:B * 2 * Fp * 4].view(B, 2, Fp, 4)[:, :, :F])):
        assert same_bits(mine, theirs), name
    assert y.shape == (B, 2, 2, a.L) and np.array_equal(y, e.y.cpu().numpy())
    assert np.isfinite(y).all() and np.abs(y).max() > 0
    R = a.get_cov()
    rows = a.cov[:, :, :F].cpu().numpy()
    assert R.shape == (B, 2, F, 2, 2) and R.dtype == np.complex64
    assert np.array_equal(R[..., 0, 0], rows[..., 0]) and np.array_equal(R[..., 1, 1], rows[..., 1])
    assert np.array_equal(R[..., 0, 1], rows[..., 2] + 1j * rows[..., 3]) and np.array_equal(R[..., 1, 0], np.conj(R[..., 0, 1]))
    # the ratio engine on the same input differs: the filter did something
    r = GCCNMFArrayEngine(n, numChannels=2, pairTDOAs=e.tdoasInSeconds[None], **kw)
    r.separate(xs)
    assert same_bits(r.argmax, a.argmax) and not same_bits(r.spec, a.spec)


def mixtures(M, B, S, seed, line, n):
    from gcc_nmf_amd.synthetic import array_mixture
    return np.stack([array_mixture(seed + b, line[:M], [40, 90, 130][:max(S, 2)], n, 16000) for b in range(B)])


CASES = [((3, 1, 3), 31, LINE), ((4, 2, 3), 42, LINE), ((8, 2, 3), SP.ENGINE_CASES[(8, 2, 3)], SP.LINE8)]


@pytest.mark.parametrize('case,seed,line', CASES, ids=['M%d-b%d-S%d' % c[0] for c in CASES])
def test_the_spatial_stage_and_the_waveforms_against_float64(case, seed, line):
    from gcc_nmf_amd import _array
    from gcc_nmf_amd.array import GCCNMFArrayEngine, azimuthDirections
    M, B, S = case
    n, n_fft, hop, Kk, D = 4096, 256, 64, 32, 61
    xs = mixtures(M, B, S, seed, line, n)
    e = GCCNMFArrayEngine(n, numChannels=M, microphonePositions=line[:M], directions=azimuthDirections(D), speedOfSound=SOUND,
                          windowSize=n_fft, hopSize=hop, numTargets=S, dictionarySize=Kk, numIterations=5, batch=B, reconstruction='spatial')
    y = e.separate(xs)
    F, T = e.F, e.T
    assert not e.status.cpu().numpy().any(), 'the mixtures are those of tests/test_gpu_array_engine.py: every file has its peaks'
    assert e.cov.shape == (B, S, e.Fp, M * M) and e.nsig_pitch == S * M + (S * M) % 2
    # the state the spatial stage started from: the ratio stage again, on the same operands
    Et = torch.zeros_like(e.spec)
    _array.reconstruct(e.W, e.H, e.argmax, None, e.X, M, F, T, Kk, S, B, e.nsig_pitch, Et)
    torch.cuda.synchronize()
    E = torch.view_as_complex(Et)[:, :S * M, :F, :T].reshape(B, S, M, F, T).cpu().numpy()
    X, spec, cov, R = e.get_X(), e.get_spec(), e.cov[:, :, :F].cpu().numpy(), e.get_cov()
    assert R.shape == (B, S, F, M, M) and np.array_equal(R, AS.hermitian(cov, M)) and np.array_equal(R, np.conj(np.swapaxes(R, -1, -2)))
    w = np.hanning(n_fft).astype(np.float32)
    behind = total = unchecked = 0
    for b in range(B):
        what = 'M=%d batch=%d S=%d file %d' % (M, B, S, b)
        fail, bits, share, (cnt, g, un) = C.check_cell(E[b], X[b], cov[b], spec[b], what)
        print('%s: largest share of a bar: %s; %d of %d elements behind a failed guard' %
              (what, ', '.join('%s %.4f' % kv for kv in sorted(share.items())), g, cnt))
        assert not fail, fail
        assert not bits, bits
        behind, total, unchecked = behind + g, total + cnt, unchecked + un
        slots = torch.view_as_complex(e.spec)[b, :, :F, :T].cpu().numpy()
        ref_y, bar = A.istft(slots, w, n_fft, hop, hop / float(n_fft) * 2)
        got_y = e._y[b].cpu().numpy()
        err = np.abs(got_y - ref_y)
        print('%s waveforms: worst share of the bar %.4f' % (what, (err / np.maximum(bar, 1e-300)).max()))
        assert (err <= bar).all(), what
        assert np.array_equal(got_y[:S * M].reshape(S, M, -1), y[b])
        if e.nsig_pitch > S * M:
            assert not slots[S * M:].any(), 'the spare spectrogram slot stays zero'
    print('M=%d: %d of %d elements behind a failed pivot guard, %d without any float64 check' % (M, behind, total, unchecked))
    assert unchecked <= C.GUARD_CAP * total
    assert np.isfinite(y).all() and np.abs(y).max() > 0


def test_ratio_is_the_engine_without_the_keyword():
    from gcc_nmf_amd.array import GCCNMFArrayEngine, azimuthDirections
    M, B, S, n = 4, 2, 3, 4096
    xs = mixtures(M, B, S, 42, LINE, n)
    kw = dict(numChannels=M, microphonePositions=LINE, directions=azimuthDirections(61), speedOfSound=SOUND, windowSize=256, hopSize=64,
              numTargets=S, dictionarySize=32, numIterations=5, batch=B)
    plain = GCCNMFArrayEngine(n, **kw)
    ratio = GCCNMFArrayEngine(n, reconstruction='ratio', **kw)
    y0, y1 = plain.separate(xs), ratio.separate(xs)
    assert plain.reconstruction == 'ratio' and ratio.cov is None and plain.cov is None
    for name in ('X', 'V', 'CC', 'W', 'H', 'ang', 'tdoa_idx', 'scores', 'argmax', 'spec', '_y'):
        assert same_bits(getattr(plain, name), getattr(ratio, name)), name
    assert np.array_equal(y0, y1)
    with pytest.raises(ValueError):
        ratio.get_cov()


def test_direct_raises():
    from gcc_nmf_amd.array import GCCNMFArrayEngine, azimuthDirections
    for bad in ('direct', 'spatial_em', None):
        with pytest.raises(ValueError):
            GCCNMFArrayEngine(4096, numChannels=4, microphonePositions=LINE, directions=azimuthDirections(61), windowSize=256, hopSize=64,
                              reconstruction=bad)
