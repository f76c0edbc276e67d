"""-m gpu: GCCNMFArrayEngine(reconstruction='spatial', spatialIterations=n) (gcc_nmf_amd/array.py).

spatialIterations=2: separate() leaves in spec, the covariances, the powers and the waveforms the bits of the staged C-ABI calls on the
engine's own operands -- gccnmf_array_reconstruct, gccnmf_array_em (n = 2) and the inverse STFT -- at M = 4 and at M = 8; get_cov()
returns the refined rows.  spatialIterations=0 is the engine without the keyword in every buffer.  M = 2 is the stereo engine with the
same spatialIterations (the recipe of tests/test_gpu_array_spatial_engine.py)."""
import numpy as np
import pytest

import array_spatial_restatement as AS
import stacked_pairs as SP
from test_gpu_array_spatial_engine import LINE, SOUND, mixtures, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

CASES = [((4, 2, 3), 42, LINE), ((8, 2, 3), SP.ENGINE_CASES[(8, 2, 3)], SP.LINE8)]


def engine_kw(M, B, S, line):
    from gcc_nmf_amd.array import azimuthDirections
    return dict(numChannels=M, microphonePositions=line[:M], directions=azimuthDirections(61), speedOfSound=SOUND, windowSize=256, hopSize=64,
                numTargets=S, dictionarySize=32, numIterations=5, batch=B)


@pytest.mark.parametrize('case,seed,line', CASES, ids=['M%d-b%d-S%d' % c[0] for c in CASES])
def test_separate_is_the_staged_calls_bit_for_bit(case, seed, line):
    from gcc_nmf_amd import _array, _array_em
    from gcc_nmf_amd.array import GCCNMFArrayEngine
    M, B, S = case
    n, N_EM = 4096, 2
    xs = mixtures(M, B, S, seed, line, n)
    e = GCCNMFArrayEngine(n, reconstruction='spatial', spatialIterations=N_EM, **engine_kw(M, B, S, line))
    y = e.separate(xs)
    F, T, Fp, Tp = e.F, e.T, e.Fp, e.Tp
    assert e.spatialIterations == N_EM and not e.status.cpu().numpy().any()
    assert e.cov.shape == (B, S, Fp, M * M) and e.powers.shape == (B, S, Fp, Tp)
    assert e.ws_em.numel() == _array_em.workspace_floats(M, F, T, S, B) and e.cov.data_ptr() == e.ws_em.data_ptr(), 'one workspace, allocated once'
    # the staged calls on the engine's own operands
    spec = torch.zeros_like(e.spec)
    _array.reconstruct(e.W, e.H, e.argmax, None, e.X, M, F, T, e.K, S, B, e.nsig_pitch, spec)
    ratio = spec.clone()
    ws = torch.full_like(e.ws_em, -1.0)
    _array_em.em(e.X, M, F, T, S, B, e.nsig_pitch, N_EM, ws, spec)
    torch.cuda.synchronize()
    ncov = B * S * Fp * M * M
    assert same_bits(e.spec, spec), 'spec'
    assert same_bits(e.cov[:, :, :F], ws[:ncov].view(B, S, Fp, M * M)[:, :, :F]), 'cov'
    assert same_bits(e.powers[:, :, :F, :T], ws[ncov:].view(B, S, Fp, Tp)[:, :, :F, :T]), 'the powers'
    assert not same_bits(e.spec, ratio)
    # the refined covariances are what get_cov() returns, and they are not the start's
    R = e.get_cov()
    rows = e.cov[:, :, :F].cpu().numpy()
    assert R.shape == (B, S, F, M, M) and np.array_equal(R, AS.hermitian(rows, M)) and np.array_equal(R, np.conj(np.swapaxes(R, -1, -2)))
    plain = GCCNMFArrayEngine(n, reconstruction='spatial', **engine_kw(M, B, S, line))
    y0 = plain.separate(xs)
    assert same_bits(plain.argmax, e.argmax) and not same_bits(plain.cov[:, :, :F], e.cov[:, :, :F]) and not same_bits(plain.spec, e.spec)
    tr = np.trace(R, axis1=-2, axis2=-1).real
    assert np.isfinite(R).all() and (tr > 0).all() and (np.linalg.eigvalsh(R.astype(np.complex128)) > 0).all(), 'full rank'
    # the waveforms: the engine's inverse STFT of that spec
    e.spec.copy_(spec)
    e.istft()
    torch.cuda.synchronize()
    assert np.array_equal(e.get_y(), y) and np.isfinite(y).all() and np.abs(y).max() > 0 and not np.array_equal(y, y0)


def test_zero_iterations_is_the_engine_without_the_keyword():
    from gcc_nmf_amd.array import GCCNMFArrayEngine
    M, B, S, n = 4, 2, 3, 4096
    xs = mixtures(M, B, S, 42, LINE, n)
    plain = GCCNMFArrayEngine(n, reconstruction='spatial', **engine_kw(M, B, S, LINE))
    zero = GCCNMFArrayEngine(n, reconstruction='spatial', spatialIterations=0, **engine_kw(M, B, S, LINE))
    y0, y1 = plain.separate(xs), zero.separate(xs)
    assert plain.spatialIterations == 0 and zero.ws_em is None and zero.powers is None
    for name in ('X', 'V', 'CC', 'W', 'H', 'ang', 'tdoa_idx', 'scores', 'argmax', 'spec', 'cov', '_y'):
        assert same_bits(getattr(plain, name), getattr(zero, name)), name
    assert np.array_equal(y0, y1)
    ratio = GCCNMFArrayEngine(n, spatialIterations=0, **engine_kw(M, B, S, LINE))
    assert ratio.cov is None and ratio.reconstruction == 'ratio'


def test_two_channels_are_the_stereo_engine_bit_for_bit():
    from gcc_nmf_amd import _hip
    from gcc_nmf_amd.array import GCCNMFArrayEngine
    from gcc_nmf_amd.engine import GCCNMFEngine
    from gcc_nmf_amd.synthetic import synthetic_batch
    n, B, N_EM = 4096, 2, 3
    xs = synthetic_batch(3, B, numSamples=n)
    kw = dict(windowSize=256, hopSize=64, numTargets=2, dictionarySize=32, numIterations=5, batch=B)
    e = GCCNMFEngine(n, numTDOAs=128, reconstruction='spatial', spatialIterations=N_EM, nmf_groups=1, **kw)
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
    a = GCCNMFArrayEngine(n, numChannels=2, pairTDOAs=e.tdoasInSeconds[None], reconstruction='spatial', spatialIterations=N_EM, **kw)
    y = a.separate(xs)
    F, Fp = a.F, a.Fp
    for name, mine, theirs in (('arg-max', a.argmax, e.argmax), ('spec', a.spec, e.spec), ('waveforms', a._y, e.y.view(B, 4, -1)),
                               ('cov', a.cov[:, :, :F], e.ws_cov[:B * 2 * Fp * 4].view(B, 2, Fp, 4)[:, :, :F])):
        assert same_bits(mine, theirs), name
    assert y.shape == (B, 2, 2, a.L) and np.array_equal(y, e.y.cpu().numpy())
