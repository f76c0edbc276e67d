"""Spatial (multichannel Wiener) reconstruction without a device: the properties of the float64 restatement
(tests/spatial_restatement.py), the ``reconstruction='spatial'`` keyword, the argument rules of the mode bit in the upper half of
gccnmf_reconstruct's batch (decided before any HIP call), the constants shared by the header and Python, and the reverberant mixture
generator of the CPU study."""
import os
import re

import numpy as np
import pytest

import spatial_restatement as SR
from conftest import REPO

RATIO = 0x100                      # GCCNMF_RECONSTRUCT_RATIO (include/gccnmf_hip.h)
SPATIAL = 1 << 16                  # GCCNMF_RECONSTRUCT_SPATIAL_BIT
ERR_ARG, ERR_UNSUPPORTED = 1, 3
P = 4096                           # a non-null, 16-byte aligned stand-in pointer: every call below returns before it touches memory


def random_estimates(S, F, T, seed):
    rng = np.random.RandomState(seed)
    E = ((rng.randn(S, 2, F, T) + 1j * rng.randn(S, 2, F, T)) * rng.uniform(0.1, 3.0, (S, 1, F, 1))).astype(np.complex64)
    return E, E.sum(axis=0).astype(np.complex64)


@pytest.mark.parametrize('S', [1, 2, 3, 8])
def test_outputs_sum_to_the_mixture(S):
    """sum_i v_i R~_i y = Sigma y = X whatever X is (it need not be the sum of the estimates)."""
    E, _ = random_estimates(S, 7, 13, S)
    rng = np.random.RandomState(50 + S)
    X = (rng.randn(2, 7, 13) + 1j * rng.randn(2, 7, 13)).astype(np.complex64)
    out = SR.spatial_filter(E, X)
    assert out.shape == E.shape and out.dtype == np.complex128
    assert np.abs(out.sum(axis=0) - X).max() <= 1e-10 * np.abs(X).max()
    if S == 1:
        assert np.abs(out[0] - X).max() <= 1e-10 * np.abs(X).max(), 'one target returns the mixture'


def test_channel_swap():
    E, X = random_estimates(3, 6, 9, 7)
    out = SR.spatial_filter(E, X)
    swapped = SR.spatial_filter(E[:, ::-1], X[::-1])
    assert np.abs(swapped[:, ::-1] - out).max() <= 1e-12 * np.abs(X).max()
    f32 = SR.spatial_filter(E, X, np.float32)
    assert np.array_equal(SR.spatial_filter(E[:, ::-1], X[::-1], np.float32)[:, ::-1], f32), 'the stated roundings are symmetric in the channels'


def test_zero_power_rule_and_identity_covariance():
    E, X = random_estimates(3, 6, 9, 11)
    E[:, :, 2, 4] = 0                      # an all-zero (f, t): every target is 0 there
    E[1, :, 5, :] = 0                      # target 1 is silent in bin 5: n = 0, R = I
    X = E.sum(axis=0).astype(np.complex64)
    R = SR.covariances(E)
    assert R.shape == (3, 6, 4) and R.dtype == np.float32
    assert np.array_equal(R[1, 5], np.array([1 + SR.LOADING, 1 + SR.LOADING, 0, 0], np.float32))
    assert np.allclose(R[..., 0] + R[..., 1], 2 + 2 * SR.LOADING, atol=1e-6), 'trace 2 plus the loading'
    out = SR.spatial_filter(E, X)
    assert (out[:, :, 2, 4] == 0).all()
    assert (out[1, :, 5, :] == 0).all(), 'v = 0: a silent target stays silent'
    assert np.isfinite(out).all()
    keep = np.ones((6, 9), bool)
    keep[2, 4] = False
    assert np.abs((out.sum(axis=0) - X)[:, keep]).max() <= 1e-10 * np.abs(X).max()


def test_nan_propagates_through_the_covariance():
    E, X = random_estimates(2, 4, 6, 13)
    E[0, 1, 2, 3] = np.nan
    out = SR.spatial_filter(E, X)
    assert np.isnan(out[:, :, 2, :]).all(), 'the bin of the NaN: its covariance is NaN in every frame'
    rest = np.ones(4, bool)
    rest[2] = False
    assert np.isfinite(out[:, :, rest, :]).all()


def test_measured_bar_is_a_float32_distance():
    E, X = random_estimates(3, 33, 20, 17)
    bar, err, ref = SR.measured_bar(E, X)
    assert bar == SR.BAR_FACTOR * err and 0 < err < 1e-3
    assert np.array_equal(ref, SR.spatial_filter(E, X))


def test_scaled_evaluation_is_the_literal_one_until_it_underflows():
    """The float32 evaluation on v_j 2^-e: the literal evaluation's bits on ordinary data; on a nearly silent frame (|X| ~ 1e-10: the
    determinant ~ 1e-43 is subnormal) the literal form loses the frame and the scaled one stays at float32 accuracy of that frame."""
    E, X = random_estimates(3, 17, 12, 23)
    assert np.array_equal(SR.spatial_filter(E, X, np.float32), SR.spatial_filter(E, X, np.float32, scaled=False))
    E[..., 5] *= np.float32(1e-10)
    X = E.sum(axis=0).astype(np.complex64)
    ref, scaled, literal = SR.spatial_filter(E, X), SR.spatial_filter(E, X, np.float32), SR.spatial_filter(E, X, np.float32, scaled=False)
    quiet = np.abs(X[..., 5]).max()
    assert np.isfinite(scaled).all() and np.abs(scaled[..., 5] - ref[..., 5]).max() <= 1e-5 * quiet
    lost = ~np.isfinite(literal[..., 5]) | (np.abs(literal[..., 5] - ref[..., 5]) > quiet)
    assert lost.any(), 'the literal float32 form does not survive this frame: the reason for the scaling'
    other = np.arange(12) != 5
    assert np.array_equal(scaled[..., other], literal[..., other])


def test_loading_is_a_parameter_of_the_restatement():
    E, X = random_estimates(2, 5, 8, 29)
    assert np.array_equal(SR.covariances(E), SR.covariances(E, loading=SR.LOADING))
    R1 = SR.covariances(E, loading=0.1)
    assert np.allclose(R1[..., :2] - SR.covariances(E)[..., :2], 0.1 - SR.LOADING, atol=1e-6) and SR.LOADING == 1e-3
    assert not np.array_equal(SR.spatial_filter(E, X, loading=0.1), SR.spatial_filter(E, X))


def test_best_assignment_sdr_scores_a_known_snr_and_undoes_a_permutation():
    """The scoring behind the study's figures: estimate[n] belongs to image[n + windowSize / 2]; an estimate that is the image plus
    noise 20 dB below it scores 20 dB, and outputs handed over in another order are assigned back."""
    rng = np.random.RandomState(3)
    ws, n = 1024, 30000
    images = rng.randn(3, 2, n) * np.array([1.0, 0.5, 2.0])[:, None, None]
    L = n - ws
    clean = images[:, :, ws // 2:ws // 2 + L]
    noise = rng.randn(3, 2, L)
    noise *= (np.sqrt((clean ** 2).sum(axis=(1, 2)) / (noise ** 2).sum(axis=(1, 2))) * 10 ** (-20 / 20.0))[:, None, None]
    order = [2, 0, 1]                                      # output j holds source order[j]
    sdr, perm = SR.best_assignment_sdr((clean + noise)[order], images, ws)
    assert list(perm) == [order.index(i) for i in range(3)]
    assert np.abs(sdr - 20.0).max() < 0.3
    shifted, _ = SR.best_assignment_sdr(np.roll(clean + noise, 7, axis=-1), images, ws)
    assert shifted.max() < 3.0, 'a misaligned estimate must not score'


def test_keyword_accepts_one_to_eight_targets():
    from gcc_nmf_amd import engine
    assert 'spatial' in engine.RECONSTRUCTIONS
    for n in range(1, 9):
        assert engine.check_reconstruction('spatial', n) == 'spatial'
    for n in (0, 9, 255):
        with pytest.raises(ValueError):
            engine.check_reconstruction('spatial', n)
    with pytest.raises(ValueError):
        engine.check_reconstruction('nonsense', 3)
    assert engine.check_reconstruction('direct', 100) == 'direct'


def test_engine_and_dropin_check_the_keyword_before_the_device():
    import torch
    from gcc_nmf_amd import _hip, gccNMFFunctions as G
    from gcc_nmf_amd.engine import GCCNMFEngine
    with pytest.raises(ValueError):
        GCCNMFEngine(160000, numTargets=9, reconstruction='spatial')
    with pytest.raises(ValueError):
        GCCNMFEngine(lengths=[160000, 80000], numTargets=9, reconstruction='spatial')
    with pytest.raises(ValueError):
        G.getTargetSpectrogramEstimates(np.zeros((9, 4, 5), np.float32), np.zeros((2, 9, 5), np.complex64), np.zeros((9, 4), np.float32),
                                        np.zeros((2, 4, 5), np.float32), reconstruction='spatial')
    if not torch.cuda.is_available():
        with pytest.raises(_hip.HipLibraryError):                           # past the keyword check, stopped by the device check
            GCCNMFEngine(160000, reconstruction='spatial')
        with pytest.raises(_hip.HipLibraryError):
            GCCNMFEngine(lengths=[160000, 80000], reconstruction='spatial', tdoaTracking=True, localizationWindowSize=9)


def test_header_constants_match_python():
    from gcc_nmf_amd import _hip
    text = open(os.path.join(REPO, 'include', 'gccnmf_hip.h')).read()
    bit = re.search(r'#define\s+GCCNMF_RECONSTRUCT_SPATIAL_BIT\s+\((\d+)\s*<<\s*(\d+)\)', text)
    assert bit and int(bit.group(1)) << int(bit.group(2)) == _hip.GCCNMF_RECONSTRUCT_SPATIAL_BIT == SPATIAL
    assert re.search(r'#define\s+GCCNMF_RECONSTRUCT_SPATIAL_BATCH\(batch\)\s+\(\(batch\) \| GCCNMF_RECONSTRUCT_SPATIAL_BIT\)', text)
    lam = re.search(r'#define\s+GCCNMF_SPATIAL_LOADING\s+(\S+)', text)
    assert lam and float(lam.group(1)) == _hip.GCCNMF_SPATIAL_LOADING == SR.LOADING == 1e-3
    ws = re.search(r'#define\s+GCCNMF_RECONSTRUCT_SPATIAL_WORKSPACE_FLOATS\(batch, S, Fp\)\s+\((\d+)L \* \(batch\) \* \(S\) \* \(Fp\)\)', text)
    assert ws and int(ws.group(1)) == 4
    for batch, S, F in ((1, 1, 513), (5, 3, 201), (64, 8, 513)):
        Fp = -(-F // 16) * 16
        assert _hip.reconstruct_spatial_workspace_floats(batch, S, Fp) == 4 * batch * S * Fp
        assert _hip.reconstruct_spatial_batch(batch) == batch | SPATIAL
    for bad in (0, 65536, -1):
        with pytest.raises(ValueError):
            _hip.reconstruct_spatial_batch(bad)


def _reconstruct(S, batch, X=P, V=P, ws=P, spec=P):
    from gcc_nmf_amd import _hip
    return _hip.lib().gccnmf_reconstruct(P, P, P, None, X, V, 513, 100, 128, S, batch, ws, spec, None)


def test_mode_bit_argument_rules():
    """Every rule is decided before the first HIP call: no device is needed, and no pointer is touched."""
    assert _reconstruct(3 | RATIO, 2 | SPATIAL, ws=None) == ERR_ARG                # the covariances need a workspace
    assert _reconstruct(3 | RATIO, 2 | SPATIAL, ws=P + 4) == ERR_ARG               # 16-byte aligned
    assert _reconstruct(3 | RATIO, 2 | SPATIAL, ws=P + 8) == ERR_ARG
    assert _reconstruct(3 | RATIO, 2 | SPATIAL, X=None) == ERR_ARG
    assert _reconstruct(3 | RATIO, 2 | SPATIAL, spec=None) == ERR_ARG
    assert _reconstruct(3, 2 | SPATIAL) == ERR_ARG                                 # the mode bit without the ratio stage
    assert _reconstruct(3, 65537) == ERR_ARG                                       # (which is what a direct batch above 65535 is)
    assert _reconstruct(3 | RATIO, SPATIAL) == ERR_ARG                             # no files
    for other in (1 << 17, 1 << 20, 1 << 30, SPATIAL | 1 << 17):
        assert _reconstruct(3 | RATIO, 2 | other) == ERR_ARG                       # no other bit rides on batch
        assert _reconstruct(3, 2 | other) == ERR_ARG
    assert _reconstruct(3 | RATIO, -2) == ERR_ARG
    assert _reconstruct(9 | RATIO, 2 | SPATIAL) == ERR_UNSUPPORTED                 # the ratio stage's envelope, after the argument rules
    assert _reconstruct(9 | RATIO, 2 | SPATIAL, ws=None) == ERR_ARG
    assert _reconstruct(0 | RATIO, 2 | SPATIAL) == ERR_ARG
    assert _reconstruct(9 | RATIO, 2, V=None, ws=None) == ERR_UNSUPPORTED          # the plain ratio mode still needs neither


def test_reverberant_mixture():
    from gcc_nmf_amd.synthetic import reverberant_mixture
    x, images = reverberant_mixture(3, numSamples=24000, returnSources=True)
    assert x.shape == (2, 24000) and x.dtype == np.float32 and images.shape == (3, 2, 24000) and images.dtype == np.float64
    assert np.array_equal(x, reverberant_mixture(3, numSamples=24000)), 'deterministic'
    assert not np.array_equal(x, reverberant_mixture(4, numSamples=24000))
    assert np.array_equal(x * 32768, np.round(x * 32768)) and np.abs(x).max() <= 0.1 + 0.5 / 32768, 'int16-representable'
    assert np.abs(images.sum(axis=0) - x).max() <= 0.5 / 32768 + 1e-12, 'the images add up to the mixture before it is rounded to int16'
    # the impulse responses give every source a full-rank spatial covariance: its channels are not delayed copies of each other
    dry, dry_images = reverberant_mixture(3, numSamples=24000, reverbGain=0.0, returnSources=True)
    for j, d in enumerate((-20, 3, 27)):
        assert np.abs(np.roll(dry_images[j, 0], d) - dry_images[j, 1]).max() <= 1e-12
        assert np.abs(np.roll(images[j, 0], d) - images[j, 1]).max() > 1e-3
