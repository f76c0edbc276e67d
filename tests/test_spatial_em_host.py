"""EM refinement of the spatial reconstruction without a device: the properties of the float64 restatement
(tests/spatial_em_restatement.py), its evaluated form against the definition as written, the ``spatialIterations`` keyword, the
argument rules of the iteration bits of gccnmf_reconstruct's S (decided before any HIP call), the constants shared by the header and
Python, and the sign of what the iterations buy on a study mixture."""
import os
import re

import numpy as np
import pytest

import spatial_em_restatement as EM
import spatial_restatement as SR
from conftest import REPO

RATIO = 0x100                      # GCCNMF_RECONSTRUCT_RATIO (include/gccnmf_hip.h)
SPATIAL = 1 << 16                  # GCCNMF_RECONSTRUCT_SPATIAL_BIT
ITER = lambda n: n << 20           # GCCNMF_RECONSTRUCT_SPATIAL_ITERATIONS(n)
ERR_ARG, ERR_UNSUPPORTED = 1, 3
P = 4096                           # a non-null, 16-byte aligned stand-in pointer: every call below returns before it touches memory


def random_estimates(S, F, T, seed):
    rng = np.random.RandomState(seed)
    E = ((rng.randn(S, 2, F, T) + 1j * rng.randn(S, 2, F, T)) * rng.uniform(0.1, 3.0, (S, 1, F, 1))).astype(np.complex64)
    return E, E.sum(axis=0).astype(np.complex64)


def test_zero_iterations_is_the_spatial_filter_bit_for_bit():
    E, X = random_estimates(3, 9, 21, 1)
    for dtype in (np.float64, np.float32):
        assert np.array_equal(EM.spatial_em(E, X, 0, dtype), SR.spatial_filter(E, X, dtype))
        # ... and the output stage used behind the iterations is SR.spatial_filter's arithmetic, given the same powers and covariances
        assert np.array_equal(EM.filter_with(SR.powers(E, dtype), SR.covariances(E), X, dtype), SR.spatial_filter(E, X, dtype))
    v, R = EM.refine(E, X, 0)
    assert np.array_equal(v, SR.powers(E)) and np.array_equal(R, SR.covariances(E))


def test_evaluated_form_is_the_definition():
    """em_step's rearranged form (no inverse of R~_i, no 2 - tr G_i) against the definition with complex 2 x 2 matrices, float64."""
    E, X = random_estimates(3, 9, 21, 2)
    v, R = SR.powers(E), SR.covariances(E)
    for _ in range(3):
        lv, lR = EM.literal_step(v, R, X)
        v, R = EM.em_step(v, R, X)
        assert np.abs(v - lv).max() <= 1e-12 * np.abs(lv).max()
        assert np.abs(lR - np.conj(np.swapaxes(lR, -1, -2))).max() <= 1e-12, 'C_i is Hermitian'
        half = 0.5 * (lR[..., 0, 0].real + lR[..., 1, 1].real)
        want = np.stack([lR[..., 0, 0].real + SR.LOADING * half, lR[..., 1, 1].real + SR.LOADING * half, lR[..., 0, 1].real, lR[..., 0, 1].imag], -1)
        assert R.dtype == np.float32 and np.abs(R - want).max() <= 2.0 ** -22, 'rounded to float32 once: entries below 4'
        assert np.abs(R[..., 0] + R[..., 1] - 2).max() < 0.2, 'no renormalisation, and the trace stays near 2'
    # the scaled float64 evaluation is the unscaled one up to rounding
    a, b = EM.em_step(SR.powers(E), SR.covariances(E), X, scaled=True), EM.em_step(SR.powers(E), SR.covariances(E), X, scaled=False)
    assert np.abs(a[0] - b[0]).max() <= 1e-12 * np.abs(b[0]).max()


@pytest.mark.parametrize('n', [1, 5])
@pytest.mark.parametrize('S', [1, 2, 3, 8])
def test_outputs_sum_to_the_mixture(S, n):
    E, _ = random_estimates(S, 7, 13, S)
    rng = np.random.RandomState(50 + S)
    X = (rng.randn(2, 7, 13) + 1j * rng.randn(2, 7, 13)).astype(np.complex64)
    bar, err, ref = EM.measured_bar(E, X, n)
    assert ref.shape == E.shape and ref.dtype == np.complex128 and 0 < err < 1e-3 and bar == EM.BAR_FACTOR * err
    assert np.array_equal(ref, EM.spatial_em(E, X, n))
    scale = np.abs(X).max()
    assert np.abs(ref.sum(axis=0) - X).max() <= bar * scale
    assert np.abs(EM.spatial_em(E, X, n, np.float32).astype(np.complex128).sum(axis=0) - X).max() <= bar * scale
    if S == 1:
        assert np.abs(ref[0] - X).max() <= bar * scale, 'one target returns the mixture at any n'
    else:
        assert np.abs(ref - SR.spatial_filter(E, X)).max() > 100 * bar * scale, 'the iterations do something'


def test_channel_swap():
    E, X = random_estimates(3, 6, 9, 7)
    for n in (1, 4):
        out = EM.spatial_em(E, X, n)
        swapped = EM.spatial_em(E[:, ::-1], X[::-1], n)
        assert np.abs(swapped[:, ::-1] - out).max() <= 1e-10 * np.abs(X).max()


def test_an_empty_target_stays_empty():
    """An all-zero target (an empty slot of numTargets='auto'): its powers stay 0, its covariance stays (1 + lambda) I, and the other
    targets get the bits they get without it."""
    E, X = random_estimates(3, 6, 9, 11)
    E4 = np.concatenate([E[:2], np.zeros_like(E[:1]), E[2:]])          # slot 2 of 4 is empty
    lam1 = np.float32(1 + SR.LOADING)
    for dtype in (np.float64, np.float32):
        v, R = EM.refine(E4, X, 3, dtype)
        assert (v[2] == 0).all() and np.array_equal(R[2], np.tile(np.array([lam1, lam1, 0, 0], np.float32), (6, 1)))
        out = EM.spatial_em(E4, X, 3, dtype)
        assert (out[2] == 0).all()
        assert np.array_equal(out[[0, 1, 3]], EM.spatial_em(E, X, 3, dtype))
    # a target silent in one frame stays silent there: the set of skipped frames is fixed by the input
    E[1, :, :, 4] = 0
    v, _ = EM.refine(E, X, 4)
    assert (v[1, :, 4] == 0).all() and (v[1, :, :4] > 0).all() and (v[[0, 2]] > 0).all()
    E[:, :, 2, 5] = 0                                                   # an all-zero (f, t)
    assert (EM.spatial_em(E, X, 2)[:, :, 2, 5] == 0).all()


def test_nan_stays_in_its_bin():
    E, X = random_estimates(2, 4, 6, 13)
    X = X.copy()
    X[0, 2, 3] = np.nan
    for dtype in (np.float64, np.float32):
        out = EM.spatial_em(E, X, 2, dtype)
        rest = np.arange(4) != 2
        assert np.isnan(out[:, :, 2, :]).all(), 'the NaN frame is counted: the covariances of its bin are NaN, and so is the bin'
        assert np.isfinite(out[:, :, rest, :]).all()
    EM.measured_bar(E, X, 2)                                            # the patterns agree between the precisions


def _reconstruct(S, batch, X=P, V=P, ws=P, spec=P):
    from gcc_nmf_amd import _hip
    return _hip.lib().gccnmf_reconstruct(P, P, P, None, X, V, 513, 100, 128, S, batch, ws, spec, None)


def test_iteration_bits_argument_rules():
    """Every rule is decided before the first HIP call: no device is needed, and no pointer is touched."""
    for n in (1, 2, 255):
        assert _reconstruct(3 | RATIO | ITER(n), 2) == ERR_ARG                     # without the spatial bit of batch
        assert _reconstruct(3 | ITER(n), 2 | SPATIAL) == ERR_ARG                   # without GCCNMF_RECONSTRUCT_RATIO
        assert _reconstruct(3 | ITER(n), 2) == ERR_ARG
        assert _reconstruct(3 | RATIO | ITER(n), 2 | SPATIAL, ws=None) == ERR_ARG
        assert _reconstruct(3 | RATIO | ITER(n), 2 | SPATIAL, ws=P + 4) == ERR_ARG
        assert _reconstruct(3 | RATIO | ITER(n), 2 | SPATIAL, ws=P + 8) == ERR_ARG
        assert _reconstruct(3 | RATIO | ITER(n), 2 | SPATIAL, X=None) == ERR_ARG
        assert _reconstruct(9 | RATIO | ITER(n), 2 | SPATIAL) == ERR_UNSUPPORTED   # the envelope, after the argument rules
        assert _reconstruct(0 | RATIO | ITER(n), 2 | SPATIAL) == ERR_ARG
    for bit in list(range(9, 20)) + [28, 29, 30]:                                  # no other bit rides on S
        assert _reconstruct(3 | RATIO | 1 << bit, 2 | SPATIAL) == ERR_ARG, bit
        assert _reconstruct(3 | RATIO | ITER(2) | 1 << bit, 2 | SPATIAL) == ERR_ARG, bit
        assert _reconstruct(3 | 1 << bit, 2) == ERR_ARG, bit
    assert _reconstruct(3 | RATIO | ITER(256), 2 | SPATIAL) == ERR_ARG             # n = 256 is bit 28
    assert _reconstruct(-(1 << 31) | 3 | RATIO | ITER(2), 2 | SPATIAL) == ERR_ARG  # bit 31
    for other in (1 << 17, 1 << 20, SPATIAL | 1 << 17):
        assert _reconstruct(3 | RATIO | ITER(2), 2 | other) == ERR_ARG             # batch keeps its rules


def test_header_constants_match_python():
    from gcc_nmf_amd import _hip
    text = open(os.path.join(REPO, 'include', 'gccnmf_hip.h')).read()
    m = re.search(r'#define\s+GCCNMF_RECONSTRUCT_SPATIAL_ITERATIONS\(n\)\s+\(\(n\) << (\d+)\)', text)
    assert m and int(m.group(1)) == _hip.GCCNMF_RECONSTRUCT_SPATIAL_ITERATIONS_SHIFT == 20
    assert _hip.MAX_SPATIAL_ITERATIONS == 255
    assert re.search(r'#define\s+GCCNMF_RECONSTRUCT_SPATIAL_EM_WORKSPACE_FLOATS\(batch, S, Fp, Tp\)\s+'
                     r'\(4L \* \(batch\) \* \(S\) \* \(Fp\) \+ \(long\)\(batch\) \* \(S\) \* \(Fp\) \* \(Tp\)\)', text)
    for batch, S, F, T in ((1, 1, 513, 1), (5, 3, 201, 37), (64, 8, 513, 622)):
        Fp, Tp = -(-F // 16) * 16, -(-T // 64) * 64
        want = 4 * batch * S * Fp + batch * S * Fp * Tp
        assert _hip.reconstruct_spatial_em_workspace_floats(batch, S, Fp, Tp) == want
        assert _hip.reconstruct_workspace_floats('spatial', T, 64, S, batch, Fp, iterations=2) == want
        assert _hip.reconstruct_workspace_floats('spatial', T, 64, S, batch, Fp) == 4 * batch * S * Fp == \
            _hip.reconstruct_workspace_floats('spatial', T, 64, S, batch, Fp, iterations=0)
        assert (4 * batch * S * Fp) % 4 == 0, 'the powers start 16-byte aligned'
        assert _hip.reconstruct_workspace_floats('ratio', T, 64, S, batch, Fp) == 0
    assert _hip.reconstruct_word(3, 'direct') == 3 and _hip.reconstruct_word(3, 'ratio') == 3 | RATIO == _hip.reconstruct_word(3, 'spatial')
    assert _hip.reconstruct_word(3, 'spatial', 5) == 3 | RATIO | ITER(5) and _hip.reconstruct_word(8, 'spatial', 255) == 8 | RATIO | ITER(255)
    assert len(_hip.SIGNATURES) == 46, 'no new entry point'


def test_keyword_is_checked_before_the_device():
    import torch
    from gcc_nmf_amd import _hip, gccNMFFunctions as G
    from gcc_nmf_amd.engine import GCCNMFEngine, GCCNMFEnhancementEngine
    for n in (0, 1, 255, np.int64(7)):
        assert _hip.check_spatial_iterations(n, 'spatial') == int(n)
    assert _hip.check_spatial_iterations(0, 'ratio') == 0 and _hip.check_spatial_iterations(0, 'direct') == 0
    bad = [dict(spatialIterations=n, reconstruction='spatial') for n in (-1, 256, 1.5, True, '2', None)]
    bad += [dict(spatialIterations=2, reconstruction='ratio'), dict(spatialIterations=1, reconstruction='direct'), dict(spatialIterations=1)]
    for kw in bad:
        with pytest.raises(ValueError):
            _hip.check_spatial_iterations(kw['spatialIterations'], kw.get('reconstruction', 'direct'))
        with pytest.raises(ValueError):
            GCCNMFEngine(160000, **kw)
        with pytest.raises(ValueError):
            GCCNMFEngine(lengths=[160000, 80000], **kw)
        with pytest.raises(ValueError):
            GCCNMFEngine(160000, numTargets='auto', **kw)
        with pytest.raises(ValueError):
            GCCNMFEnhancementEngine(160000, **kw)
        with pytest.raises(ValueError):
            G.getTargetSpectrogramEstimates(np.zeros((3, 4, 5), np.float32), np.zeros((2, 9, 5), np.complex64), np.zeros((9, 4), np.float32),
                                            np.zeros((2, 4, 5), np.float32), **kw)
        with pytest.raises(ValueError):
            _hip.reconstruct_word(3, kw.get('reconstruction', 'direct'), kw['spatialIterations'])
    if not torch.cuda.is_available():
        for make in (lambda: GCCNMFEngine(160000, reconstruction='spatial', spatialIterations=3),
                     lambda: GCCNMFEngine(lengths=[160000, 80000], reconstruction='spatial', spatialIterations=3),
                     lambda: GCCNMFEngine(160000, reconstruction='spatial', spatialIterations=3, dictionaryW=np.ones((513, 64), np.float32),
                                          numFreeAtoms=16),
                     lambda: GCCNMFEngine(160000, reconstruction='spatial', spatialIterations=3, tdoaTracking=True, localizationWindowSize=9),
                     lambda: GCCNMFEngine(160000, reconstruction='spatial', spatialIterations=3, numTargets='auto'),
                     lambda: GCCNMFEnhancementEngine(160000, reconstruction='spatial', spatialIterations=3)):
            with pytest.raises(_hip.HipLibraryError):                      # past the keyword check, stopped by the device check
                make()


def test_iterations_raise_the_sdr_of_a_study_mixture():
    """The first mixture of scripts/spatial_em_study.py, shortened to 2 s with K = 32 and 30 KL-NMF iterations so that the test takes a
    few seconds: the mean image SDR at n = 5 is above n = 0.  Only the sign is asserted; the study script records the sizes."""
    from gcc_nmf_amd.synthetic import reverberant_mixture
    from oracle import gccnmf_oracle as O
    import ratio_restatement as R
    x, images = reverberant_mixture(seed=0, numSamples=32000, returnSources=True)
    S = len(images)
    r = O.runGCCNMF(x, 16000, 1024, 256, 128, 1.0, S, dictionarySize=32, numIterations=30, return_intermediates=True)
    ratio = R.ratio_one_hot(r['W'], r['H'], np.nanargmax(r['G'], axis=0), S, r['X'])
    mean = {}
    for n in (0, 5):
        y = O.getTargetSignalEstimates(EM.spatial_em(ratio, r['X'], n).astype(np.complex64), 1024, 256, np.hanning)
        mean[n] = float(SR.best_assignment_sdr(y, images, 1024)[0].mean())
    print('mean image SDR: n = 0 %.2f dB, n = 5 %.2f dB' % (mean[0], mean[5]))
    assert mean[5] > mean[0]
