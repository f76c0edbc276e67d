"""Ratio-mask reconstruction without a device: the engines' ``reconstruction`` keyword, the argument rules of the mode bit of
gccnmf_reconstruct (decided before any HIP call), and the float64 restatement (tests/ratio_restatement.py) on the reference's own
factors."""
import numpy as np
import pytest

import ratio_restatement as R
from conftest import golden

RATIO = 0x100                      # GCCNMF_RECONSTRUCT_RATIO (include/gccnmf_hip.h)
ERR_ARG, ERR_UNSUPPORTED = 1, 3
P = 4096                           # a non-null stand-in pointer: every call below returns before it touches memory


def _lib():
    from gcc_nmf_amd import _hip
    return _hip.lib()


def _no_device():
    import torch
    return not torch.cuda.is_available()


def test_engine_keyword_is_checked_before_the_device():
    from gcc_nmf_amd import _hip
    from gcc_nmf_amd.engine import GCCNMFEngine, RaggedGCCNMFEngine
    with pytest.raises(ValueError):
        GCCNMFEngine(160000, reconstruction='nonsense')
    with pytest.raises(ValueError):
        GCCNMFEngine(lengths=[160000, 80000], reconstruction='nonsense')
    with pytest.raises(ValueError):
        RaggedGCCNMFEngine([160000, 80000], reconstruction='nonsense')
    with pytest.raises(ValueError):
        GCCNMFEngine(160000, numTargets=9, reconstruction='ratio')          # the fused kernel's envelope: at most 8 targets
    if _no_device():
        for mode in ('ratio', 'direct'):
            with pytest.raises(_hip.HipLibraryError):                       # past the keyword check, stopped by the device check
                GCCNMFEngine(160000, reconstruction=mode)
            with pytest.raises(_hip.HipLibraryError):
                GCCNMFEngine(lengths=[160000, 80000], reconstruction=mode)


def test_header_constant_matches_python():
    import os
    import re
    from conftest import REPO
    from gcc_nmf_amd import engine
    text = open(os.path.join(REPO, 'include', 'gccnmf_hip.h')).read()
    m = re.search(r'#define\s+GCCNMF_RECONSTRUCT_RATIO\s+(\w+)', text)
    assert m and int(m.group(1), 0) == engine.GCCNMF_RECONSTRUCT_RATIO == RATIO


def _reconstruct(S, X=P, V=P, ws=P, argmax=P, masks=None):
    return _lib().gccnmf_reconstruct(P, P, argmax, masks, X, V, 513, 100, 128, S, 2, ws, P, None)


def test_mode_bit_argument_rules():
    assert _reconstruct(9 | RATIO) == ERR_UNSUPPORTED
    assert _reconstruct(9 | RATIO, V=None, ws=None) == ERR_UNSUPPORTED      # neither |X| nor the workspace is needed in this mode
    assert _reconstruct(255 | RATIO) == ERR_UNSUPPORTED
    assert _reconstruct(3 | RATIO, X=None) == ERR_ARG
    assert _reconstruct(9 | RATIO, X=None) == ERR_ARG                       # arguments first, as for the direct mode
    assert _reconstruct(3, X=None) == ERR_ARG
    assert _reconstruct(3 | RATIO, argmax=None, masks=None) == ERR_ARG
    assert _reconstruct(0 | RATIO) == ERR_ARG
    for other in (0x200, 0x400, 1 << 16, RATIO | 0x200):
        assert _reconstruct(3 | other) == ERR_ARG                           # no other mode rides on S
    assert _reconstruct(3, ws=None) == ERR_ARG                              # the direct mode still needs its workspace and |X|
    assert _reconstruct(3, V=None) == ERR_ARG


def test_dropin_keyword_is_checked_first():
    from gcc_nmf_amd import gccNMFFunctions as G
    M = np.zeros((3, 4, 5), np.float32)
    X = np.zeros((2, 9, 5), np.complex64)
    with pytest.raises(ValueError):
        G.getTargetSpectrogramEstimates(M, X, np.zeros((9, 4), np.float32), np.zeros((2, 4, 5), np.float32), reconstruction='nonsense')
    with pytest.raises(ValueError):
        G.getTargetSpectrogramEstimates(np.zeros((9, 4, 5), np.float32), X, np.zeros((9, 4), np.float32), np.zeros((2, 4, 5), np.float32),
                                        reconstruction='ratio')


@pytest.fixture(scope='module')
def factors():
    g = golden('dev1_hop256_K128')
    W, H, am = g['W_sub'], g['H_sub'], g['argmax']
    assert W.shape == (513, 128) and H.shape == (128, 1244) and am.shape == (128, 622)
    rng = np.random.RandomState(5)
    X = np.exp(1j * rng.uniform(-np.pi, np.pi, (2, 513, 622)))             # unit modulus
    return W, H, am, X


def test_restatement_on_the_reference_factors(factors):
    W, H, am, X = factors
    S = int(am.max()) + 1
    assert S == 3
    den = R.denominators(W, H, argmax=am, S=S)
    assert den.shape == (2, 513, 622) and (den > 0).all(), 'den > 0 everywhere on this fixture: nothing is masked out below'
    est = R.ratio_one_hot(W, H, am, S, X)
    assert est.shape == (S, 2, 513, 622)
    # the targets add up to the mixture
    assert np.abs(est.sum(axis=0) - X).max() <= 1e-12
    # one target returns the mixture
    one = R.ratio_one_hot(W, H, np.zeros_like(am), 1, X)
    assert np.abs(one[0] - X).max() <= 1e-14
    # the soft form, given one-hot masks, is the one-hot form: W.H_c == sum_i W.(H_c o M_i) up to float64 rounding
    soft = R.ratio_soft(W, H, R.one_hot(am, S), X)
    assert np.abs(soft - est).max() <= 1e-12 * np.abs(X).max()
    assert (np.abs(soft - est) <= 1e-12 * np.abs(X)[None]).all()


def test_restatement_zero_denominator_and_nan():
    rng = np.random.RandomState(2)
    F, K, T, S = 9, 6, 7, 3
    W, H = rng.rand(F, K), rng.rand(K, 2 * T)
    am = rng.randint(0, S, (K, T))
    X = rng.randn(2, F, T) + 1j * rng.randn(2, F, T)
    H[:, 3] = 0                                                            # frame 3 of channel 0: den == 0
    H[2, T + 5] = np.nan                                                   # frame 5 of channel 1
    est = R.ratio_one_hot(W, H, am, S, X)
    assert (est[:, 0, :, 3] == 0).all()
    assert np.isnan(est[:, 1, :, 5]).all()
    keep = np.ones((2, T), bool)
    keep[0, 3] = keep[1, 5] = False
    assert np.isfinite(est[:, keep[:, None, :].repeat(F, 1)]).all()
    assert np.abs((est.sum(0) - X)[keep[:, None, :].repeat(F, 1)]).max() < 1e-12
