"""Argument rules of the fixed-dictionary KL-NMF call (GCCNMF_FLAG_FIXED_W / GCCNMF_FLAG_H_ONES) and the engine's dictionary checks:
all decided before anything reaches a device."""
import numpy as np
import pytest

FIXED_W, H_ONES = 1 << 16, 1 << 17
ERR_ARG, ERR_UNSUPPORTED = 1, 3
P = 4096        # a non-null stand-in pointer: every call below returns before it touches memory


def _lib():
    from gcc_nmf_amd import _hip
    return _hip.lib()


def _klnmf(flags, F=513, N=100, K=128, batch=2):
    return _lib().gccnmf_klnmf(P, P, P, P, F, N, K, batch, 10, 0.0, 1e-16, flags, None)


@pytest.mark.parametrize('extra', [1, 2, 4, 4 | (2 << 8), 1 << 15, 1 << 18])
def test_fixed_w_with_other_bits_is_an_argument_error(extra):
    assert _klnmf(FIXED_W | extra) == ERR_ARG
    assert _klnmf(FIXED_W | H_ONES | extra) == ERR_ARG


def test_h_ones_alone_is_an_argument_error():
    assert _klnmf(H_ONES) == ERR_ARG


@pytest.mark.parametrize('bit', [FIXED_W, H_ONES, FIXED_W | H_ONES])
def test_stage_and_ragged_reject_the_new_bits(bit):
    import ctypes
    lib = _lib()
    assert lib.gccnmf_klnmf_stage(P, P, P, P, 513, 100, 128, 2, 0.0, 1e-16, bit, 1, None) == ERR_ARG
    n = (ctypes.c_int * 2)(100, 80)
    assert lib.gccnmf_klnmf_ragged(P, P, P, P, 513, n, 100, 128, 2, 10, 0.0, 1e-16, bit, None) == ERR_ARG


def test_outside_the_envelope_is_unsupported():
    assert _klnmf(FIXED_W, K=1025) == ERR_UNSUPPORTED
    assert _klnmf(FIXED_W, F=2050) == ERR_UNSUPPORTED


def test_plan_bit_4_only_with_the_flag():
    lib = _lib()
    for F, N, K, B in [(513, 1244, 128, 64), (513, 1244, 1024, 64), (129, 77, 1, 1), (2049, 1, 1024, 3)]:
        assert lib.gccnmf_klnmf_plan(F, N, K, B, FIXED_W) == 16
        assert lib.gccnmf_klnmf_plan(F, N, K, B, FIXED_W | H_ONES) == 16
        plain = lib.gccnmf_klnmf_plan(F, N, K, B, 0)
        assert plain >= 0 and not plain & 16
    assert lib.gccnmf_klnmf_plan(513, 100, 1025, 2, FIXED_W) == -1
    assert lib.gccnmf_klnmf_plan(513, 100, 128, 2, FIXED_W | 1) == -1


def test_engine_rejects_bad_dictionaries():
    from gcc_nmf_amd.engine import check_dictionary
    W = np.random.RandomState(0).rand(513, 64).astype(np.float32)
    assert check_dictionary(W, 513).dtype == np.float32
    with pytest.raises(ValueError):
        check_dictionary(W[:512], 513)
    with pytest.raises(ValueError):
        check_dictionary(W[:, 0], 513)
    with pytest.raises(ValueError):
        check_dictionary(np.zeros((513, 1025), np.float32), 513)
    bad = W.copy()
    bad[3, 4] = -1
    with pytest.raises(ValueError):
        check_dictionary(bad, 513)
    bad[3, 4] = np.nan
    with pytest.raises(ValueError):
        check_dictionary(bad, 513)
