"""CPU: the comparison rules of the GCC stage tests (tests/gcc_checks.py) are sensitive.  A float32 product computed here passes them, and
each typical kernel mistake, applied to that product, is caught -- so the GPU tests that use these rules are not vacuous."""
import numpy as np
import pytest

import gcc_checks as C
from oracle import gccnmf_oracle as O


def gemm_case(M=129, N=70, Kd=201, seed=0):
    """float32 operands with the last reduction index and the last (Nyquist) output row 100x larger, as in the GPU stage tests."""
    rng = np.random.RandomState(seed)
    A = rng.uniform(-1, 1, (M, Kd)).astype(np.float32)
    B = rng.uniform(-1, 1, (Kd, N)).astype(np.float32)
    A[-1] *= 100
    A[:, -1] *= 100
    B[-1] *= 100
    ref = np.dot(A.astype(np.float64), B.astype(np.float64))
    absprod = np.dot(np.abs(A).astype(np.float64), np.abs(B).astype(np.float64))
    return A, B, ref, absprod


def test_float32_product_passes():
    for seed in range(4):
        A, B, ref, absprod = gemm_case(seed=seed)
        C.check_gemm_like(np.dot(A, B), ref, absprod, A.shape[1])
        # a sequential float32 sum (the worst order) still passes: the bound is a worst case, not a typical error
        acc = np.zeros(ref.shape, np.float32)
        for k in range(A.shape[1]):
            acc = (acc + np.outer(A[:, k], B[k]).astype(np.float32)).astype(np.float32)
        C.check_gemm_like(acc, ref, absprod, A.shape[1])


def _mutations():
    def drop_last_term(A, B, got):
        return np.dot(A[:, :-1], B[:-1])

    def drop_first_term(A, B, got):
        return np.dot(A[:, 1:], B[1:])

    def nyquist_row_zero(A, B, got):
        got[-1] = 0
        return got

    def nyquist_row_from_f_minus_2(A, B, got):
        got[-1] = got[-2]
        return got

    def tail_frame_shifted(A, B, got):
        got[:, -1] = got[:, -2]
        return got

    def tail_frame_unwritten(A, B, got):
        got[:, -1] = np.nan
        return got

    def tail_row_from_wrong_operand(A, B, got):
        got[-1] = np.dot(A[-2], B)             # the VALU tail row read one row off
        return got

    def one_element_off_by_one_term(A, B, got):
        got[3, 5] += np.float32(A[3, 100] * B[100, 5])
        return got

    return [drop_last_term, drop_first_term, nyquist_row_zero, nyquist_row_from_f_minus_2, tail_frame_shifted, tail_frame_unwritten,
            tail_row_from_wrong_operand, one_element_off_by_one_term]


@pytest.mark.parametrize('mutate', _mutations(), ids=lambda f: f.__name__)
def test_gemm_bound_catches(mutate):
    A, B, ref, absprod = gemm_case()
    got = mutate(A, B, np.dot(A, B))
    with pytest.raises(AssertionError):
        C.check_gemm_like(got, ref, absprod, A.shape[1])
    assert C.gemm_share(got, ref, absprod, A.shape[1]) > 1, 'the printed share of the bar says what the check says'
    with pytest.raises(AssertionError):
        C.report_gemm_like(got, ref, absprod, A.shape[1])


def test_the_printed_share_is_below_one_where_the_check_passes():
    A, B, ref, absprod = gemm_case()
    assert 0 < C.report_gemm_like(np.dot(A, B), ref, absprod, A.shape[1]) < 1
    assert C.gemm_share(ref.astype(np.complex64), ref.astype(np.complex128), absprod, A.shape[1]) < 1
    assert C.gemm_share(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), 5) == 0


def test_padding_set_to_one_is_caught():
    pad = np.zeros((3, 64, 61), np.float32)
    C.check_zero(pad)
    pad[2, 63, 60] = 1
    with pytest.raises(AssertionError):
        C.check_zero(pad)
    pad[2, 63, 60] = np.nan                     # never written over the NaN fill
    with pytest.raises(AssertionError):
        C.check_zero(pad)


def test_mean_check_catches_a_dropped_frame():
    ang = np.random.RandomState(1).uniform(-5, 5, (40, 65)).astype(np.float32)
    C.check_mean(np.mean(ang.astype(np.float64), axis=-1), ang)
    with pytest.raises(AssertionError):
        C.check_mean(np.sum(ang[:, :-1].astype(np.float64), axis=-1) / 65, ang)
    with pytest.raises(AssertionError):
        C.check_mean(np.mean(ang.astype(np.float32), axis=-1), ang.astype(np.float64) + 1e-3)


def test_peak_rule_keeps_the_larger_index_on_ties():
    v = np.zeros(30)
    v[5], v[10], v[20] = 1.0, 1.0, 2.0
    assert C.expected_peaks(v, 2) == ([10, 20], 0)
    assert O.estimateTargetTDOAIndexesFromAngularSpectrum(v, 1.0, 30, 2) == [10, 20]
    C.check_peaks([10, 20], 0, v, 2)
    with pytest.raises(AssertionError):
        C.check_peaks([5, 20], 0, v, 2)         # the smallest-index rule
    # plateaus are not strict maxima, NaN never compares greater, edges never qualify
    w = np.array([9.0, 1, 3, 3, 1, 2, np.nan, 5, 1, 4, 3, 8])
    assert C.expected_peaks(w, 2) == ([9, -1], 1)
    w2 = np.array([0.0, 2, 0, 2, 0, 1, 0])
    assert C.expected_peaks(w2, 2) == ([1, 3], 0) and C.expected_peaks(w2, 1) == ([3], 0)
    assert C.expected_peaks(w2, 4) == ([1, 3, 5, -1], 1)
    with pytest.raises(AssertionError):
        C.check_peaks([1, 3, 5, 0], 1, w2, 4)


def test_peak_rule_is_the_oracle_on_distinct_heights():
    rng = np.random.RandomState(3)
    for D in (3, 5, 33, 128, 200, 4096):
        for S in (1, 2, 3, 7):
            v = rng.standard_normal(D)
            idx, status = C.expected_peaks(v, S)
            if status == 0:
                assert idx == O.estimateTargetTDOAIndexesFromAngularSpectrum(v, 1.0, D, S), (D, S)
            else:
                with pytest.raises(ValueError):
                    O.estimateTargetTDOAIndexesFromAngularSpectrum(v, 1.0, D, S)


def test_argmax_check_catches_the_wrong_tie_winner_and_nan():
    s = np.random.RandomState(2).standard_normal((3, 8, 7)).astype(np.float32)
    s[2, 1, 6] = s[0, 1, 6] = 10.0              # tie in the last frame: nanargmax takes target 0
    s[0, 2, 5] = np.nan
    s[1, 2, 5] = 50.0
    good = np.nanargmax(s, axis=0)
    C.check_argmax(good, s)
    bad = good.copy()
    bad[1, 6] = 2
    with pytest.raises(AssertionError):
        C.check_argmax(bad, s)
    bad = np.argmax(s, axis=0)                  # NaN not ignored: argmax picks the NaN
    with pytest.raises(AssertionError):
        C.check_argmax(bad, s)
