"""Comparison rules of the GCC stage tests (tests/test_gpu_gcc_stages.py), in plain NumPy so that the CPU suite can show they are
sensitive (tests/test_gcc_checks.py) without torch or a device.

Every float rule is a worst-case bound per output element, not a norm: a float32 sum of Kd products, each operand exactly the float32
value the kernel read, is within gamma_Kd * sum_k |a_k| |b_k| of the exact sum (gamma_n = n u / (1 - n u), u = 2^-24), whatever the
summation order.  The checks allow c * (Kd + 4) * u * sum |a||b| (the + 4 covers the few roundings of the element-wise stages around the
GEMMs: the steering product, the float32 cos / sin tables, the phase factor), so they cannot flake, yet a missing, doubled or misplaced
reduction term is far outside them wherever that term is not tiny -- which is why the stage tests scale the Nyquist row and the last
reduction index by 100.
"""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53


def gemm_bound(absprod, Kd, c=2.0):
    return c * (Kd + 4) * U32 * np.asarray(absprod, np.float64)


def _where(mask):
    return tuple(int(i) for i in np.argwhere(mask)[0])


def check_gemm_like(got, ref64, absprod, Kd, c=2.0, what='result'):
    """|got - ref64| <= c (Kd + 4) 2^-24 absprod elementwise; absprod = the float64 sum of |a| |b| over the reduction for each element."""
    got = np.asarray(got)
    ref64 = np.asarray(ref64)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    bad = ~np.isfinite(got)
    assert not bad.any(), '%s: %d non-finite elements (first at %s): not written?' % (what, int(bad.sum()), _where(bad))
    if np.iscomplexobj(got) or np.iscomplexobj(ref64):
        err = np.abs(got.astype(np.complex128) - ref64)
    else:
        err = np.abs(got.astype(np.float64) - ref64)
    bound = gemm_bound(absprod, Kd, c)
    bad = err > bound
    if bad.any():
        i = _where(bad)
        raise AssertionError('%s: %d elements outside the bound, first at %s: got %r, float64 %r, |err| %.3e > %.3e (Kd = %d)'
                             % (what, int(bad.sum()), i, got[i], ref64[i], err[i], bound[i], Kd))


def gemm_share(got, ref64, absprod, Kd, c=2.0):
    """The largest |got - ref64| / gemm_bound(absprod, Kd, c) over the elements (0 / 0 counts as 0, a non-finite element as inf)."""
    got = np.asarray(got)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float('inf')
    err = np.abs(got.astype(np.complex128 if np.iscomplexobj(got) or np.iscomplexobj(ref64) else np.float64) - np.asarray(ref64))
    bound = np.broadcast_to(gemm_bound(absprod, Kd, c), err.shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        share = np.where(err == 0, 0.0, err / bound)
    return float(share.max())


def report_gemm_like(got, ref64, absprod, Kd, c=2.0, what='result'):
    """check_gemm_like, which prints the worst share of its bar before it asserts -> that share."""
    share = gemm_share(got, ref64, absprod, Kd, c)
    print('%s: worst share of the bar (%d * 2^-24 absprod) %.4f' % (what, c * (Kd + 4), share))
    check_gemm_like(got, ref64, absprod, Kd, c, what)
    return share


def check_written(got, what='output'):
    """Every element finite: the buffers are NaN-filled before the call, so a NaN left is an element the kernel did not write."""
    bad = ~np.isfinite(np.asarray(got))
    assert not bad.any(), '%s: %d elements not written (first at %s)' % (what, int(bad.sum()), _where(bad))


def check_zero(got, what='padding'):
    """Exactly zero (the padding the geometry promises; NaN-filled before the call, so NaN here = not written)."""
    got = np.asarray(got)
    bad = got != 0
    assert not bad.any(), '%s: %d elements not zero (first at %s: %r)' % (what, int(bad.sum()), _where(bad), got[_where(bad)])


def check_mean(got, ang, what='mean_ang'):
    """float64 time mean of the device's own angular spectrogram rows: two double summations in different orders."""
    ang = np.asarray(ang, np.float64)
    T = ang.shape[-1]
    ref = np.mean(ang, axis=-1)
    bound = 4.0 * (T + 1) * U64 * np.mean(np.abs(ang), axis=-1) + 1e-300
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = ~(err <= bound)
    assert not bad.any(), '%s: %d rows off (first %s: %r vs %r)' % (what, int(bad.sum()), _where(bad), got[_where(bad)], ref[_where(bad)])


def expected_peaks(v, S):
    """The peak rule of gccnmf_pick_tdoa_peaks: strict local maxima (argrelmax, order 1: edges never, NaN never greater), the S
    largest -- among equal heights the LARGER index, i.e. the last S of a stable ascending sort -- in ascending index order,
    -1 in slots no peak fills.  -> (indexes, status 0 / 1)."""
    v = np.asarray(v, np.float64)
    i = np.arange(1, len(v) - 1)
    peaks = i[(v[i] > v[i - 1]) & (v[i] > v[i + 1])]
    keep = sorted(int(p) for p in peaks[np.argsort(v[peaks], kind='stable')[-S:]])
    status = 0 if len(keep) == S else 1
    return keep + [-1] * (S - len(keep)), status


def check_peaks(got_idx, got_status, v, S, what='peaks'):
    want, status = expected_peaks(v, S)
    assert [int(i) for i in got_idx] == want and int(got_status) == status, (what, list(got_idx), int(got_status), want, status)


def check_argmax(got, scores, what='argmax'):
    """Exactly numpy.nanargmax over the target axis (first index on ties, NaN ignored): scores (S, ..., T), got (..., T)."""
    want = np.nanargmax(np.asarray(scores), axis=0)
    bad = np.asarray(got) != want
    assert not bad.any(), '%s: %d positions differ (first at %s: %d vs %d)' % (what, int(bad.sum()), _where(bad), got[_where(bad)],
                                                                               want[_where(bad)])
