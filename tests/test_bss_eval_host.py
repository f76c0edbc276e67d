"""CPU-only checks of the scoring feature: the float64 restatement of the BSS Eval image criteria
(tests/bss_eval_restatement.py) is pinned by identities that hold for any correct implementation, on random inputs; the argument rules
of gcc_nmf_amd.evaluation.bss_eval_images; header, ctypes table and exported symbols of libgccnmf_eval.so name by name; every argument
rule of its C entry points (decided before any launch, so dummy pointers do); and no CPU fallback."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from conftest import REPO

import bss_eval_restatement as R

HEADER = os.path.join(REPO, 'include', 'gccnmf_eval.h')
SHAPES = R.SHAPES[:7]
IDS = ['J%d-C%d-n%d-L%d' % s for s in SHAPES]


@pytest.mark.parametrize('shape', SHAPES[:2] + SHAPES[3:], ids=IDS[:2] + IDS[3:])
def test_the_four_error_terms_add_up_and_the_artefact_is_orthogonal(shape):
    """s + e_spat + e_interf + e_artif == e to rounding, and e_artif is orthogonal to every delayed reference: normalised inner products
    below 1e-12 (the prototype gave 4e-14)."""
    J, C, n, L = shape
    s, e = R.make_case(*shape, seed=3)
    P_all, P_i, cond = R.decompose(s, e, L)
    assert cond < 1e3
    sp, ep, D = R.pad(s, L), R.pad(e, L), R.delayed(s.astype(np.float64), L)
    for j in range(J):
        for i in range(J):
            e_spat, e_interf, e_artif = P_i[j, i] - sp[i], P_all[j] - P_i[j, i], ep[j] - P_all[j]
            total = sp[i] + e_spat + e_interf + e_artif
            assert np.abs(total - ep[j]).max() <= 8 * np.finfo(np.float64).eps * np.abs(ep[j]).max()
            for c in range(C):
                inner = D @ e_artif[c]
                norm = np.linalg.norm(D, axis=1) * np.linalg.norm(e_artif[c])
                assert (np.abs(inner) / norm).max() < 1e-12
            # e_spat lies in the span of source i's delayed images minus s_i; e_interf in the span of all of them
            rows = slice(i * C * L, (i + 1) * C * L)
            for c in range(C):
                coef = np.linalg.lstsq(D[rows].T, P_i[j, i, c], rcond=None)[0]
                assert np.abs(D[rows].T @ coef - P_i[j, i, c]).max() < 1e-9 * max(1.0, np.abs(P_i[j, i, c]).max())


@pytest.mark.parametrize('shape', SHAPES[:2], ids=IDS[:2])
def test_sdr_is_the_plain_energy_ratio(shape):
    s, e = R.make_case(*shape, seed=4)
    sdr = R.bss_eval_images(s, e, shape[3], computePermutation=False)[0]
    s64, e64 = s.astype(np.float64), e.astype(np.float64)
    for i in range(shape[0]):
        want = 10 * np.log10(np.sum(s64[i] ** 2) / np.sum((e64[i] - s64[i]) ** 2))
        assert abs(sdr[i] - want) < 1e-10


def test_a_perfect_estimate_scores_above_150_db():
    s, _ = R.make_case(3, 2, 600, 8, seed=5)
    for v in R.bss_eval_images(s, s.copy(), 8)[:4]:
        assert ((v > 150) | np.isposinf(v)).all(), v


def test_one_source_has_infinite_sir():
    s, e = R.make_case(1, 2, 257, 8, seed=6)
    sdr, isr, sir, sar, perm = R.bss_eval_images(s, e, 8)
    assert np.isposinf(sir).all() and np.isfinite(sdr).all() and np.isfinite(isr).all() and np.isfinite(sar).all() and perm.tolist() == [0]


def test_a_shuffled_estimate_order_is_recovered_by_perm():
    s, e = R.make_case(3, 2, 800, 8, seed=7)
    base = R.bss_eval_images(s, e, 8)
    assert base[4].tolist() == [0, 1, 2]
    for order in ([2, 0, 1], [1, 0, 2], [2, 1, 0]):
        shuffled = e[order]                                   # estimate k is true source order[k]
        got = R.bss_eval_images(s, shuffled, 8)
        assert got[4].tolist() == np.argsort(order).tolist()  # estimate perm[j] is true source j
        for a, b in zip(got[:4], base[:4]):
            assert np.allclose(a, b, rtol=0, atol=1e-9)


def test_two_float64_evaluations_agree_within_a_tenth_of_the_device_tolerance_budget():
    """The dB tolerance of the device tests (R.DB_TOLERANCE) is 10 x the largest disagreement, over the GPU tests' inputs, between float64
    evaluations of the restatement that differ in solver (Cholesky, LU, least squares) and summation order (forward, reversed).  Here the
    disagreement is measured again and has to stay inside the tolerance itself; the measured value is in DESIGN section 4i."""
    worst = 0.0
    for L, s, e in R.all_test_files():
        a = R.all_pairs(s, e, L, 'cholesky', 'forward')
        assert a[4] < 1e3, (s.shape, L, a[4])
        for other in (R.all_pairs(s, e, L, 'lu', 'reversed'), R.all_pairs(s, e, L, 'lstsq', 'forward')):
            for x, y in zip(a[:4], other[:4]):
                m = np.isfinite(x)
                assert (np.isfinite(y) == m).all()
                worst = max(worst, float(np.abs(x[m] - y[m]).max(initial=0.0)))
    print('largest disagreement between float64 evaluations: %.3e dB (tolerance %.1e dB)' % (worst, R.DB_TOLERANCE))
    assert worst <= R.DB_TOLERANCE <= 1e-6


def test_the_bars_hold_for_float64_numpy_sums():
    """The two derived bars hold for any summation order: NumPy's own float64 sums sit inside them."""
    s, e = R.make_case(2, 2, 300, 5, seed=8)
    A, B = s.reshape(4, 300), e.reshape(4, 300)
    exact, bar = R.lag_correlations_exact(A, B, 5)
    a64, b64 = A.astype(np.float64), B.astype(np.float64)
    for l in range(-4, 5):
        lo, hi = max(0, -l), min(300, 300 - l)
        got = np.einsum('an,bn->ab', a64[:, lo:hi], b64[:, lo + l:hi + l])
        assert (np.abs(got - exact[:, :, l + 4]) <= bar[:, :, l + 4]).all()
    coef = np.random.default_rng(9).standard_normal((3, 4, 5))
    ranges = np.array([[0, 4], [0, 2], [2, 2]])
    ref, pbar = R.projections_reference(A, coef, ranges)
    got = np.zeros((3, 304))
    for q in range(3):
        for a in range(ranges[q, 0], ranges[q, 0] + ranges[q, 1]):
            got[q] += np.convolve(coef[q, a], a64[a])
    assert (np.abs(got - ref.astype(np.float64)) <= pbar).all() and (pbar[:, 4:300] > 0).all()


# ---- the public function's argument rules: ValueError before a device is looked for ------------------------------------------------------
def test_bss_eval_images_argument_rules():
    from gcc_nmf_amd.evaluation import bss_eval_images, check_images
    z = lambda *shape: np.ones(shape, np.float32)
    with pytest.raises(ValueError, match='same shape'):
        bss_eval_images(z(2, 2, 300), z(2, 2, 301), 5)
    with pytest.raises(ValueError, match='shape'):
        bss_eval_images(z(2, 300), z(2, 300), 5)
    with pytest.raises(ValueError, match='at most 8 sources'):
        bss_eval_images(z(9, 2, 3000), z(9, 2, 3000), 5)
    with pytest.raises(ValueError, match='channels'):
        bss_eval_images(z(2, 3, 300), z(2, 3, 300), 5)
    for L in (0, -1, 2.5, True, 4097, None):
        with pytest.raises(ValueError, match='filterLength'):
            bss_eval_images(z(2, 2, 300), z(2, 2, 300), L)
    with pytest.raises(ValueError, match='singular by construction'):
        bss_eval_images(z(3, 2, 2560), z(3, 2, 2560), 512)           # 3072 taps, 3071 samples
    check_images(z(3, 2, 2562), z(3, 2, 2562), 512)                  # 3072 taps, 3073 samples: accepted
    for bad in (np.nan, np.inf):
        x = z(2, 2, 300)
        x[1, 0, 7] = bad
        with pytest.raises(ValueError, match='finite'):
            bss_eval_images(x, z(2, 2, 300), 5)
        with pytest.raises(ValueError, match='finite'):
            bss_eval_images(z(1, 2, 2, 300), x[None], 5)
    s, e, batched = check_images(np.ones((2, 2, 300)), np.ones((2, 2, 300)), 5)
    assert s.shape == e.shape == (1, 2, 2, 300) and s.dtype == e.dtype == np.float32 and not batched
    assert check_images(z(4, 2, 1, 300), z(4, 2, 1, 300), 5)[2]


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a device is present')
    from gcc_nmf_amd import _eval
    from gcc_nmf_amd._hip import HipLibraryError
    from gcc_nmf_amd.evaluation import bss_eval_images
    s, e = R.make_case(2, 2, 300, 5)
    with pytest.raises(HipLibraryError):
        bss_eval_images(s, e, 5)
    with pytest.raises(HipLibraryError):
        _eval.require_device()


# ---- the library ----------------------------------------------------------------------------------------------------------------------------
def declared_functions():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(?:int|long)\s+(gccnmf_\w+)\s*\(', src)))


def test_header_ctypes_table_and_exported_symbols_agree():
    from gcc_nmf_amd import _eval, _hip
    names = declared_functions()
    assert names == sorted(_eval.SIGNATURES) and len(names) == 4
    handle = ctypes.CDLL(_eval.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), n
    exported = set(m.decode() for m in re.findall(rb'gccnmf_eval_\w+', open(_eval.LIB_PATH, 'rb').read()))
    assert exported == set(names), 'libgccnmf_eval.so carries other gccnmf_eval_ names than its header declares: %s' % sorted(exported ^ set(names))
    assert b'gccnmf_set_tuning' not in open(_eval.LIB_PATH, 'rb').read(), 'the scoring library takes nothing from the separation library'
    assert not set(names) & set(_hip.SIGNATURES), 'the separation ABI stays as it is'
    assert _eval.lib().gccnmf_eval_version() >= 100
    src = open(HEADER).read()
    assert int(re.search(r'#define GCCNMF_EVAL_SYMMETRIC (\d+)', src).group(1)) == _eval.GCCNMF_EVAL_SYMMETRIC
    assert int(re.search(r'#define GCCNMF_EVAL_BLOCK (\d+)', src).group(1)) == _eval.GCCNMF_EVAL_BLOCK
    for code, name in ((0, 'GCCNMF_OK'), (1, 'GCCNMF_ERR_ARG'), (2, 'GCCNMF_ERR_LAUNCH'), (3, 'GCCNMF_ERR_UNSUPPORTED')):
        assert int(re.search(r'#define %s (\d+)' % name, src).group(1)) == code and _hip.STATUS[code].startswith(name)


P, Q2 = 0x10000, 0x20000          # dummy device pointers, 16-byte aligned: every call below is rejected before anything is launched
ARG, UNSUPPORTED = 1, 3


def test_workspace_bytes_in_closed_form_and_its_argument_rules():
    from gcc_nmf_amd import _eval
    lib = _eval.lib()
    w = lib.gccnmf_eval_workspace_bytes
    assert w(6, 6, 160000, 512, 64) == 64 * 36 * 157 * 1023 * 8
    assert w(4, 4, 1024, 5, 1) == 16 * 1 * 9 * 8 and w(4, 4, 1025, 5, 1) == 16 * 2 * 9 * 8 and w(1, 2, 1, 1, 3) == 3 * 2 * 1 * 1 * 8
    assert w(6, 6, 2000, 4096, 1) == 36 * 2 * 8191 * 8
    for bad in ((0, 6, 100, 5, 1), (6, 0, 100, 5, 1), (6, 6, 0, 5, 1), (6, 6, 100, 0, 1), (6, 6, 100, 4097, 1), (6, 6, 100, 5, 0),
                (6, 6, 100, 5, 65536), (6, 6, -1, 5, 1), (256, 256, 100, 5, 1), (100, 100, 100, 4096, 1), (6, 6, 2 ** 31 - 1, 5, 1)):
        assert w(*bad) == -1, bad
    with pytest.raises(_eval.HipLibraryError):
        _eval.workspace_bytes(6, 6, 100, 0, 1)


def test_lag_correlations_argument_rules():
    from gcc_nmf_amd import _eval
    f = _eval.lib().gccnmf_eval_lag_correlations
    ok = dict(A=P, B=Q2, Ma=6, Mb=6, n=1000, L=16, batch=2, flags=0, ws=P, R=P)
    call = lambda **kw: f(*[dict(ok, **kw)[k] for k in ('A', 'B', 'Ma', 'Mb', 'n', 'L', 'batch', 'flags', 'ws', 'R')], 0)
    for kw in (dict(L=0), dict(L=-3), dict(L=4097), dict(Ma=0), dict(Mb=0), dict(Ma=-1), dict(n=0), dict(n=-5), dict(batch=0), dict(batch=-1),
               dict(A=0), dict(B=0), dict(ws=0), dict(R=0), dict(A=P + 4), dict(B=P + 8), dict(ws=P + 8), dict(R=P + 8),
               dict(flags=2), dict(flags=-1), dict(flags=1), dict(flags=1, B=P, Mb=5)):
        assert call(**kw) == ARG, kw
    for kw in (dict(batch=65536), dict(Ma=256, Mb=256), dict(Ma=100, Mb=100, L=4096), dict(n=2 ** 31 - 1)):
        assert call(**kw) == UNSUPPORTED, kw


def test_project_argument_rules():
    from gcc_nmf_amd import _eval
    f = _eval.lib().gccnmf_eval_project
    ok = dict(A=P, coef=Q2, ranges=P, Ma=6, Q=24, n=1000, L=16, batch=2, P=P)
    call = lambda **kw: f(*[dict(ok, **kw)[k] for k in ('A', 'coef', 'ranges', 'Ma', 'Q', 'n', 'L', 'batch', 'P')], 0)
    for kw in (dict(L=0), dict(L=4097), dict(Ma=0), dict(Q=0), dict(Q=-2), dict(n=0), dict(batch=0), dict(A=0), dict(coef=0), dict(ranges=0),
               dict(P=0), dict(A=P + 4), dict(coef=P + 8), dict(ranges=P + 4), dict(P=P + 8)):
        assert call(**kw) == ARG, kw
    for kw in (dict(batch=65536), dict(Q=65536), dict(n=2 ** 31 - 1)):
        assert call(**kw) == UNSUPPORTED, kw


def test_the_wrappers_reject_what_the_library_rejects_without_a_device():
    """_eval's own functions check shapes and dtypes before they call the library: the status of a rejected call is a HipLibraryError."""
    import torch
    from gcc_nmf_amd import _eval
    A = torch.zeros((1, 2, 100), dtype=torch.float32)
    with pytest.raises(_eval.HipLibraryError):
        _eval.lag_correlations(A, A, 0)                      # L = 0: gccnmf_eval_workspace_bytes says -1
    with pytest.raises(AssertionError):
        _eval.lag_correlations(A.double(), A.double(), 4)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert _eval.workspace_bytes(2, 2, 100, 4, 1) == 4 * 7 * 8
