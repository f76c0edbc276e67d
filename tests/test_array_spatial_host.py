"""CPU-only checks of the M x M spatial filter of the microphone-array path (include/gccnmf_array_spatial.h): header,
ctypes table and exported symbols of libgccnmf_array_spatial.so and every argument rule of its entry points (decided before any launch,
so dummy pointers do); the restatement tests/array_spatial_restatement.py against the stereo one at M = 2 and against its own
properties in float64 at M = 3, 5, 8; the derived bars of tests/array_spatial_checks.py on NumPy's own float32 at the cells of
tests/test_gpu_array_spatial_stages.py; planted mistakes; the engine's keyword (no device needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

import array_spatial_checks as C
import array_spatial_restatement as AS
import spatial_checks as SC
import spatial_restatement as SR

HEADER = os.path.join(REPO, 'include', 'gccnmf_array_spatial.h')
SOURCE = os.path.join(REPO, 'gcc_nmf_amd', 'csrc', 'array_spatial.hip')


# ---- the library --------------------------------------------------------------------------------------------------------------------------
def declared_functions(path):
    src = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(?:int|long)\s+(gccnmf_\w+)\s*\(', src)))


def test_header_ctypes_table_and_exported_symbols_agree():
    from gcc_nmf_amd import _array, _array_spatial, _hip
    names = declared_functions(HEADER)
    assert names == sorted(_array_spatial.SIGNATURES) and len(names) == 3
    handle = ctypes.CDLL(_array_spatial.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), n
    image = open(_array_spatial.LIB_PATH, 'rb').read()
    exported = set(m.decode() for m in re.findall(rb'gccnmf_array_\w+', image))
    assert exported == set(names), 'libgccnmf_array_spatial.so carries other gccnmf_array_ names than its header declares: %s' % sorted(exported ^ set(names))
    assert b'gccnmf_set_tuning' not in image and b'gccnmf_launch_spatial' not in image, 'nothing from the separation library'
    assert not set(names) & (set(_hip.SIGNATURES) | set(_array.SIGNATURES)), 'the other two ABIs stay as they are'
    assert _array_spatial.lib().gccnmf_array_spatial_version() >= 100
    src = open(HEADER).read()
    for macro, value in (('MIN_CHANNELS', _array_spatial.MIN_CHANNELS), ('MAX_CHANNELS', _array_spatial.MAX_CHANNELS),
                         ('MAX_TARGETS', _array_spatial.MAX_TARGETS)):
        assert int(re.search(r'#define GCCNMF_ARRAY_SPATIAL_%s (\d+)' % macro, src).group(1)) == value
    assert (_array_spatial.MIN_CHANNELS, _array_spatial.MAX_CHANNELS, _array_spatial.MAX_TARGETS) == (_array.MIN_CHANNELS, _array.MAX_CHANNELS,
                                                                                                    _array.MAX_TARGETS)


def test_the_loading_is_the_stereo_headers():
    from gcc_nmf_amd import _array_spatial
    mine = re.search(r'#define GCCNMF_ARRAY_SPATIAL_LOADING (\S+)', open(HEADER).read()).group(1)
    stereo = re.search(r'#define GCCNMF_SPATIAL_LOADING (\S+)', open(os.path.join(REPO, 'include', 'gccnmf_hip.h')).read()).group(1)
    assert float(mine) == float(stereo) == _array_spatial.LOADING == AS.LOADING == SR.LOADING


def test_source_includes_and_build_flags():
    src = open(SOURCE).read()
    assert set(re.findall(r'#include\s+"([^"]+)"', src)) == {'common.h', 'spatial.h', '../../include/gccnmf_array_spatial.h'}
    assert not re.findall(r'#include\s+<', src)
    make = open(os.path.join(REPO, 'gcc_nmf_amd', 'csrc', 'Makefile')).read()
    rule = re.search(r'^array_spatial\.o:.*\n\t(.*)$', make, flags=re.M).group(1)
    assert '-ffp-contract=off' in rule
    assert re.search(r'^all:.*\$\(ARRAY_SPATIAL_OUT\)', make, flags=re.M) and 'libgccnmf_array_spatial.so' in re.search(r'^clean:\n\t(.*)$', make, flags=re.M).group(1)


ARG, UNSUPPORTED = 1, 3
PTR = 4096            # a non-null, 16-byte aligned dummy: every rule is decided before the first HIP call


def test_argument_rules():
    from gcc_nmf_amd import _array_spatial
    f = _array_spatial.lib().gccnmf_array_spatial
    ok = dict(X=PTR, M=3, F=33, T=5, S=2, batch=2, pitch=6, cov=PTR, spec=PTR)
    order = ('X', 'M', 'F', 'T', 'S', 'batch', 'pitch', 'cov', 'spec')
    call = lambda **kw: f(*[dict(ok, **kw)[k] for k in order], 0)
    for kw in (dict(X=0), dict(spec=0), dict(cov=0), dict(cov=PTR + 4), dict(cov=PTR + 8), dict(M=1), dict(M=9), dict(M=0), dict(F=1), dict(T=0),
               dict(T=-1), dict(batch=0), dict(batch=-2), dict(pitch=5), dict(pitch=0), dict(S=3)):
        assert call(**kw) == ARG, kw
    for kw in (dict(S=0), dict(S=9, pitch=27), dict(S=-1), dict(batch=21846), dict(T=(1 << 30))):
        assert call(**kw) == UNSUPPORTED, kw


def test_workspace_floats():
    from gcc_nmf_amd import _array_spatial
    from gcc_nmf_amd._hip import HipLibraryError
    f = _array_spatial.lib().gccnmf_array_spatial_workspace_floats
    assert f(2, 513, 3, 1) == 3 * 528 * 4, 'the stereo GCCNMF_RECONSTRUCT_SPATIAL_WORKSPACE_FLOATS at M = 2'
    assert f(8, 33, 8, 5) == 5 * 8 * 48 * 64 and f(3, 2, 1, 1) == 16 * 9
    assert f(8, 4097, 8, 8191) == 8191 * 8 * 4112 * 64 > 2 ** 31, 'a long'
    for bad in ((1, 33, 2, 1), (9, 33, 2, 1), (3, 1, 2, 1), (3, 33, 0, 1), (3, 33, 9, 1), (3, 33, 2, 0), (3, 33, 2, 21846)):
        assert f(*bad) == -1, bad
    assert _array_spatial.workspace_floats(4, 33, 3, 2) == 2 * 3 * 48 * 16
    with pytest.raises(HipLibraryError):
        _array_spatial.workspace_floats(9, 33, 3, 2)


def test_no_cpu_fallback_and_the_engines_keyword():
    import torch
    from gcc_nmf_amd import _array_spatial
    from gcc_nmf_amd._hip import HipLibraryError
    from gcc_nmf_amd.array import GCCNMFArrayEngine, azimuthDirections
    line = np.array([[0.0, 0, 0], [0.2, 0, 0], [0.5, 0, 0], [1.0, 0, 0]])
    kw = dict(numChannels=4, microphonePositions=line, directions=azimuthDirections(31), windowSize=256, hopSize=64)
    for bad in ('direct', 'Spatial', '', None, 1):
        with pytest.raises(ValueError):                       # before any device work: raised with or without a device
            GCCNMFArrayEngine(4096, reconstruction=bad, **kw)
    if torch.cuda.is_available():
        return                                                # (with a device the engine is exercised by the gpu tests)
    with pytest.raises(HipLibraryError):
        GCCNMFArrayEngine(4096, reconstruction='spatial', **kw)
    with pytest.raises(HipLibraryError):
        _array_spatial.require_device()


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def random_estimates(M, S, F, T, seed):
    """Estimates with an inter-channel structure (S point sources through random mixing vectors, soft time-varying masks) -> (E, X)."""
    rng = np.random.RandomState(seed)
    steer = rng.randn(S, M, F, 1) + 1j * rng.randn(S, M, F, 1)
    src = (rng.randn(S, 1, F, T) + 1j * rng.randn(S, 1, F, T)) * 10.0 ** rng.uniform(-2, 0, (S, 1, F, T))
    X = (steer * src).sum(axis=0).astype(np.complex64)
    share = rng.uniform(0.05, 1.0, (S, M, F, T))
    E = (X[None] * (share / share.sum(axis=0))).astype(np.complex64)
    return E, X


def test_pair_order_and_layout():
    from gcc_nmf_amd import _array
    for M in range(2, 9):
        assert AS.pairs(M) == _array.pairs(M)
        assert [AS.pair_index(M, a, b) for a, b in AS.pairs(M)] == list(range(M * (M - 1) // 2))
    row = np.arange(1, 10, dtype=np.float32)
    assert np.array_equal(AS.hermitian(row, 3), np.array([[1, 4 + 5j, 6 + 7j], [4 - 5j, 2, 8 + 9j], [6 - 7j, 8 - 9j, 3]], np.complex64))


def test_two_channels_are_the_stereo_restatement():
    """covariances and powers are compared as independent code.  spatial_filter hands M = 2 over to the stereo restatement (as the kernel
    hands it to spatial_frame), so that half holds by construction: it pins the delegation, nothing more."""
    for seed, (S, F, T) in enumerate([(1, 4, 1), (3, 17, 129), (8, 5, 257)]):
        E, X = random_estimates(2, S, F, T, seed)
        E[0, :, 1] = 0
        assert SC._bits(AS.covariances(E), SR.covariances(E))
        assert SC._bits(AS.covariances(E, frame_sum=SC.device_sum), SR.covariances(E, frame_sum=SC.device_sum))
        for dtype in (np.float64, np.float32):
            assert SC._bits(AS.powers(E, dtype), SR.powers(E, dtype)), 'x / 2 and 0.5 x are the same number'
            assert SC._bits(AS.spatial_filter(E, X, dtype), SR.spatial_filter(E, X, dtype))
            R = AS.covariances(E, frame_sum=SC.device_sum)
            assert SC._bits(AS.spatial_filter(E, X, dtype, R=R), SR.spatial_filter(E, X, dtype, R=R))


@pytest.mark.parametrize('M', [3, 5, 8])
def test_properties_in_float64(M):
    S, F, T = 3, 6, 70
    E, X = random_estimates(M, S, F, T, 40 + M)
    R = AS.covariances(E)
    full = AS.hermitian(R, M).astype(np.complex128)
    assert np.abs(np.trace(full, axis1=-2, axis2=-1).real - M * (1 + AS.LOADING)).max() < 4 * M * 2.0 ** -24, 'tr R_i = M'
    assert np.array_equal(full, np.conj(np.swapaxes(full, -1, -2))) and (np.linalg.eigvalsh(full) > 0).all()
    # entry (a, b) is sum_t E_a conj(E_b) / n
    Ed = E.astype(np.complex128)
    direct = np.einsum('saft,sbft->sfab', Ed, np.conj(Ed))
    direct = direct / (np.trace(direct, axis1=-2, axis2=-1).real / M)[..., None, None] + AS.LOADING * np.eye(M)
    assert np.abs(full - direct).max() < 1e-6
    out = AS.spatial_filter(E, X)
    scale = np.abs(X).max()
    assert np.abs(out.sum(axis=0) - X).max() < 1e-12 * scale, 'the targets add up to X'
    one = AS.spatial_filter(E[:1], X)
    assert np.abs(one[0] - X).max() < 1e-12 * scale, 'one target returns X'
    # permuting the channels permutes the outputs and the rows and columns of R
    perm = np.random.RandomState(M).permutation(M)
    Rp = AS.hermitian(AS.covariances(E[:, perm]), M)
    assert np.abs(Rp - AS.hermitian(R, M)[..., perm, :][..., :, perm]).max() < 1e-6
    outp = AS.spatial_filter(E[:, perm], X[perm])
    assert np.abs(outp - out[:, perm]).max() < 1e-6 * scale
    # a silent frame gives zeros; a target that is absent from a bin has R = I there
    Ez, Xz = E.copy(), X.copy()
    Ez[:, :, :, 5], Xz[:, :, 5] = 0, 0
    Ez[1, :, 2] = 0
    outz = AS.spatial_filter(Ez, Xz)
    assert not outz[:, :, :, 5].any() and np.abs(outz[0, :, :, 4]).min() > 0
    expect = np.zeros(M * M, np.float32)
    expect[:M] = np.float32(1 + AS.LOADING)
    assert np.array_equal(AS.covariances(Ez)[1, 2], expect) and not outz[1, :, 2].any()
    assert not AS.spatial_filter(Ez, Xz, np.float32)[:, :, :, 5].any()
    # a NaN in one bin stays in that bin
    En = E.copy()
    En[0, 1, 3, 7] = np.nan
    for dtype in (np.float64, np.float32):
        outn = AS.spatial_filter(En, X, dtype)
        assert np.isnan(outn[:, :, 3]).all() and not np.isnan(np.delete(outn, 3, axis=2)).any()
    # the float32 order solves the same system
    out32 = AS.spatial_filter(E, X, np.float32)
    assert np.abs(out32 - out).max() < 1e-4 * scale


def test_the_solve_of_the_header_is_a_solve():
    """ldl_solve in float64 against numpy.linalg.solve on a random positive definite matrix, and the pivots against the LDL^H of a
    Cholesky factor."""
    M = 8
    rng = np.random.RandomState(0)
    G = rng.randn(M, M) + 1j * rng.randn(M, M)
    A = G @ np.conj(G.T) + 0.1 * np.eye(M)
    x = rng.randn(M) + 1j * rng.randn(M)
    sg = [np.float64(A[a, a].real).reshape(1, 1) for a in range(M)]
    for a, b in AS.pairs(M):
        sg += [np.float64(A[a, b].real).reshape(1, 1), np.float64(A[a, b].imag).reshape(1, 1)]
    yr, yi, d = AS.ldl_solve(sg, [np.float64(v.real).reshape(1, 1) for v in x], [np.float64(v.imag).reshape(1, 1) for v in x], M)
    y = np.array([yr[k][0, 0] + 1j * yi[k][0, 0] for k in range(M)])
    assert np.abs(y - np.linalg.solve(A, x)).max() < 1e-12 * np.abs(y).max()
    assert np.allclose([v[0, 0] for v in d], np.diag(np.linalg.cholesky(A)).real ** 2, rtol=1e-12)


# ---- the bars on NumPy's own float32 ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def problems():
    """cell -> [(E, X)] per file of its batch, computed once and left unchanged."""
    out = {}
    for cell in C.CELLS:
        out[cell] = [(C.host_ratio(p, cell[1]), p[3]) for p in C.cell_files(cell)]
        for E, X in out[cell]:
            E.setflags(write=False)
            X.setflags(write=False)
    return out


def host_stages(E, X, frame_sum=SC.device_sum, loading=AS.LOADING, trace=None, **variant):
    cov = AS.covariances(E, loading=loading, frame_sum=frame_sum, trace=trace)
    return cov, AS.spatial_filter(E, X, np.float32, R=cov, **variant)


def test_the_cell_table_covers_what_it_has_to(problems):
    cells = list(C.CELLS)
    assert {c[0] for c in cells} == set(range(3, 9)), 'every M of the LDL^H kernels'
    assert {c[1] for c in cells} >= {1, 2, 3, 4, 5, 8} and {c[3] for c in cells} >= {1, 2, 127, 128, 129, 130, 257}
    options = set()
    for c in C.CELLS.values():
        options |= set(c['args'])
    assert options >= {'weak', 'absent', 'zero_frame', 'tiny_frame'}
    E, X = problems[(7, 5, 17, 127, 1)][0]
    v = AS.powers(E)
    share = v[3].sum() / v.sum()
    level = np.abs(X).max(axis=(0, 2))
    print('weak80: the weak target holds %.3g of the power; the bins span %.1f dB' % (share, 20 * np.log10(level.max() / level.min())))
    assert 1e-10 < share < 1e-6 and level.max() / level.min() > 300
    assert np.abs(AS.covariances(E)[:, :, 7:]).max() > 0.5, 'the estimates have an inter-channel structure'
    E, X = problems[(3, 3, 33, 128, 1)][0]
    assert (E[0, :, 7] == 0).all()
    E, X = problems[(6, 4, 40, 257, 1)][0]
    assert (X[:, :, 130] == 0).all() and 1e-11 < np.abs(X[:, :, 11]).max() < 1e-9


@pytest.mark.parametrize('cell', list(C.CELLS), ids=['M%d-S%d-F%d-T%d-b%d' % c for c in C.CELLS])
def test_the_float32_restatement_passes_every_bar(problems, cell):
    """The float32 restatement (the device's order) lies within bar_filter_M of the float64 one (numpy.linalg.solve) at every element
    of every cell, its device-order covariances within one float32 ulp of the ascending ones.  Elements behind a failed guard, of the
    non-zero finite elements, per cell in table order: 0 of 408, 0 of 40, 0 of 305712 (three files), 0 of 491520, 0 of 151130, 0 of
    532032 (two files), 0 of 75264 -- the cap is 0.1 %."""
    behind = total = 0
    for b, (E, X) in enumerate(problems[cell]):
        cov, out = host_stages(E, X)
        fail, bits, share, (n, g, _) = C.check_cell(E, X, cov, out, '%s[%d]' % (cell, b))
        print('%s[%d]: largest share of a bar: %s; %d of %d elements behind a failed guard' %
              (cell, b, ', '.join('%s %.4f' % kv for kv in sorted(share.items())), g, n))
        assert not fail, fail
        assert not bits, bits
        behind, total = behind + g, total + n
    assert behind <= C.GUARD_CAP * total


def test_the_bars_evaluation_is_the_contract(problems):
    """The values carried inside bar_filter_M (the header's order in float64) against numpy.linalg.solve, and the bar relative to the
    element: the same for the weak target as for the others."""
    cell = (7, 5, 17, 127, 1)
    E, X = problems[cell][0]
    cov = AS.covariances(E, frame_sum=SC.device_sum)
    ref = AS.spatial_filter(E, X, np.float64, R=cov)
    bar_re, bar_im, ok, value = C.bar_filter_M(C.q_powers(E), cov, X)
    assert ok.all()
    assert np.allclose(value, ref, rtol=1e-6, atol=1e-9 * np.abs(ref).max())
    rel = np.hypot(bar_re, bar_im) / np.abs(ref)
    med = [float(np.median(rel[i])) for i in range(5)]
    print('weak80: median bar / |reference| per target %s' % ['%.3g' % m for m in med])
    assert med[3] < 4 * max(med[:3] + med[4:])


# mistake -> (cell, what must see it: 'bars' = a failure under the bars, 'bits' = the bit comparison alone)
PLANTED = {
    'conjugate':  ((4, 3, 33, 129, 3), 'bars'),     # R_ba taken for R_ab: the stored imaginary parts negated, in the filter
    'trace_2':    ((4, 3, 33, 129, 3), 'bars'),     # the trace normalised to 2 instead of M
    'no_loading': ((3, 3, 33, 128, 1), 'bars'),     # R, not R~
    'pair_order': ((4, 3, 33, 129, 3), 'bars'),     # the pairs in another order: (0, 2) before (0, 1)
    'drop_sigma': ((4, 3, 33, 129, 3), 'bars'),     # Sigma_w without one target
    'drop_sigma_M6': ((6, 4, 40, 257, 1), 'bars'),  # the same at six microphones, where the float32 restatement uses 3e-4 of a bar
    'conjugate_M8': ((8, 8, 17, 130, 2), 'bars'),   # R_ba for R_ab at eight
    'drop128':    ((4, 3, 33, 129, 3), 'bars'),     # frames >= 128 dropped from the covariance sums
    'power_2':    ((3, 3, 33, 128, 1), 'bits'),     # the powers divided by 2 instead of M
}


@pytest.mark.parametrize('mistake', sorted(PLANTED))
def test_planted_mistakes_fail(problems, mistake):
    """Each mistake, planted in the float32 restatement, fails check_cell -- the function the device test calls.  power_2 is seen by the
    bit comparison alone, and that is all there is to see: a common factor of the powers cancels in w_i R~_i Sigma_w^-1 X (exactly, bit
    for bit, where M / 2 is a power of two: the reason the cell has M = 3), so only the roundings move."""
    cell, seen_by = PLANTED[mistake]
    E, X = problems[cell][C.CELLS[cell]['pos']]
    cov, out = host_stages(E, X)
    fail, bits, _, _ = C.check_cell(E, X, cov, out, 'as it should be')
    assert not fail and not bits
    M = cell[0]
    if mistake.startswith('conjugate'):
        wrong = cov.copy()
        wrong[:, :, M + 1::2] *= -1
        out = AS.spatial_filter(E, X, np.float32, R=wrong)
    elif mistake == 'trace_2':
        cov, out = host_stages(E, X, trace=2)
    elif mistake == 'no_loading':
        cov, out = host_stages(E, X, loading=0.0)
    elif mistake == 'pair_order':
        cov = cov.copy()
        cov[:, :, M:M + 4] = cov[:, :, [M + 2, M + 3, M, M + 1]]
        out = AS.spatial_filter(E, X, np.float32, R=cov)
    elif mistake.startswith('drop_sigma'):
        out = AS.spatial_filter(E, X, np.float32, R=cov, without=1)
    elif mistake == 'drop128':
        cov, out = host_stages(E, X, frame_sum=lambda x: SC.device_sum(np.asarray(x)[..., :128]))
    elif mistake == 'power_2':
        out = AS.spatial_filter(E, X, np.float32, R=cov, divisor=2)
    fail, bits, share, _ = C.check_cell(E, X, cov, out, mistake)
    print('%s on %s: %d failures under the bars (up to %.3g of a bar), %d stages with other bits' %
          (mistake, cell, len(fail), max(share.values()), len(bits)))
    assert bits, mistake
    if seen_by == 'bars':
        assert any('of the bar' in f for f in fail), (mistake, fail)
    else:
        assert not fail


# ---- where the pivots' guards give up: the normwise bar ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def line_problem():
    """Three talkers in front of an eight-microphone LINE (structured(line=True)): the regime of the engine case (M, batch, S) =
    (8, 2, 3) of tests/test_gpu_array_spatial_engine.py, without a device."""
    p = C.structured(8, 33, 61, 3, 77, line=True)
    E, X = C.host_ratio(p, 3), p[3]
    E.setflags(write=False)
    X.setflags(write=False)
    return E, X


def test_a_line_array_at_eight_microphones_is_held_by_the_normwise_bar(line_problem):
    """Sigma_w is well conditioned there (pivots >= 5e-4 against a perturbation near 4e-6); what gives up is the running bound of
    bar_filter_M, which grows by 1 / d_k at each of the five small pivots: 94416 of 96624 elements behind a failed guard.  Every one of
    them is held by normwise_filter -- the float32 restatement (the device's order) against numpy.linalg.solve under a bound from the
    backward error of the solve and the measured condition of Sigma_w -- and by the residual of the sum of the targets: no element is
    left without a float64 check."""
    E, X = line_problem
    cov, out = host_stages(E, X)
    fail, bits, share, (n, behind, unchecked) = C.check_cell(E, X, cov, out, 'line')
    print('line, M = 8, S = 3: %d of %d behind a failed pivot guard, %d without any float64 check; shares: %s' %
          (behind, n, unchecked, ', '.join('%s %.2e' % kv for kv in sorted(share.items()))))
    assert not fail and not bits
    assert behind > 0.5 * n, 'the regime the test is for'
    assert unchecked == 0
    nshare, rshare, checked, live = C.normwise_filter(E, cov, X, out)
    assert checked.all() and live.all()
    # the distance itself, for the record: float32 in the header's order against float64, relative to the frame's |X|
    ref = AS.spatial_filter(E, X, np.float64, R=cov)
    rel = np.abs(out - ref).max(axis=(0, 1)) / np.abs(X).max(axis=0)
    print('  float32 order against float64: at most %.2e of the frame\'s max |X|' % rel.max())
    assert rel.max() < 1e-4


@pytest.mark.parametrize('mistake', ['drop_sigma', 'conjugate', 'no_loading'])
def test_the_normwise_bar_sees_planted_mistakes_where_the_guards_fail(line_problem, mistake):
    """A target left out of Sigma_w and R_ba for R_ab are outside the normwise bar.  A filter run on covariances without the loading is
    not: 0.16 of the bar (kappa times the backward error is a loose bound for a change of 1e-3 in the smallest eigenvalues); the
    covariance launch's own check -- one ulp against the ascending sums, no guard involved -- is what sees that one."""
    E, X = line_problem
    cov, out = host_stages(E, X)
    if mistake == 'drop_sigma':
        out = AS.spatial_filter(E, X, np.float32, R=cov, without=1)
    elif mistake == 'conjugate':
        wrong = cov.copy()
        wrong[:, :, 9::2] *= -1
        out = AS.spatial_filter(E, X, np.float32, R=wrong)
    else:
        out = AS.spatial_filter(E, X, np.float32, R=AS.covariances(E, loading=0.0, frame_sum=SC.device_sum))
    nshare, rshare, checked, _ = C.normwise_filter(E, cov, X, out)
    print('%s: %.3g of the normwise bar, %.3g of the residual bar' % (mistake, nshare.max(), rshare.max()))
    assert checked.all()
    if mistake == 'no_loading':
        fail = C.check_cell(E, X, AS.covariances(E, loading=0.0, frame_sum=SC.device_sum), out, mistake)[0]
        assert nshare.max() < 1 and any('covariance launch' in f for f in fail)
    else:
        assert nshare.max() > 1 or rshare.max() > 1
