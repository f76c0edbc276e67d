"""CPU-only checks of the EM refinement of the M x M spatial filter of the microphone-array path (DESIGN section 4j;
include/gccnmf_array_em.h): header, ctypes table and exported symbols of libgccnmf_array_em.so and every argument rule of its entry points
(decided before any launch, so dummy pointers do); the restatement tests/array_em_restatement.py against the stereo one at M = 2 and
against the definition as written (numpy.linalg.inv) at M = 3, 5, 8; planted mistakes; the engine's keyword (no device needed); the
condition the measured bars of tests/test_gpu_array_em_stages.py rest on, at every one of its cells."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

import array_em_restatement as AE
import array_spatial_checks as C
import array_spatial_restatement as AS
import spatial_checks as SC
import spatial_em_restatement as EM
import spatial_restatement as SR
from test_array_spatial_host import ARG, UNSUPPORTED, PTR, declared_functions, random_estimates

HEADER = os.path.join(REPO, 'include', 'gccnmf_array_em.h')
SOURCE = os.path.join(REPO, 'gcc_nmf_amd', 'csrc', 'array_spatial_em.hip')


# ---- the library --------------------------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_exported_symbols_agree():
    from gcc_nmf_amd import _array, _array_em, _array_spatial, _hip
    names = declared_functions(HEADER)
    assert names == sorted(_array_em.SIGNATURES) and len(names) == 3
    handle = ctypes.CDLL(_array_em.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), n
    image = open(_array_em.LIB_PATH, 'rb').read()
    exported = set(m.decode() for m in re.findall(rb'gccnmf_array_\w+', image))
    assert exported == set(names), 'libgccnmf_array_em.so carries other gccnmf_array_ names than its header declares: %s' % sorted(exported ^ set(names))
    assert b'gccnmf_set_tuning' not in image and b'gccnmf_launch_spatial' not in image, 'nothing from the separation library'
    assert not set(names) & (set(_hip.SIGNATURES) | set(_array.SIGNATURES) | set(_array_spatial.SIGNATURES)), 'the other ABIs stay as they are'
    assert _array_em.lib().gccnmf_array_em_version() >= 100
    assert int(re.search(r'#define GCCNMF_ARRAY_EM_MAX_ITERATIONS (\d+)', open(HEADER).read()).group(1)) == _array_em.MAX_ITERATIONS == \
        _hip.MAX_SPATIAL_ITERATIONS
    old = open(_array_spatial.LIB_PATH, 'rb').read()
    assert b'gccnmf_array_em' not in old, 'the filter library knows nothing of this one'


def test_source_reuses_the_filter_librarys_kernels_and_build_flags():
    src = open(SOURCE).read()
    assert set(re.findall(r'#include\s+"([^"]+)"', src)) == {'array_spatial.hip', '../../include/gccnmf_array_em.h'}
    assert not re.findall(r'#include\s+<', src)
    assert set(re.findall(r'__global__\s+__launch_bounds__\([^)]*\)\s+void\s+(\w+)', src)) == {'array_em2_kernel', 'array_em_kernel'}, 'the two other kernels are not copied'
    assert 'array_spatial_cov_launch<M>' in src and 'array_spatial_filter_dispatch<M, true>' in src, '... but launched through array_spatial.hip'
    make = open(os.path.join(REPO, 'gcc_nmf_amd', 'csrc', 'Makefile')).read()
    rule = re.search(r'^array_spatial_em\.o:.*\n\t(.*)$', make, flags=re.M).group(1)
    assert '-ffp-contract=off' in rule
    assert re.search(r'^all:.*\$\(ARRAY_EM_OUT\)', make, flags=re.M) and 'libgccnmf_array_em.so' in re.search(r'^clean:\n\t(.*)$', make, flags=re.M).group(1)
    for path in ('README.md', os.path.join('include', 'gccnmf_array_spatial.h')):
        assert 'no M-channel form yet' not in open(os.path.join(REPO, path)).read(), path


def test_argument_rules():
    from gcc_nmf_amd import _array_em
    f = _array_em.lib().gccnmf_array_em
    ok = dict(X=PTR, M=3, F=33, T=5, S=2, batch=2, pitch=6, n=1, ws=PTR, spec=PTR)
    order = ('X', 'M', 'F', 'T', 'S', 'batch', 'pitch', 'n', 'ws', 'spec')
    call = lambda **kw: f(*[dict(ok, **kw)[k] for k in order], 0)
    # the rules of gccnmf_array_spatial, the workspace in the place of cov
    for kw in (dict(X=0), dict(spec=0), dict(ws=0), dict(ws=PTR + 4), dict(ws=PTR + 8), dict(M=1), dict(M=9), dict(M=0), dict(F=1), dict(T=0),
               dict(T=-1), dict(batch=0), dict(batch=-2), dict(pitch=5), dict(pitch=0), dict(S=3)):
        assert call(**kw) == ARG, kw
    for kw in (dict(S=0), dict(S=9, pitch=27), dict(S=-1), dict(batch=21846), dict(T=(1 << 30))):
        assert call(**kw) == UNSUPPORTED, kw
    # n outside 1..255
    for n in (0, -1, 256, 1 << 20):
        assert call(n=n) == UNSUPPORTED, n
    assert call(n=0, X=0) == ARG, 'an argument error comes first'


def test_workspace_floats():
    from gcc_nmf_amd import _array_em, _array_spatial
    from gcc_nmf_amd._hip import HipLibraryError, reconstruct_spatial_em_workspace_floats
    f = _array_em.lib().gccnmf_array_em_workspace_floats
    assert f(2, 513, 626, 3, 1) == 3 * 528 * 4 + 3 * 528 * 640 == reconstruct_spatial_em_workspace_floats(1, 3, 528, 640), 'the stereo workspace at M = 2'
    assert f(8, 33, 65, 8, 5) == 5 * 8 * 48 * 64 + 5 * 8 * 48 * 128 and f(3, 2, 1, 1, 1) == 16 * 9 + 16 * 64
    assert f(8, 4097, 1, 8, 8191) == 8191 * 8 * 4112 * (64 + 64) > 2 ** 31, 'a long'
    for M, F, T, S, B in ((4, 33, 5, 3, 2), (6, 17, 64, 1, 1), (3, 16, 129, 8, 3)):
        assert f(M, F, T, S, B) == _array_spatial.workspace_floats(M, F, S, B) + B * S * -(-F // 16) * 16 * -(-T // 64) * 64
    for bad in ((1, 33, 5, 2, 1), (9, 33, 5, 2, 1), (3, 1, 5, 2, 1), (3, 33, 5, 0, 1), (3, 33, 5, 9, 1), (3, 33, 5, 2, 0), (3, 33, 5, 2, 21846),
                (3, 33, 0, 2, 1), (3, 33, -1, 2, 1), (3, 33, 1 << 30, 2, 1)):
        assert f(*bad) == -1, bad
    assert _array_em.workspace_floats(4, 33, 5, 3, 2) == 2 * 3 * 48 * (16 + 64)
    with pytest.raises(HipLibraryError):
        _array_em.workspace_floats(9, 33, 5, 3, 2)


def test_the_engines_keyword():
    import torch
    from gcc_nmf_amd import _array_em
    from gcc_nmf_amd._hip import HipLibraryError
    from gcc_nmf_amd.array import GCCNMFArrayEngine, azimuthDirections
    line = np.array([[0.0, 0, 0], [0.2, 0, 0], [0.5, 0, 0], [1.0, 0, 0]])
    kw = dict(numChannels=4, microphonePositions=line, directions=azimuthDirections(31), windowSize=256, hopSize=64)
    for bad in (-1, 256, 1.0, '2', None, True):
        with pytest.raises(ValueError):                       # before any device work: raised with or without a device
            GCCNMFArrayEngine(4096, reconstruction='spatial', spatialIterations=bad, **kw)
    with pytest.raises(ValueError):
        GCCNMFArrayEngine(4096, reconstruction='ratio', spatialIterations=2, **kw)
    with pytest.raises(ValueError):
        GCCNMFArrayEngine(4096, spatialIterations=1, **kw)    # the default reconstruction is 'ratio'
    if torch.cuda.is_available():
        return                                                # (with a device the engine is exercised by the gpu tests)
    with pytest.raises(HipLibraryError):
        GCCNMFArrayEngine(4096, reconstruction='spatial', spatialIterations=2, **kw)
    with pytest.raises(HipLibraryError):
        _array_em.require_device()


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def test_two_channels_are_the_stereo_restatement():
    for seed, (S, F, T) in enumerate([(1, 4, 1), (3, 17, 129), (8, 5, 257)]):
        E, X = random_estimates(2, S, F, T, seed)
        E[0, :, 1] = 0
        for dtype in (np.float64, np.float32):
            v, R = SR.powers(E, dtype), SR.covariances(E)
            stereo = EM.em_step(v, R, X, dtype, frame_sum=SC.device_sum if dtype == np.float32 else None)
            mine = AE.em_step(AS.powers(E, dtype), AS.covariances(E), X, dtype)
            assert SC._bits(mine[0], stereo[0]) and SC._bits(mine[1], stereo[1])
            assert SC._bits(AE.filter_with(mine[0], mine[1], X, dtype), EM.filter_with(stereo[0], stereo[1], X, dtype))
            v2, R2 = AE.refine(E, X, 2, dtype)
            v2s, R2s = EM.refine(E, X, 2, dtype, frame_sum=SC.device_sum) if dtype == np.float32 else EM.refine(E, X, 2, dtype)
            if dtype == np.float64:                           # (float32 starts from the covariances in the device's order)
                assert SC._bits(v2, v2s) and SC._bits(R2, R2s)
                assert SC._bits(AE.array_em(E, X, 2), EM.spatial_em(E, X, 2))
        assert SC._bits(AE.array_em(E, X, 0, np.float32), SR.spatial_filter(E, X, np.float32))


def _loaded(Rl, M, loading='trace'):
    tr = np.trace(Rl, axis1=-2, axis2=-1).real / M
    return Rl + (AS.LOADING * tr if loading == 'trace' else AS.LOADING * np.ones_like(tr))[..., None, None] * np.eye(M)


def _against_the_definition(M, S, **variant):
    """-> (largest distance of v' relative to max v', largest distance of an entry of R~' in float32 ulps of the entry's row maximum)."""
    E, X = random_estimates(M, S, 6, 70, 40 + M)
    E, X = E.copy(), X.copy()
    if S > 1:
        E[1, :, 2] = 0                                         # a target absent from bin 2: n_i = 0 there, R' = I
        E[:, :, :, 5] = 0                                      # a silent frame: v' = 0 for every target, not counted
        X[:, :, 5] = 0
    v, R = AS.powers(E), AS.covariances(E)
    vn, Rn = AE.em_step(v, R, X, **variant)
    vl, Rl = AE.literal_step(v, R, X)
    full = _loaded(Rl, M)
    ulp = np.spacing(np.abs(full).max(axis=(-1, -2)).astype(np.float32)).astype(np.float64)[..., None, None]
    if S > 1:
        assert not vl[:, :, 5].any() and not vl[1, 2].any() and np.array_equal(Rl[1, 2], np.eye(M))
    return np.abs(vn - vl).max() / np.abs(vl).max(), (np.abs(AS.hermitian(Rn, M).astype(np.complex128) - full) / ulp).max(), (vn, Rn, vl)


@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('M', [3, 5, 8])
def test_the_evaluated_form_is_the_definition(M, S):
    """float64 em_step against literal_step.  The definition inverts R~_i, whose condition is at most M (1 + lambda) / lambda ~ 8e3, and
    subtracts tr G_i from M: 1e-10 of the largest power is float64 rounding for it (measured: 1e-15 at S = 3, 6e-13 at S = 1, where R~_i
    of the one target is the worst conditioned).  R~' is compared after its one rounding to float32: within 0.51 ulp of the row's largest
    entry (half an ulp is the rounding itself)."""
    dv, dR, (vn, Rn, vl) = _against_the_definition(M, S)
    print('M = %d, S = %d: v\' within %.3g of max v\'; R~\' within %.3g float32 ulp' % (M, S, dv, dR))
    assert dv < 1e-10 and dR < 0.51
    if S > 1:
        expect = np.zeros(M * M, np.float32)
        expect[:M] = np.float32(1 + AS.LOADING)
        assert np.array_equal(Rn[1, 2], expect) and not vn[1, 2].any() and not vn[:, :, 5].any()
        assert (vn[0, :, :5] > 0).all()
    else:
        # one target: N, k and P are exact zeros, v' = w h / M and the filter returns X
        E, X = random_estimates(M, 1, 6, 70, 40 + M)
        assert np.abs(AE.array_em(E, X, 2)[0] - X).max() < 1e-12 * np.abs(X).max()


@pytest.mark.parametrize('M', [3, 5, 8])
def test_properties_of_the_refined_filter(M):
    S, F, T = 3, 6, 70
    E, X = random_estimates(M, S, F, T, 40 + M)
    scale = np.abs(X).max()
    out = AE.array_em(E, X, 3)
    assert np.abs(out.sum(axis=0) - X).max() < 1e-11 * scale, 'the targets add up to X'
    v, R = AE.refine(E, X, 3)
    full = AS.hermitian(R, M).astype(np.complex128)
    assert (np.linalg.eigvalsh(full) > 0).all(), 'full rank'
    out32 = AE.array_em(E, X, 3, np.float32)
    assert np.abs(out32 - out).max() < 1e-4 * scale, 'the float32 order evaluates the same recursion'
    # a NaN in one bin stays in that bin
    En = E.copy()
    En[0, 1, 3, 7] = np.nan
    for dtype in (np.float64, np.float32):
        outn = AE.array_em(En, X, 2, dtype)
        assert np.isnan(outn[:, :, 3]).all() and not np.isnan(np.delete(outn, 3, axis=2)).any()
    # filter_with on the powers of the estimates is the filter
    R0 = AS.covariances(E)
    assert SC._bits(AE.filter_with(AS.powers(E, np.float32), R0, X, np.float32), AS.spatial_filter(E, X, np.float32, R=R0))
    assert np.abs(AE.filter_with(AS.powers(E), R0, X) - AS.spatial_filter(E, X, R=R0)).max() < 1e-12 * scale, 'LDL^H against numpy.linalg.solve'


@pytest.mark.parametrize('mistake', ['divisor', 'loading', 'count'])
def test_planted_mistakes_fail(mistake):
    """The wrong divisor (2 for M), the loading without the trace, and every frame counted in n_i (the silent frame too), planted in
    em_step, are outside what test_the_evaluated_form_is_the_definition allows."""
    M, S = 4, 3
    variant = dict(divisor=dict(divisor=2), loading=dict(loading='lambda'), count=dict(count='all'))[mistake]
    dv0, dR0, _ = _against_the_definition(M, S)
    assert dv0 < 1e-10 and dR0 < 0.51
    dv, dR, _ = _against_the_definition(M, S, **variant)
    print('%s: v\' off by %.3g of max v\', R~\' by %.3g float32 ulp' % (mistake, dv, dR))
    assert dv >= 1e-10 or dR >= 0.51
    if mistake == 'divisor':
        assert dv > 0.1, 'v" is M / 2 = 2 times too large'
    else:
        assert dv < 1e-10, 'the powers of this iteration do not depend on step 2'


# ---- the condition of the measured bars, at the cells of the device test -------------------------------------------------------------------
@pytest.mark.parametrize('cell', list(C.CELLS), ids=['M%d-S%d-F%d-T%d-b%d' % c for c in C.CELLS])
def test_the_bars_condition_holds_at_every_cell(cell):
    """float32 and float64 have the same zero pattern and the same NaN pattern after 1, 2 and 3 iterations (10 at the cell that runs 10),
    on the ratio stage's restatement of the cell's own file; the bar itself is printed."""
    c = C.CELLS[cell]
    p = C.cell_files(cell)[c['pos']]
    E, X = C.host_ratio(p, cell[1]), p[3]
    for n in (3, 10) if cell == (4, 3, 33, 129, 3) else (3,):
        bar, err, ref, (v32, R32, out32) = AE.measured_bar(E, X, n)      # asserts the condition
        print('%s n=%d: measured bar %.3g of max|X|' % (cell, n, bar))
        assert 0 < err < 1e-4 and np.isfinite(ref).all()
    cache = {}
    for n in (1, 2, 3):
        v64, _ = AE.refine(E, X, n, np.float64, cache=cache)
        v32, R32 = AE.refine(E, X, n, np.float32, cache=cache)
        assert np.array_equal(v64 == 0, v32 == 0) and not np.isnan(v64).any() and not np.isnan(v32).any() and not np.isnan(R32).any()
    if 'zero_frame' in c['args']:
        assert not v32[:, :, c['args']['zero_frame']].any()
    if 'absent' in c['args']:
        assert not v32[c['args']['absent'][0], c['args']['absent'][1]].any()
