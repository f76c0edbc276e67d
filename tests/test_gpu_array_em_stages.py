"""-m gpu: gccnmf_array_em (include/gccnmf_array_em.h, csrc/array_spatial_em.hip) through the C ABI, element by element.

The estimates E are produced by gccnmf_array_reconstruct on the device and copied before the call.  Per cell of
tests/array_spatial_checks.py (M, S, F, T, batch) and n = 1, 2, 3 (n = 1: the first sweep on the powers of the estimates; n = 2: the new
powers read back from the workspace and the new cov rows from LDS; n = 3: a second hand-over), one cell at n = 10:
  cov, the powers and spec   bit for bit the float32 restatement (tests/array_em_restatement.py: the header's order, the device's frame sums)
  spec   every element within the measured bar of the float64 restatement -- BAR_FACTOR times the float32-to-float64 distance of the
         restatement, relative to max|X| -- printed per case
  padding rows and frames of the S M written slots are zeros out of a NaN-filled spec;  slots >= S M and the workspace's rows >= F keep
  the bits they had.
M = 2: all three buffers hold the bits of gccnmf_reconstruct in spatial mode with the same n.  A file alone gives the bits it gives in a
batch; a NaN in X stays in its bin of its file; argument errors leave every buffer untouched."""
import numpy as np
import pytest

import array_em_restatement as AE
import array_spatial_checks as C
import spatial_checks as SC
from test_gpu_array_spatial_stages import NAN, OK, ARG, UNSUPPORTED, rup, dev, same_bits, device_operands, host

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SENTINEL = -12345.0


@pytest.fixture(scope='module')
def libs():
    from gcc_nmf_amd import _array, _array_em, _array_spatial, _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib(), _array.lib(), _array_spatial.lib(), _array_em.lib()


def run_device(files, S, pitch, n, dX=None):
    """-> (E, cov, powers, out) as the device left them: E [B][pitch][Fp][Tp][2] before the call, cov [B][S][Fp][M M] and powers
    [B][S][Fp][Tp] the two parts of the workspace, out like E."""
    from gcc_nmf_amd import _array, _array_em
    B = len(files)
    M, F, T = files[0][3].shape
    dW, dH, dA, X = device_operands(files)
    dX = X if dX is None else dX
    Fp, Tp = dX.shape[2], dX.shape[3]
    spec = torch.full((B, pitch, Fp, Tp, 2), NAN, dtype=torch.float32, device='cuda')
    _array.reconstruct(dW, dH, dA, None, dX, M, F, T, C.K_ATOMS, S, B, pitch, spec)
    E = spec.clone()
    ncov = B * S * Fp * M * M
    assert _array_em.workspace_floats(M, F, T, S, B) == ncov + B * S * Fp * Tp
    ws = torch.full((ncov + B * S * Fp * Tp,), SENTINEL, dtype=torch.float32, device='cuda')
    _array_em.em(dX, M, F, T, S, B, pitch, n, ws, spec)
    torch.cuda.synchronize()
    return E, ws[:ncov].view(B, S, Fp, M * M), ws[ncov:].view(B, S, Fp, Tp), spec


@pytest.fixture(scope='module')
def chains():
    """(cell, file) -> the cache of AE.refine: the restatement's states after 0, 1, 2, ... iterations, computed once and extended."""
    return {}


CASES = [(cell, n) for cell in C.CELLS for n in (1, 2, 3)] + [((4, 3, 33, 129, 3), 10)]


@pytest.mark.parametrize('cell,n', CASES, ids=['M%d-S%d-F%d-T%d-b%d-n%d' % (c + (n,)) for c, n in CASES])
def test_cells_element_by_element(libs, chains, cell, n):
    M, S, F, T, B = cell
    c = C.CELLS[cell]
    p = c['pos']
    pitch = c['pitch'] or rup(S * M, 2)
    files = C.cell_files(cell)
    E, cov, powers, out = run_device(files, S, pitch, n)
    # what the call must not touch, and what it must write as zeros
    assert same_bits(out[:, S * M:], E[:, S * M:]) and (pitch == S * M or bool(torch.isnan(out[:, S * M:]).all())), 'slots >= S M keep their bits'
    written = out[:, :S * M]
    assert not bool(torch.isnan(written[:, :, F:]).any()) and not written[:, :, F:].any(), 'rows >= F are zeros'
    assert not bool(torch.isnan(written[:, :, :, T:]).any()) and not written[:, :, :, T:].any(), 'frames >= T are zeros'
    assert bool((cov[:, :, F:] == SENTINEL).all()) and bool((powers[:, :, F:] == SENTINEL).all()), 'the workspace: rows f < F are written, no other'
    assert bool((powers[:, :, :, T:] == SENTINEL).all()), 'the powers: frames >= T keep their bits (M >= 3)'
    assert not bool((cov[:, :, :F] == SENTINEL).any()) and not bool((powers[:, :, :F, :T] == SENTINEL).any())
    # the cell's own file against the restatement
    Eb, Xb = host(E[p], S, M, F, T), files[p][3]
    cache = chains.setdefault((cell, p), {})
    if cache.get('E') is None:
        cache['E'] = Eb
    assert SC._bits(cache['E'], Eb), 'the ratio stage gives the same estimates in every run'
    v64, R64 = AE.refine(Eb, Xb, n, np.float64, cache=cache)
    v32, R32 = AE.refine(Eb, Xb, n, np.float32, cache=cache)
    assert np.array_equal(v64 == 0, v32 == 0) and np.array_equal(np.isnan(v64), np.isnan(v32)), 'the condition the bar rests on'
    ref, f32 = AE.filter_with(v64, R64, Xb, np.float64), AE.filter_with(v32, R32, Xb, np.float32)
    scale = float(np.abs(Xb).max())
    err = float(np.abs(f32 - ref).max()) / scale
    bar = AE.BAR_FACTOR * err
    got = host(out[p], S, M, F, T)
    dist = float(np.abs(got.astype(np.complex128) - ref).max()) / scale
    print('%s n=%d: measured bar %.3g of max|X| (float32 restatement %.3g); the device is at %.3g' % (cell, n, bar, err, dist))
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    assert np.array_equal(got == 0, ref == 0), 'the exact zeros of the reference'
    assert dist <= bar, (dist, bar)
    dcov, dpow = cov[p, :, :F].cpu().numpy(), powers[p, :, :F, :T].cpu().numpy()
    differ = {k: int((a.view(np.int32) != b.view(np.int32)).sum()) for k, a, b in
              (('cov', dcov, R32), ('powers', dpow, v32), ('spec', got.view(np.float32), f32.view(np.float32)))}
    assert not any(differ.values()), 'elements that are not the float32 restatement\'s bits: %s' % differ
    if 'zero_frame' in c['args']:
        assert not got[:, :, :, c['args']['zero_frame']].any() and not dpow[:, :, c['args']['zero_frame']].any(), 'a silent frame gives zeros'
    if 'absent' in c['args']:
        i, f = c['args']['absent']
        row = np.zeros(M * M, np.float32)
        row[:M] = np.float32(1 + 1e-3)
        assert np.array_equal(dcov[i, f], row) and not dpow[i, f].any() and not got[i, :, f].any(), 'n_i = 0: R\' = I'
    if B > 1 and n == 2:
        # the cell's file alone = the file in the batch, bit for bit
        E1, cov1, pow1, out1 = run_device(files[p:p + 1], S, pitch, n)
        assert same_bits(E1[0], E[p]) and same_bits(cov1[0, :, :F], cov[p, :, :F]) and same_bits(pow1[0, :, :F, :T], powers[p, :, :F, :T])
        assert same_bits(out1[0, :S * M], out[p, :S * M])
        # ... and at another place in a batch
        other = (p + 1) % B
        swapped = list(files)
        swapped[p], swapped[other] = files[other], files[p]
        E2, cov2, pow2, out2 = run_device(swapped, S, pitch, n)
        assert same_bits(cov2[other, :, :F], cov[p, :, :F]) and same_bits(pow2[other, :, :F, :T], powers[p, :, :F, :T])
        assert same_bits(out2[other, :S * M], out[p, :S * M])


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('T', [2, 129])
@pytest.mark.parametrize('S', [1, 3])
def test_two_channels_are_the_stereo_call_bit_for_bit(libs, S, T, n):
    from gcc_nmf_amd import _hip
    M, F, B = 2, 17, 2
    files = [C.structured(M, F, T, S, 500 + 10 * S + T, zero_frame=T // 2 if T > 2 else None), C.uniform(M, F, T, S, 900 + S + T)]
    E, cov, powers, out = run_device(files, S, 2 * S, n)
    dW, dH, dA, dX = device_operands(files)
    Fp, Tp = dX.shape[2], dX.shape[3]
    stereo = torch.full((B, 2 * S, Fp, Tp, 2), NAN, dtype=torch.float32, device='cuda')
    need = _hip.reconstruct_workspace_floats('spatial', T, C.K_ATOMS, S, B, Fp, iterations=n)
    assert need == B * S * Fp * 4 + B * S * Fp * Tp
    ws = torch.full((need,), SENTINEL, dtype=torch.float32, device='cuda')
    _hip.reconstruct(dW, dH, dA, None, dX, None, F, T, C.K_ATOMS, S, B, stereo, mode='spatial', workspace=ws, iterations=n)
    torch.cuda.synchronize()
    assert same_bits(cov, ws[:B * S * Fp * 4].view(B, S, Fp, 4)), 'cov'
    assert same_bits(powers, ws[B * S * Fp * 4:].view(B, S, Fp, Tp)), 'the powers'
    assert same_bits(out, stereo), 'spec'
    assert bool(torch.isfinite(out).all()) and out.abs().max() > 0


def test_a_nan_stays_in_its_bin_of_its_file(libs):
    M, S, F, T, B, n = 3, 2, 17, 70, 2, 2
    files = [C.structured(M, F, T, S, 71), C.uniform(M, F, T, S, 72)]
    E, cov, powers, out = run_device(files, S, S * M, n)
    dX = device_operands(files)[3]
    f, t = 5, 33
    dX[0, 1, f, t, 0] = NAN
    En, covn, pown, outn = run_device(files, S, S * M, n, dX=dX)
    assert bool(torch.isnan(outn[0, :, f, :T]).all()) and bool(torch.isnan(covn[0, :, f]).all()), 'the bin of the NaN is NaN'
    keep = [g for g in range(F) if g != f]
    assert same_bits(outn[0][:, keep], out[0][:, keep]) and same_bits(covn[0][:, keep], cov[0][:, keep])
    assert same_bits(pown[0][:, keep], powers[0][:, keep])
    assert same_bits(outn[1], out[1]) and same_bits(covn[1], cov[1]) and same_bits(pown[1], powers[1]), 'the other file'
    assert not bool(torch.isnan(out[:, :, :F, :T]).any())


def test_argument_errors_leave_the_buffers_untouched(libs):
    lib = libs[3]
    M, F, T, S, B = 3, 33, 5, 2, 2
    Fp, Tp = 48, 64
    X = torch.ones((B, M, Fp, Tp, 2), dtype=torch.float32, device='cuda')
    spec = torch.full((B, S * M, Fp, Tp, 2), NAN, dtype=torch.float32, device='cuda')
    ws = torch.full((B * S * Fp * (M * M + Tp),), NAN, dtype=torch.float32, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    ok = dict(X=X.data_ptr(), M=M, F=F, T=T, S=S, batch=B, pitch=S * M, n=2, ws=ws.data_ptr(), spec=spec.data_ptr())
    order = ('X', 'M', 'F', 'T', 'S', 'batch', 'pitch', 'n', 'ws', 'spec')
    call = lambda **kw: lib.gccnmf_array_em(*[dict(ok, **kw)[k] for k in order], st)
    for kw in (dict(X=0), dict(spec=0), dict(ws=0), dict(ws=ws.data_ptr() + 4), dict(M=1), dict(M=9), dict(F=1), dict(T=0), dict(batch=0),
               dict(pitch=S * M - 1)):
        assert call(**kw) == ARG, kw
    for kw in (dict(S=0), dict(S=9, pitch=27), dict(batch=21846), dict(n=0), dict(n=256), dict(n=-1)):
        assert call(**kw) == UNSUPPORTED, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(spec).all()) and bool(torch.isnan(ws).all())
    spec.fill_(1.0)
    assert call() == OK
    torch.cuda.synchronize()
    assert not bool(torch.isnan(spec).any()) and not bool(torch.isnan(ws[:B * S * Fp * M * M].view(B, S, Fp, M * M)[:, :, :F]).any())
