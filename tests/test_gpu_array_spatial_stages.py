"""-m gpu: gccnmf_array_spatial (include/gccnmf_array_spatial.h, csrc/array_spatial.hip) through the C ABI, element by element.

The estimates E are produced by gccnmf_array_reconstruct on the device and copied before the call, so that both stages are checked on
the state they started from.  Per cell of tests/array_spatial_checks.py (M, S, F, T, batch), by its check_cell:
  cov    bit for bit the restatement with the device's summation order; within one float32 ulp of the ascending-order sums
  spec   bit for bit the float32 restatement (the header's order); within bar_filter_M of the float64 one (numpy.linalg.solve)
  spec   also within the normwise bar of array_spatial_checks.normwise_filter, with the residual of the sum of the targets
  the sum of the targets within the summed bars of X;  padding rows and frames zero out of NaN-filled buffers;  slots >= S M untouched
and a file alone gives the bits it gives in the batch.  M = 2: cov and spec hold the bits of gccnmf_reconstruct in spatial mode."""
import numpy as np
import pytest

import array_spatial_checks as C

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

OK, ARG, UNSUPPORTED = 0, 1, 3
NAN = float('nan')


@pytest.fixture(scope='module')
def libs():
    from gcc_nmf_amd import _array, _array_spatial, _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib(), _array.lib(), _array_spatial.lib()


def rup(a, b):
    return -(-a // b) * b


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def device_operands(files, K=C.K_ATOMS):
    """files: [(W, H, argmax, X)] of one shape -> padded device buffers (W, H, argmax, X); X's padding is NaN (the kernels use none of it)."""
    B = len(files)
    M, F, T = files[0][3].shape
    Fp, Kp, Tp, Np = rup(F, 16), rup(K, 64), rup(T, 64), rup(M * T, 64)
    Wp, Hp, Ap = np.zeros((B, Fp, Kp), np.float32), np.zeros((B, Kp, Np), np.float32), np.zeros((B, Kp, Tp), np.uint8)
    Xp = np.full((B, M, Fp, Tp, 2), NAN, np.float32)
    for b, (W, H, am, X) in enumerate(files):
        Wp[b, :F, :K], Hp[b, :K, :M * T], Ap[b, :K, :T] = W, H, am
        Xp[b, :, :F, :T, 0], Xp[b, :, :F, :T, 1] = X.real, X.imag
    return dev(Wp), dev(Hp), dev(Ap), dev(Xp)


def run_device(files, S, pitch):
    """-> (E, cov, out) as the device left them: E [B][pitch][Fp][Tp][2] before the spatial call, cov [B][S][Fp][M M], out like E."""
    from gcc_nmf_amd import _array, _array_spatial
    B = len(files)
    M, F, T = files[0][3].shape
    dW, dH, dA, dX = device_operands(files)
    Fp, Tp = dX.shape[2], dX.shape[3]
    spec = torch.full((B, pitch, Fp, Tp, 2), NAN, dtype=torch.float32, device='cuda')
    _array.reconstruct(dW, dH, dA, None, dX, M, F, T, C.K_ATOMS, S, B, pitch, spec)
    E = spec.clone()
    assert _array_spatial.workspace_floats(M, F, S, B) == B * S * Fp * M * M
    cov = torch.full((B, S, Fp, M * M), NAN, dtype=torch.float32, device='cuda')
    _array_spatial.spatial(dX, M, F, T, S, B, pitch, cov, spec)
    torch.cuda.synchronize()
    return E, cov, spec


def host(planes, S, M, F, T):
    """[pitch][Fp][Tp][2] -> (S, M, F, T) complex64"""
    a = np.ascontiguousarray(planes[:S * M, :F, :T].cpu().numpy())
    return a.view(np.complex64)[..., 0].reshape(S, M, F, T)              # (re + 1j * im would turn an imaginary part -0 into +0)


@pytest.mark.parametrize('cell', list(C.CELLS), ids=['M%d-S%d-F%d-T%d-b%d' % c for c in C.CELLS])
def test_cells_element_by_element(libs, cell):
    M, S, F, T, B = cell
    c = C.CELLS[cell]
    pitch = c['pitch'] or rup(S * M, 2)
    files = C.cell_files(cell)
    E, cov, out = run_device(files, S, pitch)
    Fp, Tp = E.shape[2], E.shape[3]
    # what the call must not touch, and what it must write as zeros
    assert same_bits(out[:, S * M:], E[:, S * M:]) and (pitch == S * M or bool(torch.isnan(out[:, S * M:]).all())), 'slots >= S M keep their bits'
    written = out[:, :S * M]
    assert not bool(torch.isnan(written[:, :, F:]).any()) and not written[:, :, F:].any(), 'rows >= F are zeros'
    assert not bool(torch.isnan(written[:, :, :, T:]).any()) and not written[:, :, :, T:].any(), 'frames >= T are zeros'
    assert bool(torch.isnan(cov[:, :, F:]).all()) and not bool(torch.isnan(cov[:, :, :F]).any()), 'cov: rows f < F are written, no other'
    behind = total = 0
    for b in range(B):
        Eb, Xb = host(E[b], S, M, F, T), files[b][3]
        fail, bits, share, (n, g, _) = C.check_cell(Eb, Xb, cov[b, :, :F].cpu().numpy(), host(out[b], S, M, F, T), '%s[%d]' % (cell, b))
        print('%s[%d]: largest share of a bar: %s; %d of %d elements behind a failed guard' %
              (cell, b, ', '.join('%s %.4f' % kv for kv in sorted(share.items())), g, n))
        assert not fail, fail
        assert not bits, bits
        behind, total = behind + g, total + n
    assert behind <= C.GUARD_CAP * total
    if 'zero_frame' in c['args']:
        assert not host(out[c['pos']], S, M, F, T)[:, :, :, c['args']['zero_frame']].any(), 'a silent frame gives zeros'
    if 'absent' in c['args']:
        i, f = c['args']['absent']
        row = np.zeros(M * M, np.float32)
        row[:M] = np.float32(1 + 1e-3)
        assert np.array_equal(cov[c['pos'], i, f].cpu().numpy(), row), 'n = 0: R = I'
    if B > 1:
        # the cell's file alone = the file in the batch, bit for bit
        p = c['pos']
        E1, cov1, out1 = run_device(files[p:p + 1], S, pitch)
        assert same_bits(E1[0], E[p]) and same_bits(cov1[0, :, :F], cov[p, :, :F]) and same_bits(out1[0, :S * M], out[p, :S * M])


@pytest.mark.parametrize('T', [1, 2, 127, 129, 257])
@pytest.mark.parametrize('S', [1, 3, 8])
def test_two_channels_are_the_stereo_spatial_mode_bit_for_bit(libs, S, T):
    from gcc_nmf_amd import _hip
    M, F, B = 2, 17, 2
    files = [C.structured(M, F, T, S, 500 + 10 * S + T, zero_frame=T // 2 if T > 2 else None), C.uniform(M, F, T, S, 900 + S + T)]
    E, cov, out = run_device(files, S, 2 * S)
    dW, dH, dA, dX = device_operands(files)
    Fp, Tp = dX.shape[2], dX.shape[3]
    stereo = torch.full((B, 2 * S, Fp, Tp, 2), NAN, dtype=torch.float32, device='cuda')
    ws = torch.full((_hip.reconstruct_workspace_floats('spatial', T, C.K_ATOMS, S, B, Fp),), NAN, dtype=torch.float32, device='cuda')
    _hip.reconstruct(dW, dH, dA, None, dX, None, F, T, C.K_ATOMS, S, B, stereo, mode='spatial', workspace=ws)
    torch.cuda.synchronize()
    assert same_bits(cov[:, :, :F], ws.view(B, S, Fp, 4)[:, :, :F]), 'cov'
    assert same_bits(out, stereo), 'spec'
    assert bool(torch.isfinite(out).all()) and out.abs().max() > 0


def test_argument_errors_leave_the_buffers_untouched(libs):
    lib = libs[2]
    M, F, T, S, B = 3, 33, 5, 2, 2
    Fp, Tp = 48, 64
    X = torch.ones((B, M, Fp, Tp, 2), dtype=torch.float32, device='cuda')
    spec = torch.full((B, S * M, Fp, Tp, 2), NAN, dtype=torch.float32, device='cuda')
    cov = torch.full((B, S, Fp, M * M), NAN, dtype=torch.float32, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    ok = dict(X=X.data_ptr(), M=M, F=F, T=T, S=S, batch=B, pitch=S * M, cov=cov.data_ptr(), spec=spec.data_ptr())
    order = ('X', 'M', 'F', 'T', 'S', 'batch', 'pitch', 'cov', 'spec')
    call = lambda **kw: lib.gccnmf_array_spatial(*[dict(ok, **kw)[k] for k in order], st)
    for kw in (dict(X=0), dict(spec=0), dict(cov=0), dict(cov=cov.data_ptr() + 4), dict(M=1), dict(M=9), dict(F=1), dict(T=0), dict(batch=0),
               dict(pitch=S * M - 1)):
        assert call(**kw) == ARG, kw
    for kw in (dict(S=0), dict(S=9, pitch=27), dict(batch=21846)):
        assert call(**kw) == UNSUPPORTED, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(spec).all()) and bool(torch.isnan(cov).all())
    spec.fill_(1.0)
    assert call() == OK
    torch.cuda.synchronize()
    assert not bool(torch.isnan(spec).any()) and not bool(torch.isnan(cov[:, :, :F]).any())
