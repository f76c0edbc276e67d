"""-m gpu: the offline spatial filter and its EM refinement (csrc/spatial.hip, csrc/spatial_em.hip, csrc/spatial.h), every launch on
its own and every element under its own derived bar, through gccnmf_reconstruct only.  tests/spatial_checks.py holds the problems,
the bars, the exact-order float32 model and the cells; tests/test_spatial_checks_host.py shows on the CPU that NumPy's float32 passes
the bars on every cell and that planted mistakes do not.

Per cell a call with m = 0, 1, ... n iterations is made on the same inputs (spec NaN-filled, the workspace filled with a sentinel).
The call with m iterations leaves the state after iteration m in its workspace, the call with m - 1 the state before it -- the kernel
gives the same bits on every run (no atomics, an order fixed by T alone), so two calls are one recursion observed at two points.

  covariance launch      cov of the m = 0 call: bit for bit the exact-order restatement of the device's ratio spec
  filter, WS = false     the m = 0 output: every element within its bar of the float64 filter on the device's cov and ratio spec
  EM iteration m         powers and cov of call m against one float64 iteration from the powers and cov of call m - 1: every power
                         within its bar (zeros exact, the zero pattern identical), every covariance entry within its bar
  filter, WS = true      the output of call m against the float64 filter on that call's own workspace
  consequences           the targets add up to X within the sum of their bars; S = 1 returns X within its bar
  ownership              rows >= F and frames >= T + T % 2 of the powers keep the sentinel, the frame beside an odd T - 1 is 0, the
                         output's padding is zeros, no input is written

and every one of these outputs is compared, bit for bit, with the float32 model.  Measured on an MI355X: DESIGN 4c and 4h."""
import numpy as np
import pytest

import spatial_checks as C

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

RATIO, SPATIAL = 0x100, 1 << 16
ITER = lambda n: n << 20
SENTINEL = -7.0


@pytest.fixture(scope='module')
def lib():
    from gcc_nmf_amd import _hip
    assert torch.cuda.is_available(), 'the gpu tests need a ROCm device'
    return _hip.lib()


def complex_of(t):
    """(..., 2) float32 -> (...) complex64, the same bits (a + 1j * b would lose the sign of a zero)."""
    return np.ascontiguousarray(t.cpu().numpy()).view(np.complex64)[..., 0]


class Call(object):
    """The operands of one batch on the device, uploaded once; ``run(n)`` is one ratio call and one spatial call with n iterations."""

    def __init__(self, lib, files, S):
        from gcc_nmf_amd.engine import Geometry
        self.lib, self.S, self.B = lib, S, len(files)
        F, K = files[0][0].shape
        T = files[0][4].shape[2]
        self.F, self.T, self.K = F, T, K
        g = self.g = Geometry(F, T, K)
        B = self.B
        Wp, Hp = np.zeros((B, g.Fp, g.Kp), np.float32), np.zeros((B, g.Kp, g.Np), np.float32)
        Ap, Xp = np.zeros((B, g.Kp, g.Tp), np.uint8), np.zeros((B, 2, g.Fp, g.Tp, 2), np.float32)
        self.soft = files[0][3] is not None
        Mp = np.zeros((B, S, g.Kp, g.Tp), np.float32) if self.soft else None
        for j, (W, H, am, masks, X) in enumerate(files):
            Wp[j, :F, :K], Hp[j, :K, :2 * T], Ap[j, :K, :T] = W, H, am
            Xp[j, :, :F, :T, 0], Xp[j, :, :F, :T, 1] = X.real, X.imag
            if self.soft:
                Mp[j, :, :K, :T] = masks
        self.host = [Wp, Hp, Xp, Mp if self.soft else Ap]
        self.dev = [torch.from_numpy(a).cuda() for a in self.host]

    def run(self, n):
        """-> (ratio spec, output) (B, S, 2, F, T) complex64, cov (B, S, F, 4), powers (B, S, F, T) or None."""
        from gcc_nmf_amd import _hip
        g, B, S, F, T, K = self.g, self.B, self.S, self.F, self.T, self.K
        dW, dH, dX, dM = self.dev
        p = lambda t: t.data_ptr()
        am, masks = (0, p(dM)) if self.soft else (p(dM), 0)
        stream = torch.cuda.current_stream().cuda_stream
        spec = torch.full((B, 2 * S, g.Fp, g.Tp, 2), float('nan'), dtype=torch.float32, device='cuda')
        assert self.lib.gccnmf_reconstruct(p(dW), p(dH), am, masks, p(dX), 0, F, T, K, S | RATIO, B, 0, p(spec), stream) == 0
        ratio = complex_of(spec).reshape(B, S, 2, g.Fp, g.Tp)[:, :, :, :F, :T].astype(np.complex64)
        spec.fill_(float('nan'))
        ncov = _hip.reconstruct_spatial_workspace_floats(B, S, g.Fp)
        total = _hip.reconstruct_spatial_em_workspace_floats(B, S, g.Fp, g.Tp)
        ws = torch.full((total,), SENTINEL, dtype=torch.float32, device='cuda')
        assert self.lib.gccnmf_reconstruct(p(dW), p(dH), am, masks, p(dX), 0, F, T, K, S | RATIO | ITER(n), B | SPATIAL, p(ws), p(spec),
                                           stream) == 0
        torch.cuda.synchronize()
        for host, dev in zip(self.host, self.dev):
            assert np.array_equal(dev.cpu().numpy(), host, equal_nan=True), 'an input was written'
        sp = complex_of(spec).reshape(B, S, 2, g.Fp, g.Tp)
        assert (sp[:, :, :, F:, :] == 0).all() and (sp[:, :, :, :, T:] == 0).all(), 'output padding must be written as zeros'
        w = ws.cpu().numpy()
        cov = w[:ncov].reshape(B, S, g.Fp, 4)
        assert (cov[:, :, F:] == SENTINEL).all(), 'rows >= F have no covariance'
        powers = w[ncov:].reshape(B, S, g.Fp, g.Tp)
        if n == 0:
            assert (powers == SENTINEL).all(), 'n = 0 does not touch the powers'
            powers = None
        else:
            assert (powers[:, :, F:] == SENTINEL).all() and (powers[:, :, :, T + T % 2:] == SENTINEL).all(), 'the workspace beyond the row'
            if T % 2:
                assert (powers[:, :, :F, T] == 0).all(), 'the frame beside an odd T - 1 is written as 0'
            powers = powers[:, :, :F, :T].copy()
        return ratio, sp[:, :, :, :F, :T].astype(np.complex64), cov[:, :, :F].copy(), powers


SHARES, NOT_EQUAL = {}, []


@pytest.mark.parametrize('name', sorted(C.CELLS))
def test_cell(lib, name):
    c = C.CELLS[name]
    files = C.cell_files(name)
    call = Call(lib, files, c['S'])
    runs = [call.run(m) for m in range(c['n'] + 1)]
    for b in range(c['B']):
        E = runs[0][0][b]
        for r in runs[1:]:
            assert np.array_equal(r[0][b], E, equal_nan=True), 'the ratio stage gives the same bits on every call'
        stages = dict(E=E, X=files[b][4], out=[r[1][b] for r in runs], cov=[r[2][b] for r in runs],
                      powers=[None if r[3] is None else r[3][b] for r in runs])
        fail, bits, share = C.check_cell(stages, '%s[%d]' % (name, b))
        print('%s[%d] F=%d T=%d S=%d n=%d: largest share of a bar: %s; bit for bit the float32 model: %s' %
              (name, b, c['F'], c['T'], c['S'], c['n'], ', '.join('%s %.3f' % kv for kv in sorted(share.items())), 'yes' if not bits else bits))
        for k, s in share.items():
            SHARES[k] = max(SHARES.get(k, 0.0), s)
        NOT_EQUAL.extend(bits)
        assert not fail, fail
        assert not bits, bits
    if c['B'] > 1:
        alone = Call(lib, [files[c['pos']]], c['S']).run(c['n'])
        for k in range(4):
            assert np.array_equal(alone[k][0], runs[-1][k][c['pos']]), 'a file gives the same bits alone and in its batch'
    print('so far, over the cells: %s; cells with an element that is not the model\'s: %d' %
          (', '.join('%s %.3f' % kv for kv in sorted(SHARES.items())), len(NOT_EQUAL)))
