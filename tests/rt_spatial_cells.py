"""The cells of the online spatial filter's stage tests (tests/test_gpu_rt_spatial_stage.py on the device, tests/test_rt_spatial_host.py on
rt_checks.model32): an rt_checks.Cell -- the call's shape and inputs -- plus the filter's own settings.  Plain NumPy."""
import numpy as np

import rt_checks as R
import rt_spatial_restatement as RS

ROW8 = 1 << 24
SPATIAL = 2                     # GCCNMF_RT_SEPARATION_SPATIAL


class SpatialCell(object):
    """tau: word 7 of every stream's row (the bank cell overrides it per stream); state: 'random' (positive-semidefinite, the test's
    own) or 'zero'; nan_frame: a NaN sample in that frame of the left channel (frames mode); rank_deficient: exempt from the condition on
    the bar; applies: the planted mistakes that must show on this cell."""

    def __init__(self, cell, tau=4.0, state='random', nan_frame=None, rank_deficient=False, applies=('update_after_use',)):
        self.c, self.tau, self.state, self.nan_frame, self.rank_deficient, self.applies = cell, tau, state, nan_frame, rank_deficient, applies
        if not (cell.bank or cell.multi):
            cell.rowlen = 8                                    # the filter's switch is word 7: the 8-word single-stream row (bit 24)
        self.name = cell.name
        self.NC = cell.NT if cell.multi else 2
        self.NY = cell.nM

    def bits(self):
        return self.c.bits() | (0 if (self.c.bank or self.c.multi) else ROW8)

    def taus(self):
        """Word 7 per stream: in the bank stream 0 filters, stream 1 has its separation off (rt_checks.make_inputs) and stream 2 a word 7 of 0."""
        t = np.full(self.c.nS, self.tau, np.float32)
        if self.c.bank:
            t[2] = 0
        return t

    def filtered(self, s):
        return bool(self.taus()[s] >= 1) and not (self.c.bank and s == 1)

    def __repr__(self):
        return self.name


def make_inputs(sc):
    """rt_checks.make_inputs plus word 7 of the rows, the NaN sample and the prior state 'spatial' (S, NC, F, 4) float32."""
    c = sc.c
    I = R.make_inputs(c)
    I['target'][:, 7] = sc.taus()
    if sc.nan_frame is not None:
        assert c.frames
        I['in_ring'][:, 0, sc.nan_frame * c.N + 5] = np.nan
    rms = float(np.sqrt(np.mean(np.square(I['in_ring'][np.isfinite(I['in_ring'])]), dtype=np.float64)))
    scale = rms * np.sqrt(c.N / 2.0)                          # the size of a bin of X, roughly
    if sc.state == 'zero':
        I['spatial'] = np.zeros((c.nS, sc.NC, c.F, 4), np.float32)
    else:
        I['spatial'] = np.stack([RS.random_state(sc.NC, c.F, 100 + s, scale) for s in range(c.nS)])
    return I


def hist_buffer(sc, I):
    """The buffer behind the call's `hist` pointer: the S history images, then from the first multiple of 4 floats the state."""
    c = sc.c
    flat = I['hist'].reshape(-1)
    off = -(-flat.size // 4) * 4
    buf = np.full(off + I['spatial'].size, np.float32(-3.0))   # the gap (if any) holds a value nothing may change
    buf[:flat.size], buf[off:] = flat, I['spatial'].reshape(-1)
    return buf, off


C = R.Cell
CELLS = [
    SpatialCell(C('n64 window tau 4', 64, 16, 48, 33, 33), applies=('update_after_use', 'no_carry', 'no_residual')),
    SpatialCell(C('n64 boxcar zero state', 64, 16, 48, 33, 33, mode=0), state='zero', applies=('update_after_use', 'no_carry', 'no_residual')),
    SpatialCell(C('n602 one frame', 602, 301, 301, 64, 32, od=1, row=(None, 3.0, 3.0, 0.0)), applies=('update_after_use', 'no_residual')),
    SpatialCell(C('n1024 one frame', 1024, 512, 512, 64, 32), applies=('update_after_use', 'no_residual')),
    SpatialCell(C('n64 inferred', 64, 16, 48, 33, 32, nH=1), applies=('update_after_use', 'no_carry', 'no_residual')),
    SpatialCell(C('multi 1', 64, 32, 64, 64, 65, NT=1), applies=()),                       # the output is X whatever the state
    SpatialCell(C('multi 3', 64, 32, 64, 33, 65, NT=3), applies=('update_after_use', 'no_carry')),
    SpatialCell(C('multi 8', 256, 128, 128, 100, 130, NT=8, L=1), applies=('update_after_use',)),
    SpatialCell(C('multi 3 inferred', 64, 32, 64, 33, 33, NT=3, nH=1), applies=('update_after_use', 'no_carry')),
    SpatialCell(C('n64 zero frame', 64, 16, 48, 33, 33, zero_frame=1, row=(None, 5.0, 2.0, 0.125)), applies=('update_after_use', 'no_carry', 'no_residual')),
    SpatialCell(C('n64 silent right', 64, 32, 64, 64, 32, silent_right=True, decided=False), state='zero', rank_deficient=True, applies=()),
    # per-channel masks: with one mask for both channels and no memory both components' covariances are the frame's own rank-1 matrix,
    # and the filter returns v_0 / (v_0 + v_1) X whatever R~ is
    SpatialCell(C('n64 tau 1 inferred', 64, 16, 48, 33, 32, nH=1), tau=1.0, applies=('update_after_use', 'no_residual')),
    SpatialCell(C('n64 tau 1e6', 64, 16, 48, 33, 33), tau=1e6, applies=('no_residual',)),
    SpatialCell(C('n64 frames nan sample', 64, 64, 192, 64, 33, frames=True), nan_frame=1, applies=('update_after_use', 'no_carry', 'no_skip')),
    SpatialCell(C('bank of 3', 64, 32, 64, 33, 33, S=3, row=(None, 4.0, 2.0, 0.125)), applies=('update_after_use', 'no_carry', 'no_residual')),
]


def stream_io(sc, O, s):
    """(Y (NY, 2, F, Tc), X (2, F, Tc)) of stream s from a call's outputs."""
    return O['Y'][s], O['X'][s]
