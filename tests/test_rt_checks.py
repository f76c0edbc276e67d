"""CPU: the nine rules of the real-time stage tests (tests/rt_checks.py) are sound and sensitive.  A float32 NumPy restatement of the whole
call (rt_checks.model32: NumPy's summation orders, not the kernels') stays inside every bar at every cell the GPU suite runs, the vacuity
guard of rule 4 holds for every cell's inputs in float64 alone, the old tolerances of tests/test_gpu_realtime.py are far outside the new
bars, and each typical kernel mistake, applied to the restatement, falls outside its rule at the cell chosen for it.

Largest share of each bar the restatement uses over all cells (printed by the first test): X radix-2 0.03, X direct 0.06, C 0.32,
arg-max allowance 0 (it agrees with float64 everywhere), HMask window 0.54 (2.1 of RT_EXP_U's units -- NumPy's float32 exp / power; the MI355X: 2.17), tfMask
0.03, Rv 0.04, Hcoef 0.08, inferred tfMask 0.04, out_ring 0.13, frames 0.03, gccphat 0.10, GCC-NONLIN 0.25 (= 1 / BAR_FACTOR by
construction)."""
import numpy as np
import pytest

import rt_checks as R

ALL = R.CELLS + R.INFERENCE_CELLS
BY_NAME = {c.name: c for c in ALL}
_cache = {}


def inputs(c):
    if c.name not in _cache:
        I = R.make_inputs(c)
        for v in I.values():
            v.setflags(write=False)
        _cache[c.name] = I
    return _cache[c.name]


@pytest.mark.parametrize('c', ALL, ids=repr)
def test_float32_restatement_stays_inside_every_bar(c):
    I = inputs(c)
    O = R.model32(c, I)
    sh = R.check_call(c, I, O)
    if c.nH:
        c2 = c.with_updates(c.nH + 1)
        sh2 = R.check_call(c2, I, R.model32(c2, I), first=O)
        assert np.array_equal(O['X'].view(np.float32), R.model32(c2, I)['X'].view(np.float32))
        sh = {k: max(sh.get(k, 0), sh2.get(k, 0)) for k in set(sh) | set(sh2)}
    print(c.name, sorted(sh.items()))
    bars = [v for k, v in sh.items() if k not in ('decided', 'tie cells', 'exp_units', 'multi agree')]
    assert bars and max(bars) < 0.75, sh                        # sound with room to spare: the bars are worst cases
    assert sh.get('exp_units', 0) <= R.RT_EXP_U


@pytest.mark.parametrize('c', ALL, ids=repr)
def test_rule_4_is_not_vacuous_for_any_cell(c):
    """From float64 alone: at least 0.9 of the (atom, frame) cells of the live frames are decided -- the float64 leader beats every
    different steering column by more than the two bounds, so rule 4 leaves the device exactly one index there."""
    I = inputs(c)
    share = R.decided64(c, I)
    print(c.name, 'decided share %.4f' % share)
    assert share >= 0.9
    if c.ties:                                                  # the duplicate columns win for many atoms
        ring = np.concatenate([I['in_ring'][0][:, c.B:], I['block_in'][0]], axis=1)
        Gs, bnd, nanf = R.scores64(c, I, R.coherence64(R.analysis64(c, I, ring)[0]))
        firsts = [a for a, b in R.TIE_PAIRS if b < c.D]
        assert np.isin(Gs.argmax(axis=0)[:, ~nanf], firsts).sum() >= 10


def test_the_tie_columns_are_duplicates_across_lane_halves_tiles_and_passes():
    c = BY_NAME['n1024 ties']
    I = inputs(c)
    first_of = R.first_identical(I['cosT'], I['sinT'], c.D)
    assert [int(first_of[b]) for a, b in R.TIE_PAIRS] == [3, 3, 5] and int(first_of[3]) == 3 and int(first_of[5]) == 5
    half, tile = lambda tau: (tau >> 2) & 1, lambda tau: tau // 32
    assert half(3) != half(7) and tile(3) + 1 == tile(36) and tile(36) // 2 == 0 and tile(5) // 2 != tile(70) // 2
    assert (first_of[:c.D] == np.arange(c.D)).sum() == c.D - 3


MISTAKES = [
    ('no_nyquist', 'n64 zero frame', 'argmaxTDOA'),             # the Nyquist row dropped from the scores
    ('no_nyquist', 'n602 delay 1', 'argmaxTDOA'),
    ('wave_last_row', 'n64 zero frame', 'argmaxTDOA'),          # the last row of the first wave's band dropped
    ('wave_last_row', 'n602 delay 1', 'argmaxTDOA'),
    ('padded_row', 'n64 zero frame', 'outside [0, D)'),         # a padded row >= D admitted to the arg-max
    ('padded_row', 'n256 hop 100 boxcar', 'outside [0, D)'),
    ('tie_larger', 'n1024 ties', 'duplicate steering column'),  # a tie resolved to the larger index
    ('tie_larger', 'n64 zero frame', 'duplicate steering column'),
    ('atom_last', 'n256 hop 100 boxcar', 'outside [0, D)'),     # atom K - 1 not written: its index is still the sentinel
    ('atom_last', 'multi 3', 'outside [0, D)'),
    ('no_nf', 'n64 zero frame', 'HMask (window function)'),     # nf left out of the window mask
    ('den_kp', 'n64 zero frame', 'tfMask'),                     # the tfMask denominator summed over Kp
    ('den_kp', 'multi 3', 'tfMask'),
    ('shift_off1', 'n400 block 600 delay 7', 'in_ring'),        # the shift off by one sample from the chunk boundary on
    ('handout', 'n64 zero frame', 'block_out'),                 # the hand-out taken from out_delay + 1
    ('handout', 'n602 delay 1', 'block_out'),
    ('hist_nowrap', 'n64 zero frame', 'hist_pos'),              # hist_pos not wrapped
    ('nan_counted', 'n64 frames nan bins', 'gccphat'),          # a NaN term counted in the nanmean
    ('stale_h', 'n64 inferred', 'Rv'),                          # the first coefficient update reading a stale Hcoef
    ('stale_h', 'n400 inferred', 'Rv'),
    ('silent_nan', 'n64 inferred zero frame', 'silent channel'),  # 0 / 0 of a silent channel left as NaN (what the kernels did)
    ('silent_nan', 'n32 inferred silent right', 'silent channel'),
]


@pytest.mark.parametrize('bug,cell,where', MISTAKES, ids=['%s at %s' % m[:2] for m in MISTAKES])
def test_each_mistake_falls_outside_its_rule(bug, cell, where):
    c = BY_NAME[cell]
    I = inputs(c)
    R.check_call(c, I, R.model32(c, I))
    with pytest.raises(AssertionError) as e:
        R.check_call(c, I, R.model32(c, I, bug=bug))
    print(e.value)
    assert where in str(e.value), str(e.value)


OLD_TOLERANCES = [
    # what tests/test_gpu_realtime.py tolerates today, applied to one element of an honest result: far outside the new bars.  (Not X: its
    # worst-case bar per element, 6 log2(N) u sum |z|, is about 3e-5 max|X| at N = 1024 -- the gain there is that it holds per element,
    # each frame against its own magnitude, not against the image's maximum.)
    ('C', (0, 5, 0), lambda O: 2e-3, ' C'),
    ('HMask', (0, 0, 5, 0), lambda O: 1e-5, 'HMask'),
    ('tfMask', (0, 0, 0, 5, 0), lambda O: 1e-4, 'tfMask'),
    ('gccphat', (0, 5, 0), lambda O: 1e-3, 'gccphat'),
]


@pytest.mark.parametrize('key,i,step,where', OLD_TOLERANCES, ids=[t[0] for t in OLD_TOLERANCES])
def test_the_old_tolerances_are_outside_the_new_bars(key, i, step, where):
    c = BY_NAME['n1024 ties']
    I = inputs(c)
    O = R.model32(c, I)
    a = O[key]
    a[i] = a[i] + np.float32(step(O))
    with pytest.raises(AssertionError) as e:
        R.check_call(c, I, O)
    assert where in str(e.value), str(e.value)


def test_an_undecided_cell_may_differ_and_a_decided_one_may_not():
    """Rule 4 on a constructed pair: moving the device's index to the float64 runner-up fails wherever the cell is decided."""
    c = BY_NAME['n64 hop 80 delay 7']
    I = inputs(c)
    O = R.model32(c, I)
    Gs, bnd, nanf = R.scores64(c, I, O['C'][0])
    second = np.argsort(Gs, axis=0)[-2]
    O['argmax'][0, 7, 1] = second[7, 1]
    with pytest.raises(AssertionError, match='below the float64 maximum'):
        R.check_call(c, I, O)
