"""CPU: tests/spatial_checks.py on NumPy's own float32 -- the float32 model of the offline spatial filter and its EM refinement passes
every derived bar on every cell of tests/test_gpu_spatial_stages.py with no element left out, the device's summation order is tied
to the ascending one of tests/spatial_restatement.py, and each planted mistake fails the bars on the cells named here.  The ratio
stage's estimates come from its restatement (tests/ratio_restatement.py) rounded to float32; on the device they are the device's own."""
import numpy as np
import pytest

import spatial_checks as C
import spatial_em_restatement as EM
import spatial_restatement as SR


@pytest.fixture(scope='module')
def problems():
    """cell -> [(E, X)] per file of its batch, computed once and left unchanged."""
    out = {}
    for name, c in C.CELLS.items():
        out[name] = [(C.host_ratio(p, c['S']), p[4]) for p in C.cell_files(name)]
        for E, X in out[name]:
            E.setflags(write=False)
            X.setflags(write=False)
    return out


def test_the_cell_table_covers_what_it_has_to():
    cells = C.CELLS.values()
    assert {c['T'] for c in cells} >= {1, 2, 127, 128, 129, 257}
    assert {c['F'] for c in cells} >= {4, 17, 33, 40}
    assert {c['S'] for c in cells} == set(range(1, 9)), 'every instantiation of the three kernel templates'
    assert {c['n'] for c in cells} >= {1, 2, 3}
    assert {(c['B'], c['pos']) for c in cells} >= {(1, 0), (3, 0), (3, 2)}
    options = set()
    for c in cells:
        options |= set(c['args']) | ({'weak%d' % c['args']['weak'][1]} if 'weak' in c['args'] else set())
    assert options >= {'weak40', 'weak80', 'absent', 'zero_bin', 'zero_frame', 'tiny_frame', 'soft'}
    assert sum(c['kind'] == 'uniform' and not c['args'] for c in cells) == 1


def test_the_problems_reach_their_regimes(problems):
    E, X = problems['weak80'][0]
    v = SR.powers(E)
    share = v[2].sum() / v.sum()
    level = np.abs(X).max(axis=(0, 2))
    print('weak80: the weak target holds %.3g of the power; the bins span %.1f dB, the frames %.1f dB' %
          (share, 20 * np.log10(level.max() / level.min()), 20 * np.log10(np.abs(X).max(axis=(0, 1)).max() / np.abs(X).max(axis=(0, 1)).min())))
    assert 1e-10 < share < 1e-6 and level.max() / level.min() > 300
    R = SR.covariances(E)
    assert np.abs(R[:, :, 2:]).max() > 0.5, 'the estimates have an inter-channel structure'
    E, X = problems['absent'][0]
    assert (E[0, :, 7] == 0).all() and np.array_equal(SR.covariances(E)[0, 7], np.float32([1 + C.LOADING, 1 + C.LOADING, 0, 0]))
    E, X = problems['zero_bin'][0]
    assert (X[:, 3] == 0).all() and (E[:, :, 3] == 0).all()
    E, X = problems['zero_frame'][2]
    assert (X[:, :, 130] == 0).all() and (np.abs(X[:, :, 129]) > 0).all()
    E, X = problems['tiny_frame'][0]
    assert 1e-11 < np.abs(X[:, :, 11]).max() < 1e-9


def test_device_sum_is_the_stated_order():
    """Against a literal loop over lanes and butterfly steps, at every T of the cells and one with a third sweep's odd tail."""
    rng = np.random.RandomState(3)
    for T in (1, 2, 127, 128, 129, 257, 300):
        x = rng.randn(3, T) * 10.0 ** rng.uniform(-8, 0, (3, T))
        for row in range(3):
            part = [0.0] * 64
            for lane in range(64):
                for t in range(2 * lane, T, 128):
                    part[lane] += x[row, t]
                    if t + 1 < T:
                        part[lane] += x[row, t + 1]
            for k in (1, 2, 4, 8, 16, 32):
                part = [part[lane] + part[lane ^ k] for lane in range(64)]
            assert len(set(part)) == 1 and part[0] == C.device_sum(x)[row]
    assert C.device_sum(np.array([np.nan, 1.0])) != C.device_sum(np.array([np.nan, 1.0]))        # NaN stays NaN


SHARES = {}


@pytest.mark.parametrize('name', sorted(C.CELLS))
def test_the_float32_model_passes_every_bar(problems, name):
    """... with no element left out (a failed guard on a non-zero element is a failure of check_cell), the zero pattern of the powers
    identical in float32 and float64 at every iteration, and the device-order covariances within one float32 ulp of the ascending ones."""
    c = C.CELLS[name]
    for b, (E, X) in enumerate(problems[name]):
        stages = C.model_stages(E, X, c['n'])
        fail, bits, share = C.check_cell(stages, '%s[%d]' % (name, b))
        assert not fail, fail
        assert not bits, bits
        for k, s in share.items():
            SHARES[k] = max(SHARES.get(k, 0.0), s)
        print('%s[%d]: largest share of a bar: %s' % (name, b, ', '.join('%s %.3f' % kv for kv in sorted(share.items()))))
        # the frames a target skips: float32 and float64 agree through the whole recursion, not only step by step
        v64, v32 = EM.refine(E, X, c['n'], np.float64)[0], EM.refine(E, X, c['n'], np.float32)[0]
        assert np.array_equal(v64 == 0, v32 == 0)
    print('so far, over the cells: %s' % ', '.join('%s %.3f' % kv for kv in sorted(SHARES.items())))


def test_the_bars_are_relative_to_the_element(problems):
    """The filter's bar on the weak-target cell, relative to the element of the reference it belongs to: the same for the weak
    target as for the others -- and the evaluation inside the bars agrees with the restatements it stands beside."""
    E, X = problems['weak80'][0]
    R = C.model_cov(E)
    ref = SR.spatial_filter(E, X, np.float64, R=R)
    bar_re, bar_im, ok, value = C.bar_filter(C.q_powers(E), R, X)
    assert ok.all()
    assert np.abs(value - ref).max() <= 1e-9 * np.abs(ref).max() and np.allclose(value, ref, rtol=1e-7, atol=0)
    rel = np.hypot(bar_re, bar_im) / np.abs(ref)
    med = [float(np.median(rel[i])) for i in range(3)]
    print('weak80: median bar / |reference| per target %s; max |weak target| / max|X| %.3g' %
          (['%.3g' % m for m in med], np.abs(ref[2]).max() / np.abs(X).max()))
    assert max(med) < 1e-4 and med[2] < 4 * max(med[:2])
    v32 = SR.powers(E, np.float32)
    plain, hooked = C.model_em_step(v32, R, X), C.model_em_step(v32, R, X, close=C.em_close)
    assert plain[0].tobytes() == hooked[0].tobytes() and plain[1].tobytes() == hooked[1].tobytes(), 'em_close is step 2 of EM.em_step'
    vref, Rref, use = C.reference_em_step(v32, R, X)
    bar, ok, value = C.bar_em_powers(C.q_powers(E), R, X)
    assert np.allclose(value, vref, rtol=1e-5, atol=0)         # q_powers starts from E, vref from the float32 powers: 7 u apart
    bar_c, okc, value = C.bar_em_cov(C.q_powers(E), R, X, use)
    assert np.allclose(value, Rref, rtol=1e-5, atol=1e-9)
    print('weak80: largest EM bar: powers %.0f u of the element, covariances %.0f u' % ((bar / vref).max() / C.U, bar_c.max() / C.U))


# mistake -> [(cell, target)]: the cells on which the bars must catch it
PLANTED = {
    'flip_im':    [('weak80', 2), ('weak40', 5)],        # the sign of Im R~01 of one (the weak) target, in the filter
    'drop_sigma': [('weak40', 5), ('weak40_soft', 1)],   # the weak target left out of Sigma
    'zero_weak':  [('weak80', 2), ('weak40', 5)],        # the weak target's output written as 0
    'drop128':    [('zero_bin', 0), ('zero_frame', 0)],  # frames >= 128 of a row left out of the covariance sums
    'odd_twice':  [('weak80', 0), ('zero_bin', 0)],      # the odd last frame counted twice
    'r_first':    [('uniform', 0), ('absent', 0)],       # R~ updated before the powers within an iteration
    'power':      [('uniform', 0), ('absent', 0)],       # the power-weighted covariance
    'lambda':     [('zero_bin', 0), ('weak40', 0)],      # the EM loading applied as lambda, not lambda 1/2 tr R'
    'count_all':  [('zero_frame', 0), ('absent', 0)],    # a skipped frame counted in cnt
}


@pytest.mark.parametrize('mistake', sorted(PLANTED))
def test_planted_mistakes_fail(problems, mistake):
    assert set(PLANTED) == set(C.MISTAKES)
    for name, target in PLANTED[mistake]:
        c = C.CELLS[name]
        E, X = problems[name][c['pos']]
        fail, _, share = C.check_cell(C.model_stages(E, X, c['n'], mistake, target), name)
        print('%s on %s: %d failures, up to %.3g of a bar' % (mistake, name, len(fail), max(share.values())))
        assert any('of the bar' in f or 'exact zeros' in f or 'zero pattern' in f for f in fail), (mistake, name)


def test_the_scalar_bar_does_not_see_the_weak_target(problems):
    """For the record: the bar of tests/test_gpu_spatial_reconstruction.py (SR.measured_bar, one number relative to max|X|) passes
    both weak-target mistakes on the weak-target cell -- the gap the derived bars close."""
    E, X = problems['weak80'][0]
    bar, err32, ref = SR.measured_bar(E, X)
    scale = float(np.abs(X).max())
    print('weak80: scalar bar %.3g of max|X|; the weak target\'s whole output %.3g of max|X|' % (bar, np.abs(ref[2]).max() / scale))
    assert np.abs(ref[2]).max() / scale < bar / 100
    for mistake in ('zero_weak', 'drop_sigma'):
        out = C.model_stages(E, X, 0, mistake, 2)['out'][0]
        dist = float(np.abs(out - ref).max()) / scale
        print('  %s: %.3g of max|X|, %.2f of the scalar bar' % (mistake, dist, dist / bar))
        assert dist <= bar
    fail, _, _ = C.check_cell(C.model_stages(E, X, 0, 'zero_weak', 2), 'weak80')
    assert fail
