"""CPU checks of tests/tracks_stage_cases.py, the inputs and expected values of tests/test_gpu_tracks_stages.py: the tables cover the
shapes, window alignments and scan patterns they are there for, every case is non-trivial, and every comparison is sensitive -- each
plausible mistake of the kernels (a window off by one frame, a window rounded to its 16-byte group, the wrong half, the wrong carry,
the wrong tie rule, a neighbouring frame's steering index), evaluated in NumPy on the very inputs of the GPU tests, gives something else
than the expected values."""
import numpy as np
import pytest

import gcc_checks as C
import tdoa_tracks_restatement as R
import tracks_stage_cases as TC
from gcc_stage_inputs import CELLS, CELL_IDS, cell_seed, host_file
from oracle import gccnmf_oracle as O

CASES = range(len(TC.TRACK_CASES))


def evaluate(A, S, L, bounds=R.window_bounds, carry='previous', ties='larger', denominator=None):
    """The tracks stage with its rules as parameters -> (tracks, status, Abar).  The window sums come from one cumulative sum: on these
    inputs every partial sum is exact, so this is the restatement's windowed mean bit for bit (test_window_sums_are_exact_in_any_order)."""
    A = np.asarray(A, np.float64)
    D, T = A.shape
    cs = np.concatenate([np.zeros((D, 1)), np.cumsum(A, axis=1)], axis=1)
    Abar = np.empty((D, T))
    for t in range(T):
        lo, hi = bounds(t, L, T)
        own_lo, own_hi = R.window_bounds(t, L, T)
        Abar[:, t] = (cs[:, hi] - cs[:, lo]) / float(denominator(L) if denominator else own_hi - own_lo)
    i = np.arange(1, D - 1)
    own = []
    for t in range(T):
        v = Abar[:, t]
        peaks = i[(v[i] > v[i - 1]) & (v[i] > v[i + 1])]
        if ties == 'smaller':
            peaks = peaks[::-1]
        keep = sorted(int(p) for p in peaks[np.argsort(v[peaks], kind='stable')[-S:]])
        own.append(keep if len(keep) == S else None)
    complete = [t for t in range(T) if own[t] is not None]
    if not complete:
        return np.full((S, T), -1, np.int32), np.full(T, 3, np.int32), Abar
    tracks, status = np.zeros((S, T), np.int32), np.zeros(T, np.int32)
    last = None
    for t in range(T):
        if carry == 'reset' and t % TC.STEP == 0:
            last = None
        if own[t] is not None:
            last = src = t
        else:
            status[t] = 1
            src = complete[0] if last is None else last
            if carry == 'next' and t > complete[0]:
                later = [u for u in complete if u > t]
                src = later[0] if later else last
        tracks[:, t] = own[src]
    return tracks, status, Abar


def mutant_hits(**rules):
    """The cases in which the stage under other rules gives other tracks or status than expected() in some file."""
    hits = []
    for case in CASES:
        D, T, S, L, batch, kind = TC.TRACK_CASES[case]
        for pattern, A, tracks, status in TC.case_files(case):
            got_tracks, got_status, _ = evaluate(A, S, L, **rules)
            if not (np.array_equal(got_tracks, tracks) and np.array_equal(got_status, status)):
                hits.append(TC.TRACK_IDS[case])
                break
    return hits


def test_window_sums_are_exact_in_any_order():
    """Every element is a multiple of 2^-10 in [0, 4): the restatement's ascending sums, a descending sum and a difference of cumulative
    sums agree in every bit, and so do the tracks -- the order of summation cannot matter to these cases."""
    for case in CASES:
        D, T, S, L, batch, kind = TC.TRACK_CASES[case]
        for pattern, A, tracks, status in TC.case_files(case):
            assert A.dtype == np.float32 and A.shape == (D, T)
            assert np.array_equal(A * 1024, np.round(A * 1024)) and A.min() >= 0 and A.max() < 4
            assert (A > 0).all() or kind == 'levels'
            want_tracks, want_status, Abar = TC.expected(A, S, L)
            assert np.array_equal(want_tracks, tracks) and np.array_equal(want_status, status)
            got_tracks, got_status, got = evaluate(A, S, L)
            assert np.array_equal(got, Abar) and np.array_equal(got_tracks, tracks) and np.array_equal(got_status, status)
            back = np.stack([A[:, lo:hi][:, ::-1].astype(np.float64).cumsum(axis=1)[:, -1] / (hi - lo)
                             for lo, hi in (R.window_bounds(t, L, T) for t in range(T))], axis=1)
            assert np.array_equal(back, Abar), TC.TRACK_IDS[case]


def test_tables_cover_every_alignment_truncation_and_listed_value():
    pairs, truncated = set(), set()
    for D, T, S, L, batch, kind in TC.TRACK_CASES:
        for lo, hi in TC.window_pairs(T, L):
            pairs.add((lo % 4, hi % 4))
        for t in range(T):
            left, right = t - L // 2 < 0, t - L // 2 + L > T
            truncated.add(('left' if left else '') + ('right' if right else ''))
    print('window alignments (lo %% 4, hi %% 4) covered: %d of 16' % len(pairs))
    assert len(pairs) == 16
    assert truncated >= {'', 'left', 'right', 'leftright'}
    col = lambda j: {c[j] for c in TC.TRACK_CASES}
    assert col(0) >= {3, 4, 63, 64, 65, 200, 4096}
    assert all(T <= 5 for D, T, S, L, batch, kind in TC.TRACK_CASES if D == 4096)
    assert col(1) >= {1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513, 700}
    assert col(3) >= {1, 2, 3, 4, 5, 7, 8, 48, TC.RAW_L} and TC.RAW_L == 2 ** 22 - 1
    assert any(L == 2 * T - 2 for D, T, S, L, batch, kind in TC.TRACK_CASES)
    assert any(L == 2 * T - 1 for D, T, S, L, batch, kind in TC.TRACK_CASES)
    assert col(2) == {1, 2, 3, 7, 255} and all(D >= 600 for D, T, S, L, batch, kind in TC.TRACK_CASES if S == 255)
    assert col(4) == {1, 3, 6, 64}
    assert col(5) == {'levels', 'grid'}
    assert all(TC.file_patterns(T, L, batch) == TC.SIX_PATTERNS for D, T, S, L, batch, kind in TC.TRACK_CASES if batch == 6)
    assert len(set(TC.TRACK_IDS)) == len(TC.TRACK_CASES)


def test_every_case_is_non_trivial():
    seen = set()
    for case in CASES:
        D, T, S, L, batch, kind = TC.TRACK_CASES[case]
        files = TC.case_files(case)
        assert len(files) == batch
        for pattern, A, tracks, status in files:
            seen.add(pattern)
            assert tracks.shape == (S, T) and status.shape == (T,)
            assert TC.is_of_pattern(pattern, T, L, tracks, status), (TC.TRACK_IDS[case], pattern)
            if pattern == 'normal' and T >= 2 and not TC.whole_file(T, L):
                assert (status == 0).any() and (status == 1).any(), TC.TRACK_IDS[case]
                assert T < 8 or len({tuple(c) for c in tracks.T.tolist()}) >= 2, TC.TRACK_IDS[case]
            if pattern == 'normal':
                assert (tracks >= 1).all() and (tracks <= D - 2).all() and (np.diff(tracks, axis=0) > 0).all()
            if pattern == 'none':
                assert (status == 3).all() and (tracks == -1).all()
            if pattern == 'only_first':
                assert np.flatnonzero(status == 0).tolist() == [0]
            if pattern == 'only_last':
                assert np.flatnonzero(status == 0).tolist() == [T - 1]
            if pattern == 'step_edge':
                done = np.flatnonzero(status == 0).tolist()
                assert 255 in done and min(t for t in done if t > 255) >= (256 + 300 if T > 556 else T - 1)
                assert tracks[:, 255].tolist() != tracks[:, done[0]].tolist()          # a carry lost at frame 256 shows
            if pattern == 'after_step':
                assert np.flatnonzero(status == 0).tolist() == [256, 257]
        if S == 255:
            assert (files[0][3] != 0).mean() > 0.5                                    # most frames are short
        if batch > 1:                                                                 # the files of a batch differ
            assert len({A.tobytes() for _, A, _, _ in files}) == batch
        if T >= 4 * TC.STEP:                                                          # the gap spans two whole steps and more
            gap = np.flatnonzero(files[0][3][TC.STEP:4 * TC.STEP] == 0)
            assert len(gap) == 0 and (files[0][3][:TC.STEP] == 0).any() and (files[0][3][4 * TC.STEP:] == 0).any()
    assert seen == set(TC.SIX_PATTERNS)
    # the only complete frame at 255 and at 256 (the last frame of the scan's first step, the first of its second)
    only = {(T, np.flatnonzero(st == 0).tolist()[0]) for case in CASES for p, A, tr, st in TC.case_files(case) if p == 'only_last'
            for T in [TC.TRACK_CASES[case][1]]}
    assert {(256, 255), (257, 256)} <= only


def test_levels_tie_at_the_S_boundary():
    """In some frame of the levels cases the S-th and the (S + 1)-th peak have one height: the tie rule decides the tracks."""
    ties = 0
    for case in CASES:
        D, T, S, L, batch, kind = TC.TRACK_CASES[case]
        if kind != 'levels':
            continue
        for pattern, A, tracks, status in TC.case_files(case):
            Abar = R.windowed_mean(A, L)
            for t in np.flatnonzero(status == 0):
                v = Abar[:, t]
                i = np.arange(1, D - 1)
                h = np.sort(v[i[(v[i] > v[i - 1]) & (v[i] > v[i + 1])]])
                ties += len(h) > S and h[-S] == h[-S - 1]
    assert ties >= 20


MUTANTS = {
    'the window starts at lo - 1': dict(bounds=lambda t, L, T: (max(0, R.window_bounds(t, L, T)[0] - 1), R.window_bounds(t, L, T)[1])),
    'the window ends at hi + 1': dict(bounds=lambda t, L, T: (R.window_bounds(t, L, T)[0], min(T, R.window_bounds(t, L, T)[1] + 1))),
    'the window starts at lo & ~3': dict(bounds=lambda t, L, T: (R.window_bounds(t, L, T)[0] & ~3, R.window_bounds(t, L, T)[1])),
    '(L + 1) // 2 in place of L // 2': dict(bounds=lambda t, L, T: (max(0, t - (L + 1) // 2), min(T, t - (L + 1) // 2 + L))),
    'the carry comes from the next complete frame': dict(carry='next'),
    'the carry is reset at every multiple of 256': dict(carry='reset'),
    'the smaller index is kept among equal heights': dict(ties='smaller'),
}


@pytest.mark.parametrize('name', list(MUTANTS))
def test_the_tracks_comparison_catches(name):
    hits = mutant_hits(**MUTANTS[name])
    print('%s: other tracks or status in %d of %d cases (%s)' % (name, len(hits), len(TC.TRACK_CASES), ', '.join(hits)))
    assert hits


def test_division_by_L_changes_every_truncated_mean_and_no_track():
    """Division by L in place of the window's own length scales a frame's means by one positive factor.  The peak rule is invariant
    under that, and the means never leave the device's LDS, so neither tracks nor status can tell -- by construction, not by a gap in
    the cases.  expected() returns the means as well, and there this mutant differs in every truncated window."""
    differ = 0
    for case in CASES:
        D, T, S, L, batch, kind = TC.TRACK_CASES[case]
        for pattern, A, tracks, status in TC.case_files(case):
            got_tracks, got_status, got = evaluate(A, S, L, denominator=lambda L: L)
            Abar = TC.expected(A, S, L)[2]
            cut = np.array([hi - lo != L for lo, hi in (R.window_bounds(t, L, T) for t in range(T))])
            assert cut.any() or L <= T
            moved = (got != Abar).any(axis=0)
            assert np.array_equal(moved, cut & (Abar != 0).any(axis=0)), TC.TRACK_IDS[case]
            differ += int(moved.any())
            assert np.array_equal(got_tracks, tracks) and np.array_equal(got_status, status)
    assert differ >= len(TC.TRACK_CASES) - 1


# ---- the score stage's per-frame indexes --------------------------------------------------------------------------------------------

def test_index_tracks_draw_afresh_every_frame():
    for F, D, S, K, T, batch, key2, key3 in CELLS:
        tracks, slots, pal = TC.index_tracks(D, T, S, 5)
        assert tracks.dtype == np.int32 and tracks.shape == (S, T) and pal.shape == (S, 3)
        assert np.array_equal(tracks, np.take_along_axis(pal, slots, axis=1))
        for i in range(S):
            assert len(set(pal[i].tolist())) == 3 and {0, D - 1} < set(pal[i].tolist()) and 0 <= pal[i].min() and pal[i].max() < D
            assert (np.diff(tracks[i]) != 0).all()                                   # neighbouring frames never agree
            for g in range(0, T, 4):
                assert len(set(tracks[i, g:g + 4].tolist())) >= min(2, T - g)         # no aligned group is constant
        if S > 1:
            assert len({tuple(p) for p in pal.tolist()}) == S                         # a palette of its own per target
        if T >= 64:                                                                   # every two lanes of a group differ somewhere
            groups = tracks[:, :T - T % 4].reshape(S, -1, 4)
            for a in range(4):
                for b in range(a + 1, 4):
                    assert (groups[:, :, a] != groups[:, :, b]).any(axis=1).all(), (a, b)
        wild, clamped, slots2, pal2 = TC.index_tracks(D, T, S, 5, out_of_range=True)
        assert wild.dtype == np.int32 and np.array_equal(slots2, slots) and np.array_equal(pal2, pal)
        out = (wild < 0) | (wild >= D)
        assert out.any() and out[0, T - 1] and set(wild[out].tolist()) <= set(TC.OUT_OF_RANGE(D))
        assert np.array_equal(clamped, np.clip(wild.astype(np.int64), 0, D - 1)) and np.array_equal(wild[~out], tracks[~out])
    every = np.concatenate([TC.index_tracks(D, T, S, 5, out_of_range=True)[0].ravel() - np.array(TC.OUT_OF_RANGE(D))[:, None]
                            for F, D, S, K, T, batch, key2, key3 in CELLS], axis=1)
    assert (every == 0).any(axis=1).all()                                             # each of the six values occurs in some cell


@pytest.mark.parametrize('F,D,S,K,T,batch,key2,key3', list(CELLS), ids=CELL_IDS)
def test_a_neighbouring_frames_index_moves_the_scores(F, D, S, K, T, batch, key2, key3):
    """Frame t + 1's index used for frame t, and frame 4 (t // 4)'s used for its whole group, move the float64 scores of every column
    whose index they change by more than 100 times the bound the GPU test allows.  (T = 1: one frame, both are the identity.)"""
    f = host_file(F, T, K, D, S, cell_seed(F, K, 0))
    freqs, tdoas = O.getFrequenciesInHz(16000, F), O.getTDOAsInSeconds(1.0, D)
    tracks = TC.index_tracks(D, T, S, cell_seed(F, K, 0))[0]
    G, Gabs = R.target_scores(f['C'], f['W'], freqs, tdoas, tracks)
    bound = C.gemm_bound(Gabs, F)
    t = np.arange(T)
    for name, other in (('next frame', tracks[:, np.minimum(t + 1, T - 1)]), ('first of the group', tracks[:, 4 * (t // 4)])):
        changed = other != tracks
        if T == 1:
            assert not changed.any()
            continue
        assert changed.any(axis=1).all()
        share = np.abs(R.target_scores(f['C'], f['W'], freqs, tdoas, other)[0] - G) / bound            # (S, K, T)
        worst = share.max(axis=1)
        print('%s: %d columns changed, their largest share of the bound between %.3g and %.3g' % (name, int(changed.sum()),
                                                                                               worst[changed].min(), worst[changed].max()))
        assert (worst[changed] > 100).all() and not worst[~changed].any()
