"""Inputs, case tables and expected values of the stage tests of the time-varying TDOA tracks (tests/test_gpu_tracks_stages.py: the
tracks mode of gccnmf_pick_tdoa_peaks and the per-frame indexes of gccnmf_target_scores_masks).  Plain NumPy -- no
torch, no device -- so that the CPU suite (tests/test_tracks_stage_cases_host.py) can show that the tables cover what they claim and
that the comparisons are sensitive.  Test infrastructure, not the product (never imported by the package).

The angular spectrograms are built so that summation order cannot matter: every element is a multiple of 2^-10 below 4, so a window
sum of up to 2^21 frames is exact in float64 whatever the order, only the division by the window's length rounds, and two different
sums over one length give quotients a relative 2^-22 or more apart.  Every comparison of tracks and status is therefore exact, with no
frame left out.  (Summation order on real spectrograms stays with test_tracks_equal_the_restatement and its measured bar.)

Two kinds of spectrogram:
  levels  heights in {0, 1, 2, 3} on odd rows: ties at the S boundary, frames with 0 to S + 1 peaks and leading frames without peaks
          are all common
  grid    every element a random multiple of 2^-10 in (0, 4), no zeros: a frame wrongly let into a window, or left out of it, changes
          that window's mean.  A frame that is to have no peak holds the same kind of values in ascending order (a sum of ascending
          columns has no strict local maximum)
"""
import functools

import numpy as np

import tdoa_tracks_restatement as R

RAW_L = (1 << 22) - 1                    # the largest window the mode word carries (bits 9-30); _hip.peaks_tracks_word would cap it
STEP = 256                               # frames per step of track_carry_kernel

# (D, T, S, L, batch, kind).  The patterns of a batch's files: file_patterns().
TRACK_CASES = [
    (3, 5, 1, 2, 1, 'grid'),             # the smallest D; one candidate peak
    (4, 4, 1, 7, 3, 'grid'),             # L = 2T - 1: the whole file
    (65, 1, 1, 1, 1, 'grid'),            # one frame
    (200, 2, 2, 3, 3, 'levels'),         # L = 2T - 1
    (4096, 3, 7, 4, 1, 'levels'),        # the largest D (dynamic LDS 8 D + 16 + D); L = 2T - 2
    (4096, 5, 3, 8, 1, 'grid'),          # L = 2T - 2
    (63, 4, 2, RAW_L, 1, 'levels'),      # the raw word's largest L
    (63, 63, 2, 125, 1, 'levels'),       # L = 2T - 1 over a file of some length: sums of many levels tie
    (64, 64, 3, 4, 1, 'grid'),
    (65, 65, 7, 5, 3, 'levels'),
    (64, 65, 3, 2, 64, 'levels'),        # 64 files whose patterns differ
    (640, 65, 255, 2, 1, 'levels'),      # the largest S: most frames are short
    (200, 255, 2, 3, 1, 'grid'),
    (200, 256, 3, 1, 3, 'levels'),       # the last file: the only complete frame at 255, the last frame of the scan's first step
    (65, 257, 2, 1, 3, 'grid'),          # the last file: the only complete frame at 256, alone in the second step
    (65, 257, 2, 48, 1, 'grid'),
    (64, 513, 2, 7, 1, 'levels'),
    (64, 700, 2, 1, 6, 'levels'),        # the six patterns
    (63, 700, 1, 1, 6, 'grid'),          # the six patterns
    (65, 700, 3, 48, 1, 'levels'),
    (64, 1100, 2, 5, 1, 'grid'),         # a gap that spans whole steps of the carry scan
]
TRACK_IDS = ['D%d-T%d-S%d-L%d-b%d-%s' % c for c in TRACK_CASES]

SIX_PATTERNS = ['normal', 'none', 'only_first', 'only_last', 'step_edge', 'after_step']


def file_patterns(T, L, batch):
    """The pattern of every file of a batch.  The patterns that name single complete frames need L = 1: a wider window lets every
    frame near a complete one see its peaks."""
    if batch == 1:
        return ['normal']
    if batch == 3:
        return ['normal', 'none', 'only_last' if L == 1 else 'normal']
    if batch == 6:
        assert L == 1 and T >= STEP + 2
        return list(SIX_PATTERNS)
    return ['none' if b in (5, 40) else 'normal' for b in range(batch)]


def complete_frames(pattern, T):
    """The frames a single-frame pattern makes complete (every other frame is short)."""
    if pattern == 'none':
        return []
    if pattern == 'only_first':
        return [0]
    if pattern == 'only_last':
        return [T - 1]
    if pattern == 'step_edge':           # 255, then nothing for 300 frames or more where T allows; an earlier set to tell a lost carry by
        return [7, STEP - 1, STEP + 300 if T > STEP + 300 else T - 1]
    if pattern == 'after_step':
        return [STEP, STEP + 1]
    raise ValueError(pattern)


def whole_file(T, L):
    return L >= 2 * T - 1


def _quiet_frames(T, L, pattern, rng):
    """Which frames hold no peak of their own (levels at L = 1: fewer than S)."""
    q = np.zeros(T, bool)
    if pattern != 'normal':
        q[:] = True
        q[complete_frames(pattern, T)] = False
        return q
    if T < 2 or whole_file(T, L):
        return q
    t = min(T - 1, L - L // 2 + rng.randint(0, 3))           # frame 0's window [0, L - L // 2) sees none
    q[:t] = True
    while t < T:
        t += rng.randint(1, max(3, min(L, 16)) + 1)           # a run of frames with peaks, then a run longer than a window without
        n = L + rng.randint(1, L + 3)
        q[t:t + n] = True
        t += n
    if T >= 4 * STEP:
        q[STEP - 6:T - 70] = True                             # the gap: steps 1, 2 and 3 of the scan hold no complete frame
    return q


def _draw(D, T, S, L, kind, pattern, seed):
    rng = np.random.RandomState(seed)
    quiet = _quiet_frames(T, L, pattern, rng)
    A = np.zeros((D, T), np.float32)
    if kind == 'grid':
        for t in range(T):
            col = rng.randint(1, 4096, D) / 1024.0
            A[:, t] = np.sort(col) if quiet[t] else col
        return A
    assert kind == 'levels'
    odd = np.arange(1, D - 1, 2)
    few = rng.choice(odd, size=min(S - 1, len(odd)), replace=False)          # 'none': the same S - 1 rows at most, in every frame
    for t in range(T):
        if pattern == 'none':
            pos = few[rng.rand(len(few)) < 0.7]
        elif quiet[t]:
            pos = rng.choice(odd, size=min(rng.randint(0, S), len(odd)), replace=False) if L == 1 else odd[:0]
        elif pattern == 'normal':
            pos = rng.choice(odd, size=min(rng.randint(0, S + 2), len(odd)), replace=False)
        else:
            pos = rng.choice(odd, size=min(S + rng.randint(0, 2), len(odd)), replace=False)
        A[pos, t] = rng.choice([1.0, 2.0, 3.0], size=len(pos))
    return A


def expected(A, S, L):
    """(tracks (S, T) int32, status (T,) int32, Abar (D, T) float64) of one angular spectrogram: the restatement, and status 3 with
    tracks -1 in every frame where it raises because no frame has S peaks."""
    A = np.asarray(A)
    Abar = R.windowed_mean(A, L)
    try:
        tracks, status = R.tracks_from_means(Abar, S)
    except ValueError:
        T = A.shape[1]
        return np.full((S, T), -1, np.int32), np.full(T, 3, np.int32), Abar
    return tracks.astype(np.int32), status.astype(np.int32), Abar


def is_of_pattern(pattern, T, L, tracks, status):
    """Whether a file is what its pattern promises.  A normal file has frames of status 0 and of status 1 and, from 8 frames on,
    tracks of two values or more -- except where every window is the whole file (or T = 1): there all frames share one mean, so the
    status is 0 throughout and the tracks are constant by definition."""
    if pattern == 'normal':
        if T < 2 or whole_file(T, L):
            return not status.any()
        moves = len({tuple(c) for c in tracks.T.tolist()}) >= 2
        return bool((status == 0).any() and (status == 1).any() and (moves or T < 8))
    if pattern == 'none':
        return bool((status == 3).all())
    return np.flatnonzero(status == 0).tolist() == sorted(set(complete_frames(pattern, T)))


def build_file(D, T, S, L, kind, pattern, seed):
    """(A, tracks, status) of one file of the pattern asked for: drawn again with another seed until it is."""
    for attempt in range(64):
        A = _draw(D, T, S, L, kind, pattern, seed + 7919 * attempt)
        tracks, status, _ = expected(A, S, L)
        if is_of_pattern(pattern, T, L, tracks, status):
            return A, tracks, status
    raise AssertionError('no %s file of pattern %s at D = %d, T = %d, S = %d, L = %d' % (kind, pattern, D, T, S, L))


@functools.lru_cache(maxsize=None)
def case_files(case):
    """[(pattern, A, tracks, status)] of the files of TRACK_CASES[case]; built once, shared, never changed (the arrays are read-only)."""
    D, T, S, L, batch, kind = TRACK_CASES[case]
    out = []
    for b, pattern in enumerate(file_patterns(T, L, batch)):
        A, tracks, status = build_file(D, T, S, L, kind, pattern, 100003 * case + 101 * b + 1)
        for a in (A, tracks, status):
            a.setflags(write=False)
        out.append((pattern, A, tracks, status))
    return out


def window_pairs(T, L):
    """{(lo, hi)} of the windows of a file."""
    return {R.window_bounds(t, L, T) for t in range(T)}


# ---- per-frame indexes for the score stage ------------------------------------------------------------------------------------------

OUT_OF_RANGE = lambda D: [-1, -5, D, D + 7, 2 ** 31 - 1, -2 ** 31]


def palettes(D, S):
    """(S, 3) int32: three indexes per target, 0 and D - 1 in every palette and a third of the target's own (D >= 3)."""
    assert D >= 3
    own = [1 + (37 * i + 11) % (D - 2) for i in range(S)]
    return np.array([[0, D - 1, own[i]][i % 3:] + [0, D - 1, own[i]][:i % 3] for i in range(S)], np.int32)


def index_tracks(D, T, S, seed, out_of_range=False):
    """Per-frame indexes for the score stage -> (tracks (S, T) int32, slots (S, T), palette (S, 3)): tracks[i, t] = palette[i, slots[i, t]].
    A target draws a slot afresh every frame, never the one it had in the frame before, so no two neighbouring frames of a target
    agree and no aligned group of four frames is constant.  out_of_range: about one entry in eight is replaced by a value outside
    [0, D) -> (tracks with those entries, the same clamped to [0, D), slots, palette)."""
    rng = np.random.RandomState(seed)
    pal = palettes(D, S)
    slots = np.zeros((S, T), np.int64)
    for i in range(S):
        s = rng.randint(0, 3)
        for t in range(T):
            s = (s + rng.randint(1, 3)) % 3
            slots[i, t] = s
    tracks = np.take_along_axis(pal, slots, axis=1).astype(np.int32)
    if not out_of_range:
        return tracks, slots, pal
    wild = tracks.astype(np.int64)
    hit = rng.rand(S, T) < 0.125
    hit[0, T - 1] = True                                                      # at least one, and in the last (partial) group
    wild[hit] = rng.choice(OUT_OF_RANGE(D), size=int(hit.sum()))
    return wild.astype(np.int32), np.clip(wild, 0, D - 1).astype(np.int32), slots, pal
