"""NumPy restatement of the offline time-varying TDOA tracks (GCCNMFEngine(tdoaTracking=True)) -- the offline twin of
the streaming multiple-mode rule.  The reference pools the angular spectrogram over the whole file
(gccNMF/runGCCNMF.py:46-48) and has nothing to compare with, so these formulas are the specification.  Test infrastructure, not the
product (never imported by the package).

Given A[tau, t] (PHAT or GCC-NONLIN), S sources and a window of L frames:
  1. windowed mean   Abar[tau, t] = mean(A[tau, lo:hi]), lo = max(0, t - L // 2), hi = min(T, t - L // 2 + L); a truncated window divides
                     by its own length; frames are added in ascending order (float64 in the restatement)
  2. peaks           the unchanged peak rule on Abar[:, t]: strict local maxima, edges excluded, the S largest, the larger index among
                     equal heights, ascending
  3. short frames    a frame with fewer than S peaks takes the previous frame's set and status 1; the frames in front of the first
                     complete frame take that frame's set (status 1 too); no complete frame at all is an error
  4. identity        target i of a frame is its i-th peak from the left: talkers whose directions cross swap outputs
  5. scores          G_i[k, t] = Re sum_f W[f, k] C[f, t] exp(-2j pi f tau_{i, t})
  6. L >= 2T - 1     every window is the whole file: constant tracks, equal to the whole-file estimate

``dtype=np.float32`` evaluates the sums of step 1 in float32 instead: the distance between the two evaluations is what the GPU tests'
bar on the windowed mean is measured from (BAR_FACTOR x, ``measured_bar``)."""
import numpy as np

from gcc_checks import expected_peaks

BAR_FACTOR = 4.0            # as in section 4a: a different summation order on top of the float32 evaluation's error


def window_bounds(t, L, T):
    lo = max(0, t - L // 2)
    return lo, min(T, t - L // 2 + L)


def windowed_mean(A, L, dtype=np.float64):
    """Abar (D, T) in ``dtype``: for every frame the sum of its window's frames in ascending order over the window's own length."""
    A = np.asarray(A)
    D, T = A.shape
    out = np.zeros((D, T), dtype)
    done = {}                                                           # frames that share a window (L >= 2T - 1: all of them) share the sum
    for t in range(T):
        lo, hi = window_bounds(t, int(L), T)
        if (lo, hi) not in done:
            s = np.zeros(D, dtype)
            for u in range(lo, hi):
                s = s + A[:, u].astype(dtype)
            done[(lo, hi)] = s / dtype(hi - lo)
        out[:, t] = done[(lo, hi)]
    return out


def tracks_from_means(Abar, numSources):
    """Steps 2 and 3 on windowed means (D, T) -> (tracks (S, T) int, status (T,) int: 0 = own peaks, 1 = another frame's set).
    ValueError when no frame has ``numSources`` peaks."""
    Abar = np.asarray(Abar, np.float64)
    D, T = Abar.shape
    S = int(numSources)
    own = [expected_peaks(Abar[:, t], S) for t in range(T)]
    complete = [t for t in range(T) if own[t][1] == 0]
    if not complete:
        raise ValueError('no frame has %d peaks' % S)
    tracks, status = np.zeros((S, T), np.int64), np.zeros(T, np.int64)
    last = complete[0]
    for t in range(T):
        if own[t][1] == 0:
            last = t
        else:
            status[t] = 1
        tracks[:, t] = own[last][0]
    return tracks, status


def tdoa_tracks(A, numSources, L):
    """(tracks (S, T), status (T,), Abar float64) of one angular spectrogram."""
    Abar = windowed_mean(A, L)
    tracks, status = tracks_from_means(Abar, numSources)
    return tracks, status, Abar


def measured_bar(A, L):
    """(bar, float32 error, Abar float64): the bar on the windowed mean is BAR_FACTOR x the largest distance of the float32 evaluation
    of the same sums from the float64 one."""
    A64 = windowed_mean(A, L, np.float64)
    A32 = windowed_mean(A, L, np.float32)
    err = float(np.abs(A32.astype(np.float64) - A64).max())
    return BAR_FACTOR * err, err, A64


def frame_margin(v, numSources, slack=0.0):
    """How far a frame's decision is from changing under a perturbation of every sample by up to ``slack`` / 2: the height of the S-th
    chosen peak over the best peak left out (the gap of a tie when they are equal), and the gap of every comparison between neighbours
    that could make a peak of the chosen heights appear or vanish (pairs that reach within ``slack`` of the S-th chosen height; all
    pairs in a frame with fewer than S peaks).  A frame whose margin exceeds ``slack`` keeps its set."""
    v = np.asarray(v, np.float64)
    S = int(numSources)
    i = np.arange(1, len(v) - 1)
    peaks = i[(v[i] > v[i - 1]) & (v[i] > v[i + 1])]
    h = np.sort(v[peaks])
    floor = h[-S] - slack if len(peaks) >= S else -np.inf
    pair_top = np.maximum(v[:-1], v[1:])
    gaps = np.abs(np.diff(v))[pair_top >= floor]
    margin = float(gaps.min()) if len(gaps) else np.inf
    if len(peaks) > S:
        margin = min(margin, float(h[-S] - h[-S - 1]))
    return margin


def steering(frequenciesInHz, tdoasInSeconds):
    return np.exp(np.outer(np.asarray(frequenciesInHz, np.float64), -(2j * np.pi) * np.asarray(tdoasInSeconds, np.float64)))     # (F, D)


def target_scores(C, W, frequenciesInHz, tdoasInSeconds, tracks):
    """Step 5: G (S, K, T) float64 and the sum of |W| |P| per element (the bound of tests/gcc_checks.py) for per-frame indexes."""
    C = np.asarray(C, np.complex128)
    W = np.asarray(W, np.float64)
    E = steering(frequenciesInHz, tdoasInSeconds)
    tracks = np.asarray(tracks)
    G, Gabs = [], []
    for i in range(tracks.shape[0]):
        e = E[:, tracks[i]]                                              # (F, T): each frame its own column
        G.append(np.dot(W.T, (C * e).real))
        Gabs.append(np.dot(np.abs(W).T, np.abs(C.real) * np.abs(e.real) + np.abs(C.imag) * np.abs(e.imag)))
    return np.array(G), np.array(Gabs)


def image_sdr(estimate, image, windowSize, first, last, guard=4000):
    """SDR (dB) of a separated left channel against a source's left-channel image over samples [first, last) of the MIXTURE, ``guard``
    samples left out at both ends.  The separated waveform starts windowSize / 2 samples into the mixture (the centred inverse STFT
    trims that much): estimate[n] belongs to image[n + windowSize / 2]."""
    off = windowSize // 2
    a, b = first + guard, last - guard
    ref = np.asarray(image, np.float64)[a:b]
    est = np.asarray(estimate, np.float64)[a - off:b - off]
    return 10.0 * np.log10(np.sum(ref ** 2) / np.sum((ref - est) ** 2))
