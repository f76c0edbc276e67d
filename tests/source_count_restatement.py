"""The talker count of numSources='auto' (the count mode of gccnmf_pick_tdoa_peaks, csrc/source_count.hip),
restated in NumPy float64 -- a helper, not a test.  Every operation below is one IEEE float64 operation rounded on its own, in the order
the header states, so the device's result is compared with it exactly.

The rule is the reference's KMeans(n_clusters=2) on the peak heights (gccNMF/gccNMFFunctions.py:105-110) in its exact form: in one
dimension the two-cluster optimum is a threshold on the sorted values, and minimising the within-cluster sum of squares is maximising
b_j = c_j^2 / j + (c_P - c_j)^2 / (P - j) over the split position j."""
import numpy as np


def peak_indexes(v):
    """Strict local maxima (argrelmax, order 1: edges never, NaN never greater): the peaks of gcc_checks.expected_peaks."""
    v = np.asarray(v, np.float64)
    i = np.arange(1, len(v) - 1)
    return i[(v[i] > v[i - 1]) & (v[i] > v[i + 1])]


def split_scores(heights):
    """b_j, j = 1 .. P-1, for heights already in the rule's order; c_j by np.cumsum (sequential addition in that order)."""
    h = np.asarray(heights, np.float64)
    P = len(h)
    c = np.cumsum(h)
    j = np.arange(1, P)
    cj = c[:-1]
    r = c[-1] - cj
    with np.errstate(over='ignore'):
        return cj * cj / j.astype(np.float64) + r * r / (P - j).astype(np.float64)


def count_sources(v, Smax):
    """-> (indexes: the counted peaks in ascending order, padded with -1 to Smax; status 0 / 1 / 2)."""
    v = np.asarray(v, np.float64)
    peaks = peak_indexes(v)
    P = len(peaks)
    if P == 0:
        return [-1] * Smax, 1
    # height descending, the larger index first among equal heights: the reverse of the stable ascending sort of the fixed-count rule
    order = peaks[np.argsort(v[peaks], kind='stable')[::-1]]
    n = 1                                                                    # one peak is one talker, whatever its height
    if P > 1:
        with np.errstate(over='ignore', invalid='ignore'):
            total = np.cumsum(v[order])[-1]
        if not np.isfinite(total):
            return [-1] * Smax, 1
        n = 1 + int(np.argmax(split_scores(v[order])))                       # argmax: the first (smallest j) of equal maxima
    status = 2 if n > Smax else 0
    keep = sorted(int(p) for p in order[:min(n, Smax)])
    return keep + [-1] * (Smax - len(keep)), status


def kmeans_upper_cluster(v, **kmeans_args):
    """The reference's branch as written, with the import it lacks: the peaks KMeans(n_clusters=2) puts into the higher cluster."""
    from sklearn.cluster import KMeans
    v = np.asarray(v, np.float64)
    peaks = peak_indexes(v)
    km = KMeans(n_clusters=2, **kmeans_args).fit(v[peaks].reshape(-1, 1))
    upper = int(np.argmax(km.cluster_centers_.ravel()))
    return sorted(int(p) for p in peaks[km.labels_ == upper])
