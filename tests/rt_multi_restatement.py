"""NumPy restatement of the real-time multi-target mode (TARGET_MODE_MULTIPLE; parity unpinned: the reference
defines the mode and never built it).  Test infrastructure, not the product.  Built on oracle.rt_oracle.GCCNMFProcessorOracle: its
windows, steering table ``expJOmegaTau``, float32 ``realGCC . W`` scores and coefficient inference."""
import numpy as np
from numpy.fft import rfft, irfft

from oracle import rt_oracle as R


def nanargmax_first(scores, axis=0):
    """Arg-max over ``axis`` with NaN ignored, the first index on ties, and 0 where every value is NaN."""
    s = np.where(np.isnan(scores), -np.inf, scores)
    idx = np.argmax(s, axis=axis)
    return np.where(np.all(np.isnan(scores), axis=axis), 0, idx)


def pick_peaks(values, n, previous):
    """The offline peak rule on a (D,) curve: strict local maxima, edges excluded, NaN never a peak; the n largest, the larger index
    kept among equal heights; ascending.  Fewer than n peaks: ``previous`` is returned unchanged."""
    v = np.asarray(values)
    D = len(v)
    with np.errstate(invalid='ignore'):
        peaks = [i for i in range(1, D - 1) if v[i] > v[i - 1] and v[i] > v[i + 1]]
    if len(peaks) < n:
        return np.asarray(previous).copy()
    order = sorted(peaks, key=lambda i: (v[i], i))          # ascending height, then index: the last n win, larger index on ties
    return np.array(sorted(order[-n:]), np.float32)


def window_mean_f32(hist, pos, L):
    """The localisation kernel's window mean in its float32 order: the last L columns of the [D][Lh] ring before write position
    ``pos``, newest first, NaN skipped, sum / count."""
    D, Lh = hist.shape
    out = np.full(D, np.nan, np.float32)
    for tau in range(D):
        s, cnt = np.float32(0), 0
        for j in range(1, L + 1):
            x = np.float32(hist[tau, (pos - j) % Lh])
            if x == x:
                s = np.float32(s + x)
                cnt += 1
        if cnt:
            out[tau] = np.float32(s / np.float32(cnt))
    return out


class MultiTargetOracle(object):
    """``base`` (a GCCNMFProcessorOracle) with N target TDOA indexes instead of one target window."""

    def __init__(self, base, targetTDOAIndexes):
        self.base = base
        self.targets = np.asarray(targetTDOAIndexes, np.float32)

    def scores(self, windowedSamples):
        """realGCC (F, Tc, D), the float32 GCC-NMF scores G (D, Tc, K) and the spectra X (2, F, Tc) of the base oracle."""
        b = self.base
        X = rfft(windowedSamples * b.windowFunction, axis=1).astype(np.complex64)
        coherenceV = X[0] * X[1].conj() / np.abs(X[0]) / np.abs(X[1])
        realGCC = (coherenceV[:, :, np.newaxis] * b.expJOmegaTau[:, np.newaxis]).real
        return X, realGCC, np.dot(realGCC.T, b.W)

    def decisions(self, G):
        """(K, Tc) target of every atom and frame, and the top-2 gap of the target scores relative to their magnitude."""
        tau = self.targets.astype(np.int64)
        Gt = G[tau]                                                      # (N, Tc, K)
        dec = nanargmax_first(Gt, axis=0).T
        if len(tau) > 1:
            srt = np.sort(np.where(np.isnan(Gt), -np.inf, Gt), axis=0)
            with np.errstate(invalid='ignore'):
                gap = (srt[-1] - srt[-2]) / np.maximum(np.abs(srt[-1]), np.abs(srt[-2]))
            gap = np.where(np.isfinite(gap), gap, np.inf).T
        else:
            gap = np.full(dec.shape, np.inf)
        return dec, gap

    def processFrames(self, windowedSamples, target_override=None, return_intermediates=False):
        """(2, windowSize, Tc) -> (N, 2, windowSize, Tc).  ``target_override`` (K, Tc): the per-atom target decisions of another
        implementation, so that the stages after a near-tie decision can be compared under that implementation's own decisions."""
        b = self.base
        N = len(self.targets)
        X, realGCC, G = self.scores(windowedSamples)
        dec, gap = self.decisions(G)
        if target_override is not None:
            dec = np.asarray(target_override).astype(np.int64)
        M = np.stack([(dec == i).astype(np.float64) for i in range(N)])  # (N, K, Tc) one-hot
        if b.separationEnabled:
            if b.numHUpdates == 0:
                recV = np.sum(b.W, axis=-1)
                tfMask = np.stack([(np.dot(b.W, M[i]).T / recV).T for i in range(N)])           # (N, F, Tc)
                Y = tfMask[:, np.newaxis] * X[np.newaxis]
            else:
                W64 = b.W.astype(np.float64)
                Hc = np.ones((2, b.numAtom, X.shape[2]))
                for c in range(2):
                    v = np.abs(X[c]).astype(np.float64)
                    for _ in range(b.numHUpdates):
                        Hc[c] *= np.dot(W64.T, R.ratio0(v, np.dot(W64, Hc[c]))) / np.sum(W64, axis=0)[:, np.newaxis]
                tfMask = np.stack([np.stack([R.ratio0(np.dot(W64, Hc[c] * M[i]), np.dot(W64, Hc[c])) for c in range(2)]) for i in range(N)])
                Y = tfMask * X[np.newaxis]
        else:
            tfMask = None
            Y = np.repeat(X[np.newaxis], N, axis=0)
        gccPHAT = np.nanmean(realGCC, axis=0).T
        b.gccPHATHistory.set(gccPHAT)
        if b.localizationEnabled:
            history = b.gccPHATHistory.getUnraveledArray()
            self.targets = pick_peaks(np.nanmean(history[:, -b.localizationWindowSize:], axis=-1), N, self.targets)
        out = irfft(Y, axis=2) * b.synthesisWindowFunction
        if return_intermediates:
            return out, dict(X=X, G=G, decisions=dec, gap=gap, HMask=M, tfMask=tfMask)
        return out


class MultiOverlapAdd(object):
    """rt_oracle.OverlapAddOracle with one output buffer per target."""

    def __init__(self, N, windowSize, hopSize, blockSize, outputDelayBlocks=2):
        self.olas = [R.OverlapAddOracle(2, windowSize, hopSize, blockSize, blockSize // hopSize, outputDelayBlocks) for _ in range(N)]

    def processFrames(self, block, processFramesFunction):
        """block (2, B) -> (N, 2, B); processFramesFunction maps (2, windowSize, Tc) to (N, 2, windowSize, Tc) and runs once."""
        frames = []
        first = self.olas[0].processFrames(block, lambda ws: frames.append(processFramesFunction(ws)) or frames[0][0])
        return np.stack([first] + [o.processFrames(block, lambda ws, i=i: frames[0][i]) for i, o in enumerate(self.olas) if i])
