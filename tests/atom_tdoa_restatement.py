"""float64 NumPy restatement of the two offline-enhancement stages (include/gccnmf_hip.h: GCCNMF_ATOM_TDOA_INDEXES and
GCCNMF_ENHANCEMENT_MASKS, csrc/atom_tdoa.hip), evaluated on the float32 inputs the device sees:

    score[k, d, t] = sum_f W[f, k] (Cr[f, t] cos[f, d] + Ci[f, t] sin[f, d])
    index[k, t]    = argmax_d score[k, d, t]      first index wins an exact tie, NaN ignored, an all-NaN column gives 0
    boxcar         m = |i - target| < eps
    window         m = exp(-(|i - target| / eps) ** beta) / (1 + nf) + nf          masks = (m, 1 - m)

Nothing here knows about the device: it is the contract the kernels are tested against."""
import numpy as np


def nan_argmax_first(S, axis):
    """arg-max along ``axis`` ignoring NaN, the first index on ties, 0 where every entry is NaN."""
    S = np.asarray(S, np.float64)
    filled = np.where(np.isnan(S), -np.inf, S)
    idx = np.argmax(filled, axis=axis)                       # numpy.argmax returns the first maximum
    return np.where(np.isnan(S).all(axis=axis), 0, idx)


def scores(C, cos, sin, W, frames=None):
    """C (F, T) complex, cos / sin (F, D), W (F, K), all read as they are (float32 values) -> (S64 (K, D, T), Sabs (K, T)) float64,
    Sabs[k, t] = max_d sum_f |W[f, k]| |Cr cos + Ci sin|.  ``frames``: evaluate only these columns."""
    C = np.asarray(C)
    Cr, Ci = np.asarray(C.real, np.float64), np.asarray(C.imag, np.float64)
    if frames is not None:
        Cr, Ci = Cr[:, frames], Ci[:, frames]
    cos, sin, W = np.asarray(cos, np.float64), np.asarray(sin, np.float64), np.asarray(W, np.float64)
    K, D, T = W.shape[1], cos.shape[1], Cr.shape[1]
    S64, Sabs = np.empty((K, D, T)), np.zeros((K, T))
    for d in range(D):
        G = Cr * cos[:, d:d + 1] + Ci * sin[:, d:d + 1]      # (F, T)
        S64[:, d, :] = W.T.dot(G)
        with np.errstate(invalid='ignore'):
            Sabs = np.fmax(Sabs, np.abs(W).T.dot(np.abs(G)))
    return S64, Sabs


def atom_tdoa(C, cos, sin, W):
    """-> (index (K, T) int64, S64, Sabs)."""
    S64, Sabs = scores(C, cos, sin, W)
    return nan_argmax_first(S64, axis=1), S64, Sabs


def brute_force_index(C, cos, sin, W):
    """The same rule as loops over (k, t, d, f): the check of the vectorised form on a tiny case."""
    F, T = C.shape
    K, D = W.shape[1], cos.shape[1]
    out = np.zeros((K, T), np.int64)
    for k in range(K):
        for t in range(T):
            best, have = 0.0, False
            for d in range(D):
                s = 0.0
                for f in range(F):
                    s += float(W[f, k]) * (float(C[f, t].real) * float(cos[f, d]) + float(C[f, t].imag) * float(sin[f, d]))
                if s != s:
                    continue
                if not have or s > best:
                    best, have, out[k, t] = s, True, d
    return out


def masks(index, target, window, eps, beta=2.0, nf=0.0):
    """index (K, T) whole numbers, target a number or (T,), parameters as float32 values -> (image (K, T) uint8: 0 talker, 1 noise;
    masks (2, K, T) float64 [talker, noise])."""
    eps, beta, nf = [float(np.float32(v)) for v in (eps, beta, nf)]
    dist = np.abs(np.asarray(index, np.float64) - np.asarray(target, np.float64))
    talker = dist < eps
    m = np.exp(-(dist / eps) ** beta) / (1 + nf) + nf if window else talker.astype(np.float64)
    return np.where(talker, 0, 1).astype(np.uint8), np.stack([m, 1 - m])


def sdr(estimate, reference):
    return 10 * np.log10(np.sum(reference ** 2) / np.sum((estimate - reference) ** 2))


def float64_enhancement(x, clean, K=64, iterations=100, D=128, eps=4.0, window=0, beta=2.0, nf=0.0, ws=1024, hop=256, sampleRate=16000):
    """The whole pipeline on the CPU (the oracle's STFT / KL-NMF / iSTFT, the restatement's two stages, the ratio-mask restatement).
    SDR is taken against the clean talker passed through the same STFT / iSTFT pair (the analysis is un-centred, the synthesis trims).
    -> (input SDR, output SDR, target index)"""
    import ratio_restatement as R
    from oracle import gccnmf_oracle as O
    X = O.computeComplexMixtureSpectrogram(x, ws, hop, np.hanning).astype(np.complex128)
    F, T = X.shape[1:]
    V = np.concatenate(np.abs(X), axis=-1)
    W, H = O.performKLNMF(V, K, iterations, 0)
    C = O.spectralCoherence(X)
    f = O.getFrequenciesInHz(sampleRate, F)
    E = np.exp(np.outer(f, -(2j * np.pi) * O.getTDOAsInSeconds(1.0, D)))
    idx = atom_tdoa(C, E.real, -E.imag, W)[0]
    ang = O.getAngularSpectrogram(C, f, 1.0, D)
    target = int(np.argmax(np.nanmean(ang, axis=-1)))
    spec = R.ratio_soft(W, H, masks(idx, target, window, eps, beta, nf)[1], X)
    back = lambda S: np.array([O.istft(S[c].astype(np.complex64), hop, ws, np.hanning) for c in range(2)]).astype(np.float64)
    ref = back(O.computeComplexMixtureSpectrogram(clean.astype(np.float32), ws, hop, np.hanning))
    return sdr(back(X), ref), sdr(back(spec[0]), ref), target
