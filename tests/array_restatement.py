"""float64 NumPy restatement of M-channel (microphone-array) GCC-NMF from the spectrogram X onwards (include/gccnmf_array.h,
gcc_nmf_amd/array.py).  Nothing here knows about the device or the package: it is the contract they are tested against.

    M channels, P = M (M - 1) / 2 pairs (a, b), a < b, lexicographic.  X (M, F, T) complex, X = conj(fft) as the STFT stores it.
    V[f, c T + t]   = |X_c[f, t]|
    C_p[f, t]       = X_a conj(X_b) / |X_a| / |X_b|,  (0, 0) where either magnitude is exactly zero
    tau[p][d]       = (r_b - r_a) . u_d / c                                         pair TDOAs in seconds
    ang[d, t]       = sum_p sum_f Re(C_p[f, t] e^{-2 pi j f tau[p][d]})             SRP-PHAT
    peaks           = the S largest strict local maxima of mean_t ang (gcc_checks.expected_peaks: the end points never qualify)
    G_i[k, t]       = sum_p sum_f W[f, k] Re(C_p[f, t] e^{-2 pi j f tau[p][d_i]})   scores; arg-max over i
    spec[i, c]      = X_c * (W.(H_c o M_i)) / den                                   ratio mask, H_c = H[:, c T:(c + 1) T]

Every sum also returns the sum of the moduli of its terms, which is what the element-wise bounds of gcc_checks scale with.
"""
import numpy as np

import fft_checks as K
import gcc_checks as C


def pairs(M):
    return [(a, b) for a in range(M) for b in range(a + 1, M)]


def azimuth_directions(numDirections, startDeg=0.0, stopDeg=180.0):
    """Unit vectors (cos az, sin az, 0) for numDirections azimuths from startDeg to stopDeg inclusive."""
    az = np.deg2rad(np.linspace(startDeg, stopDeg, numDirections))
    return np.stack([np.cos(az), np.sin(az), np.zeros_like(az)], axis=1)


def pair_tdoas_from_geometry(positions, directions, c):
    """tau[p][d] = (r_b - r_a) . u_d / c -> (P, D) float64."""
    r = np.asarray(positions, np.float64)
    u = np.asarray(directions, np.float64)
    return np.stack([(r[b] - r[a]).dot(u.T) / c for a, b in pairs(len(r))])


def features(X, pair_list=None):
    """X (M, F, T) complex64 -> V (F, M T), C (P, F, T) complex128."""
    X = np.asarray(X).astype(np.complex128)
    M, F, T = X.shape
    A = np.abs(X)
    V = np.concatenate([A[c] for c in range(M)], axis=1)
    pl = pairs(M) if pair_list is None else pair_list
    Cs = np.zeros((len(pl), F, T), np.complex128)
    for p, (a, b) in enumerate(pl):
        ok = (A[a] > 0) & (A[b] > 0)
        with np.errstate(divide='ignore', invalid='ignore'):
            c = X[a] * np.conj(X[b]) / A[a] / A[b]
        Cs[p] = np.where(ok, c, 0)
    return V, Cs


def steering(frequenciesInHz, pairTDOAs):
    """E[p, f, d] = e^{-2 pi j f tau[p][d]}."""
    f = np.asarray(frequenciesInHz, np.float64)
    tau = np.asarray(pairTDOAs, np.float64)
    return np.exp(-2j * np.pi * f[None, :, None] * tau[:, None, :])


def angular(Cs, frequenciesInHz, pairTDOAs):
    """-> (ang (D, T), absprod (D, T)): SRP-PHAT and the sum of |cos| |Re C| + |sin| |Im C| over pairs and bins."""
    E = steering(frequenciesInHz, pairTDOAs)
    Cs = np.asarray(Cs, np.complex128)
    cr, ci = Cs.real, Cs.imag
    er, ei = E.real, -E.imag                                  # cos, sin of 2 pi f tau
    ang = np.einsum('pfd,pft->dt', er, cr) + np.einsum('pfd,pft->dt', ei, ci)
    absprod = np.einsum('pfd,pft->dt', np.abs(er), np.abs(cr)) + np.einsum('pfd,pft->dt', np.abs(ei), np.abs(ci))
    return ang, absprod


def peaks(mean_ang, S):
    return C.expected_peaks(mean_ang, S)


def scores(Cs, W, frequenciesInHz, pairTDOAs, indexes):
    """-> (G (S, K, T), absprod (S, K, T)) for the target directions ``indexes``."""
    E = steering(frequenciesInHz, pairTDOAs)
    Cs = np.asarray(Cs, np.complex128)
    W = np.asarray(W, np.float64)
    G, A = [], []
    for d in indexes:
        steered = (Cs * E[:, :, int(d)][:, :, None]).real                 # (P, F, T)
        G.append(np.einsum('fk,pft->kt', W, steered))
        A.append(np.einsum('fk,pft->kt', np.abs(W), np.abs(Cs.real * E[:, :, int(d)].real[:, :, None])
                           + np.abs(Cs.imag * E[:, :, int(d)].imag[:, :, None])))
    return np.stack(G), np.stack(A)


def argmax(G):
    return np.nanargmax(np.asarray(G), axis=0)


def one_hot(am, S):
    a = np.asarray(am)
    return np.stack([(a == i) for i in range(S)]).astype(np.float64)


def numerators(W, H, masks, M, stride=None):
    """W (F, K), H (K, >= M T), masks (S, K, T) -> num (S, M, F, T); channel c's coefficients start at column c * stride (default T)."""
    W = np.asarray(W, np.float64)
    H = np.asarray(H, np.float64)
    Mk = np.asarray(masks, np.float64)
    S, _, T = Mk.shape
    stride = T if stride is None else stride
    num = np.empty((S, M, W.shape[0], T))
    for c in range(M):
        Hc = H[:, c * stride:c * stride + T]
        for i in range(S):
            num[i, c] = W.dot(Hc * Mk[i])
    return num


def denominators(W, H, M, argmax=None, S=None, masks=None, targets=None):
    """den (M, F, T): the ascending-target sum of the one-hot numerators (over ``targets``, default all S), or W.H_c for soft masks."""
    if masks is None:
        num = numerators(W, H, one_hot(argmax, S), M)
        idx = list(range(S)) if targets is None else list(targets)
        den = num[idx[0]].copy()
        for i in idx[1:]:
            den = den + num[i]
        return den
    W = np.asarray(W, np.float64)
    H = np.asarray(H, np.float64)
    T = np.asarray(masks).shape[2]
    return np.stack([W.dot(H[:, c * T:(c + 1) * T]) for c in range(M)])


def _apply(num, den, X):
    X = np.asarray(X, np.complex128)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = num / den[None]
    out = X[None] * q
    dead = den <= 0                                      # False where den is NaN: those propagate
    out[:, dead] = 0
    return out


def ratio_one_hot(W, H, am, S, X, stride=None, targets=None):
    """Arg-max image (K, T) -> target spectrograms (S, M, F, T) complex128."""
    M = np.asarray(X).shape[0]
    num = numerators(W, H, one_hot(am, S), M, stride)
    if stride is None and targets is None:
        den = denominators(W, H, M, argmax=am, S=S)
    else:
        idx = list(range(S)) if targets is None else list(targets)
        den = num[idx[0]].copy()
        for i in idx[1:]:
            den = den + num[i]
    return _apply(num, den, X)


def ratio_soft(W, H, masks, X):
    """Arbitrary masks (S, K, T) -> target spectrograms (S, M, F, T) complex128; den = W.H_c."""
    M = np.asarray(X).shape[0]
    return _apply(numerators(W, H, masks, M), denominators(W, H, M, masks=masks), X)


def ratio_absprod(W, H, M):
    """sum_k |W| |H_c| (M, F, T): what the numerators' and the denominator's rounding errors scale with."""
    W = np.abs(np.asarray(W, np.float64))
    H = np.abs(np.asarray(H, np.float64))
    T = H.shape[1] // M
    return np.stack([W.dot(H[:, c * T:(c + 1) * T]) for c in range(M)])


def istft(spec, window, N, hop, gain):
    """spec (nsig, F, T) complex64, nsig even -> (y (nsig, L) float64, bar (nsig, L)): the centred inverse STFT of the stored spectra
    (fft_checks.istft_frames64 per signal pair, overlap-added in float64, times the gain) and its element-wise bar -- the frame bars of
    fft_checks.frames_bar overlap-added, plus the float32 overlap-add itself: a sample adds at most ceil(N / hop) frames and is scaled
    once, each operation within u of the running sum, which the sum of the frames' moduli bounds."""
    spec = np.asarray(spec)
    nsig, F, T = spec.shape
    trim, L = K.istft_length(N, hop, T, 1)
    n_add = -(-N // hop) + 1
    ys, bars = [], []
    for p in range(nsig // 2):
        frames, sumabs = K.istft_frames64(spec[2 * p], spec[2 * p + 1], window, N)
        fbar = K.frames_bar(sumabs, window, N)
        for c in range(2):
            y, a, b = np.zeros(N + hop * (T - 1)), np.zeros(N + hop * (T - 1)), np.zeros(N + hop * (T - 1))
            for t in range(T):
                y[t * hop:t * hop + N] += frames[c, t]
                a[t * hop:t * hop + N] += np.abs(frames[c, t])
                b[t * hop:t * hop + N] += fbar[t]
            ys.append(y[trim:trim + L] * gain)
            bars.append((b[trim:trim + L] + n_add * K.U32 * (a[trim:trim + L] + b[trim:trim + L])) * abs(gain))
    return np.stack(ys), np.stack(bars)
