"""float64 NumPy restatement of the ratio-mask (Wiener-like) reconstruction (include/gccnmf_hip.h, gccnmf_reconstruct with
GCCNMF_RECONSTRUCT_RATIO; csrc/ratio.hip).  Per channel c, target i, bin f, frame t, with H_c = H[:, c*T:(c+1)*T]:

    num_i[f,t] = sum_k W[f,k] H_c[k,t] M_i[k,t]
    den[f,t]   = sum_i num_i[f,t]  (ascending i)   one-hot form: M_i = [argmax == i]
               = sum_k W[f,k] H_c[k,t]             soft form: arbitrary masks
    S[i,c]     = X_c * (num_i / den)  if den > 0, else 0 for every i           (NaN / Inf propagate: `den <= 0` is false for NaN)

Nothing here knows about the device: it is the contract the kernel is tested against."""
import numpy as np


def numerators(W, H, masks):
    """W (F, K), H (K, 2T), masks (S, K, T) -> num (S, 2, F, T) float64."""
    W = np.asarray(W, np.float64)
    H = np.asarray(H, np.float64)
    M = np.asarray(masks, np.float64)
    S, K, T = M.shape
    num = np.empty((S, 2, W.shape[0], T))
    for c in range(2):
        Hc = H[:, c * T:(c + 1) * T]
        for i in range(S):
            num[i, c] = W.dot(Hc * M[i])
    return num


def one_hot(argmax, S):
    a = np.asarray(argmax)
    return np.stack([(a == i) for i in range(S)]).astype(np.float64)


def _apply(num, den, X):
    X = np.asarray(X, np.complex128)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = num / den[None]
    out = X[None] * q
    dead = den <= 0                                      # False where den is NaN: those propagate
    out[:, dead] = 0
    return out


def denominators(W, H, argmax=None, S=None, masks=None):
    """den (2, F, T): the sum of the one-hot numerators in ascending target order, or W.H_c for soft masks."""
    if masks is None:
        num = numerators(W, H, one_hot(argmax, S))
        den = num[0].copy()
        for i in range(1, num.shape[0]):
            den = den + num[i]
        return den
    W = np.asarray(W, np.float64)
    H = np.asarray(H, np.float64)
    T = np.asarray(masks).shape[2]
    return np.stack([W.dot(H[:, c * T:(c + 1) * T]) for c in range(2)])


def ratio_one_hot(W, H, argmax, S, X):
    """Arg-max image (K, T) -> target spectrograms (S, 2, F, T) complex128."""
    num = numerators(W, H, one_hot(argmax, S))
    return _apply(num, denominators(W, H, argmax=argmax, S=S), X)


def ratio_soft(W, H, masks, X):
    """Arbitrary masks (S, K, T) -> target spectrograms (S, 2, F, T) complex128; den = W.H_c."""
    return _apply(numerators(W, H, masks), denominators(W, H, masks=masks), X)
