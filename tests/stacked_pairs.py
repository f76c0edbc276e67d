"""The stereo localisation and scores calls at the shapes the microphone-array engine hands them (gcc_nmf_amd/array.py: the P pairs STACKED
along the bin axis, pair p in rows p Fp .. p Fp + F - 1 of Fs = (P - 1) Fp + F bins), in plain NumPy: the cells, the launch rule that says
which kernel a cell reaches, the host-built inputs, and the checks of one file's outputs against tests/array_restatement.py.  The device test
(tests/test_gpu_stacked_pairs.py) runs the checks on what the library wrote, the host test (tests/test_array_host.py) on a float64
evaluation of the stacked buffers with mistakes planted in it, so that both go through the same functions and the same bounds:

    angular spectrogram    gcc_checks.check_gemm_like at Kd = 2 P F against array_restatement.angular
    its mean, the peaks    gcc_checks.check_mean, check_peaks: exact on the device's own spectrogram
    steering products      the workspace of the scores call, row by row against Re(C_p e_p) at Kd = 1; exact zeros in the padding rows of
                           every pair block and in the padding frames
    scores                 check_gemm_like at Kd = P F against array_restatement.scores;  arg-max: check_argmax on the device's own scores

The Nyquist row of every pair's coherence and the last atom of W are 100 times larger than the rest, and every pair has its own TDOA row
(an eight-microphone line whose 28 spacings are all different), so that a dropped, shifted or exchanged pair block is far outside the
bounds.
"""
import numpy as np

import array_restatement as A
import gcc_checks as C

SOUND = 340.29
# a Golomb ruler (no two differences equal) in units of 3 cm: no two pair vectors of the line are equal, whichever M <= 8 of them are used
LINE8 = np.stack([0.03 * np.array([0.0, 1, 4, 9, 15, 22, 32, 34]), np.zeros(8), np.zeros(8)], axis=1)
RING_LIMIT = 4096                                        # gemm_ring.h, gccnmf_ring_supports: 1 <= Kd <= 4096


def rup(a, b):
    return -(-a // b) * b


def shapes(M, F):
    """-> (P, Fp, Fs)"""
    P, Fp = M * (M - 1) // 2, rup(F, 16)
    return P, Fp, (P - 1) * Fp + F


def kernels(M, F, D, S, K, T, batch, key2, key3):
    """'angular | scores': the kernel each GEMM of a cell reaches, restated from the launch rules of csrc/gcc.hip (gcc_small_launch with
    tuning key 2 = 0 by size, 1 throughput tile, 2 ring; the D > 128 and K > 128 switches; tuning key 3 = LDS-DMA for the tall scores) and
    the ring kernel's limit.  The scores' last bin is a rank-1 epilogue term (k-tail) when Fs % 16 == 1, which shortens the reduction by one."""
    P, Fp, Fs = shapes(M, F)

    def small(rows, cols, Kd):
        if not 1 <= Kd <= RING_LIMIT or key2 == 1:
            return False
        return key2 == 2 or batch * -(-rows // 512) * -(-cols // 64) < 256

    ang = 'ring' if small(D, T, 2 * P * Fp) else 'gemm<4,1>' if D > 128 else 'gemm<1,4>'
    ktail = Fs % 16 == 1
    if small(K, S * rup(T, 64), Fs - 1 if ktail else Fs):
        sc = 'ring'
    else:
        sc = 'dma' if K > 128 and key3 else 'gemm<4,1>' if K > 128 else 'gemm<1,4>'
    return '%s | %s%s' % (ang, sc, ' k-tail' if ktail else '')


# (M, F, D, S, K, T, batch, key 2, key 3) -> 'angular | scores' kernels.  Fs and the two reduction lengths are in the comments.
CELLS = {
    (8, 33, 33, 3, 70, 5, 1, 2, 1): 'ring | ring k-tail',                  # Fs 1329: angular reduction 2688, scores 1328
    (8, 129, 64, 2, 16, 3, 1, 2, 1): 'gemm<1,4> | ring k-tail',            # Fs 4017: scores 4016, the longest the ring takes here; angular 8064 is refused
    (7, 257, 33, 3, 200, 5, 1, 2, 1): 'gemm<1,4> | dma k-tail',            # Fs 5697: scores 5696, beyond the ring
    (7, 257, 33, 3, 200, 5, 1, 2, 0): 'gemm<1,4> | gemm<4,1> k-tail',
    (7, 257, 33, 3, 64, 5, 1, 2, 1): 'gemm<1,4> | gemm<1,4> k-tail',
    (6, 41, 200, 4, 129, 65, 1, 1, 1): 'gemm<4,1> | dma',                  # Fs 713: F % 16 != 1, no k-tail
    (6, 41, 200, 4, 129, 65, 1, 1, 0): 'gemm<4,1> | gemm<4,1>',
    (5, 513, 181, 3, 130, 5, 1, 1, 1): 'gemm<4,1> | dma k-tail',           # Fs 5265
    (8, 513, 200, 3, 129, 3, 1, 0, 1): 'gemm<4,1> | dma k-tail',           # Fs 14769: the default window at the widest array
    (8, 2049, 64, 2, 64, 2, 1, 0, 1): 'gemm<1,4> | gemm<1,4> k-tail',      # Fs 57777: grid extent 57792, reductions 57776 and 115584
    (3, 129, 64, 2, 129, 5, 9, 1, 0): 'gemm<1,4> | gemm<4,1> k-tail',      # Fs 417, a batch: a file alone gives the bits it gives in the batch
    (3, 129, 64, 2, 129, 5, 3, 2, 1): 'ring | ring k-tail',
    # no stacking (M = 2): the ring limit itself
    (2, 4097, 33, 2, 16, 3, 1, 2, 1): 'gemm<1,4> | ring k-tail',           # scores reduction 4096: the last the ring takes
    (2, 4113, 33, 2, 16, 3, 1, 2, 1): 'gemm<1,4> | gemm<1,4> k-tail',      # 4112: the first it refuses
}


def pair_tdoas(M, D):
    return A.pair_tdoas_from_geometry(LINE8[:M], A.azimuth_directions(D), SOUND)


def frequencies(F):
    return np.linspace(0, 8000.0, F)


def host_file(M, F, D, S, K, T, seed):
    """One file's float32 inputs: C (P, F, T) random unit-modulus coherence with every pair's Nyquist row x 100; W (F, K) in [0.01, 1] with
    the last atom x 100; S distinct TDOA indexes, ascending."""
    P = M * (M - 1) // 2
    rng = np.random.RandomState(seed)
    Cs = np.exp(1j * rng.uniform(-np.pi, np.pi, (P, F, T))).astype(np.complex64)
    Cs[:, F - 1] *= np.float32(100)
    W = rng.uniform(0.01, 1.0, (F, K)).astype(np.float32)
    W[:, K - 1] *= np.float32(100)
    tdoa = np.sort(rng.choice(D, S, replace=False)).astype(np.int32)
    return dict(C=Cs, W=W, tdoa=tdoa)


def stacked_operands(f, Fp, Kp, Tp):
    """-> CC [2][P Fp][Tp] (pair p in rows p Fp .. p Fp + F - 1, zero elsewhere), Ws [P Fp][Kp] (W under every pair's rows, as
    GCCNMFArrayEngine.masks copies it)."""
    P, F, T = f['C'].shape
    K = f['W'].shape[1]
    CC = np.zeros((2, P * Fp, Tp), np.float32)
    Ws = np.zeros((P * Fp, Kp), np.float32)
    for p in range(P):
        CC[0, p * Fp:p * Fp + F, :T], CC[1, p * Fp:p * Fp + F, :T] = f['C'][p].real, f['C'][p].imag
        Ws[p * Fp:p * Fp + F, :K] = f['W']
    return CC, Ws


def evaluate(CC, trig, Ws, tdoa, D, S, K, T):
    """What the two library calls hold for one file, evaluated in float64 on the stacked float32 buffers themselves and rounded to float32
    (the mean, the peaks and the arg-max from the rounded values, as the device takes them from its own): the host-side copy that
    tests/test_array_host.py plants its mistakes in.  -> the dict checks() reads."""
    cr, ci = CC[0].astype(np.float64), CC[1].astype(np.float64)
    cos, sin = trig[0].astype(np.float64), trig[1].astype(np.float64)
    ang = (cos.T.dot(cr) + sin.T.dot(ci)).astype(np.float32)
    mean = ang[:D, :T].astype(np.float64).mean(axis=1)
    idx, status = C.expected_peaks(mean, S)
    R, Tp = cr.shape
    Pw = np.zeros((R, S, Tp))
    for i, d in enumerate(tdoa):
        Pw[:, i, :T] = cr[:, :T] * cos[:, d][:, None] + ci[:, :T] * sin[:, d][:, None]
    Pw = Pw.astype(np.float32)
    scores = np.einsum('rk,rit->kit', Ws.astype(np.float64), Pw.astype(np.float64)).astype(np.float32)
    am = np.zeros((Ws.shape[1], Tp), np.uint8)
    am[:K, :T] = np.nanargmax(scores[:K, :, :T], axis=1)
    return dict(ang=ang, mean=mean, idx=np.array(idx), status=status, P=Pw, scores=scores, argmax=am)


def checks(out, f, M, F, D, S, K, T, what=''):
    """The named checks of one file: out = dict(ang (Dp, Tp), mean (>= D,), idx (S,), status, P (P Fp, S, Tp) the scores workspace,
    scores (Kp, S, Tp), argmax (Kp, Tp)) against the file's own host inputs f.  -> [(name, callable)]; a callable raises AssertionError."""
    Pn, Fp, Fs = shapes(M, F)
    freqs, tau = frequencies(F), pair_tdoas(M, D)
    Cs = f['C'].astype(np.complex128)
    label = lambda name: '%s%s' % (what, name)

    def angular():
        ref, absprod = A.angular(Cs, freqs, tau)
        C.report_gemm_like(out['ang'][:D, :T], ref, absprod, 2 * Pn * F, what=label('angular spectrogram'))

    def mean():
        C.check_mean(out['mean'][:D], out['ang'][:D, :T], what=label('mean'))

    def peaks():
        if D >= 3:
            C.check_peaks(out['idx'], out['status'], out['mean'][:D], S, what=label('peaks'))

    def steering():
        E = A.steering(freqs, tau)[:, :, f['tdoa']]                                       # (P, F, S)
        ref = (Cs[:, :, None, :] * E[:, :, :, None]).real                                 # (P, F, S, T)
        absprod = (np.abs(Cs.real)[:, :, None, :] * np.abs(E.real)[:, :, :, None]
                   + np.abs(Cs.imag)[:, :, None, :] * np.abs(E.imag)[:, :, :, None])
        got = out['P'].reshape(Pn, Fp, S, -1)[:, :F, :, :T]
        worst = 0.0
        for p in range(Pn):                                                               # row by row: the first miss names its pair
            worst = max(worst, C.gemm_share(got[p], ref[p], absprod[p], 1))
        print('%s: worst share of the bar (10 * 2^-24 absprod) %.4f' % (label('steering products'), worst))
        for p in range(Pn):
            C.check_gemm_like(got[p], ref[p], absprod[p], 1, what=label('steering products of pair %d' % p))

    def steering_padding_rows():
        C.check_zero(out['P'].reshape(Pn, Fp, S, -1)[:, F:], what=label('steering products, padding rows of every pair block'))

    def steering_padding_frames():
        C.check_zero(out['P'][:, :, T:], what=label('steering products, padding frames'))

    def scores():
        ref, absprod = A.scores(Cs, f['W'], freqs, tau, f['tdoa'])
        C.report_gemm_like(np.transpose(out['scores'][:K, :, :T], (1, 0, 2)), ref, absprod, Pn * F, what=label('scores'))

    def scores_padding_frames():
        C.check_zero(out['scores'][:K, :, T:], what=label('scores, padding frames'))

    def argmax():
        C.check_argmax(out['argmax'][:K, :T], np.transpose(out['scores'][:K, :, :T], (1, 0, 2)), what=label('arg-max'))
        C.check_zero(out['argmax'][K:], what=label('arg-max, padding atoms'))
        C.check_zero(out['argmax'][:, T:], what=label('arg-max, padding frames'))

    return [('angular', angular), ('mean', mean), ('peaks', peaks), ('steering', steering), ('steering padding rows', steering_padding_rows),
            ('steering padding frames', steering_padding_frames), ('scores', scores), ('scores padding frames', scores_padding_frames),
            ('arg-max', argmax)]


# ---- the engine at 5 to 8 microphones (tests/test_gpu_array_engine.py) ----------------------------------------------------------------------
# (M, batch, S) -> seed of synthetic.array_mixture; file b of a case is seed + b.  The mixtures are chosen on the host (tests/test_array_host.py):
# the float64 restatement alone finds S peaks in every file, each clear of its neighbours by far more than the float32 spectrogram's error.
ENGINE_CASES = {(5, 1, 2): 0, (7, 1, 3): 3, (6, 3, 2): 0, (8, 2, 3): 2}
ENGINE_SHAPE = dict(n=4096, n_fft=256, hop=64, D=61)
# the corner of the envelope: eight microphones, the longest window, three frames
CORNER_CASE, CORNER_SEED = (8, 1, 2), 0
CORNER_SHAPE = dict(n=4096 + 2 * 1024, n_fft=4096, hop=1024, D=61)
AZIMUTHS = [40, 90, 130]


def engine_mixtures(M, B, S, seed, n):
    from gcc_nmf_amd.synthetic import array_mixture
    return np.stack([array_mixture(seed + b, LINE8[:M], AZIMUTHS[:max(S, 2)], n, 16000) for b in range(B)])


def reference_peaks(x, n_fft, hop, D, S):
    """One file x (M, n) through the float64 restatement alone -> (indexes, status, the smallest height of a chosen peak above its higher
    neighbour as a share of the mean spectrum's range)."""
    import fft_checks as K
    M, n = x.shape
    T = 1 + (n - n_fft) // hop
    w = np.hanning(n_fft).astype(np.float32)
    pad = np.concatenate([x, np.zeros((M % 2, n), np.float32)])
    X = np.concatenate([K.stft64(pad[c:c + 2], w, n_fft, hop, T)[0] for c in range(0, M, 2)])[:M]
    _, Cs = A.features(X.astype(np.complex64))
    ang, _ = A.angular(Cs, np.linspace(0, 8000.0, n_fft // 2 + 1), pair_tdoas(M, D))
    mean = ang.mean(axis=1)
    idx, status = A.peaks(mean, S)
    clear = min([mean[i] - max(mean[i - 1], mean[i + 1]) for i in idx if i >= 0] or [0.0]) / (mean.max() - mean.min())
    return idx, status, clear
