/* libgccnmf_array.so -- C ABI of the microphone-array stages for the MI355X (gfx950): the two stages of M-channel GCC-NMF that the
 * stereo entry points of include/gccnmf_hip.h cannot serve (gcc_nmf_amd/array.py, GCCNMFArrayEngine).  DESIGN section 4j.
 *
 * M-channel GCC-NMF: the NMF runs on the magnitudes of all channels side by side, the GCC-PHAT functions of all microphone pairs are
 * summed (SRP-PHAT), and an atom is scored by the sum of its pairwise GCC-NMF scores.  With the pairs STACKED along the bin axis the sums
 * run on the stereo entry points (gccnmf_angular_spectrogram, gccnmf_target_scores_masks with F = Fs); what is left is here.
 *
 * A library of its own beside libgccnmf_hip.so, with the same conventions -- every pointer is a DEVICE pointer aligned to 16 bytes,
 * every call is asynchronous on `stream` (a hipStream_t passed as void*), every function returns a status code (0 = GCCNMF_OK) decided
 * BEFORE anything is launched, nothing throws across the boundary.  gcc_nmf_amd/_array.py is the ctypes binding.
 *
 * Notation: M channels, 2 <= M <= 8;  P = M (M - 1) / 2 pairs (a, b), a < b, in lexicographic order (0,1), (0,2), ..., (M-2,M-1);
 * F, T, K, S and the pitches Fp = round_up(F, 16), Kp = round_up(K, 64), Tp = round_up(T, 64) as in gccnmf_hip.h;  N = M T columns of
 * V and H with pitch Np = round_up(M T, 64).  Stacked bins: Fs = (P - 1) Fp + F, whose padded pitch round_up(Fs, 16) is P Fp; pair p
 * owns rows p Fp .. p Fp + F - 1.  At M = 2 (P = 1, Fs = F) every layout is the stereo one.
 */
#ifndef GCCNMF_ARRAY_H
#define GCCNMF_ARRAY_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef GCCNMF_OK
#define GCCNMF_OK 0
#define GCCNMF_ERR_ARG 1
#define GCCNMF_ERR_LAUNCH 2
#define GCCNMF_ERR_UNSUPPORTED 3
#endif

#define GCCNMF_ARRAY_MIN_CHANNELS 2
#define GCCNMF_ARRAY_MAX_CHANNELS 8
#define GCCNMF_ARRAY_MAX_TARGETS 8

int gccnmf_array_version(void);

/* Magnitudes of all channels and PHAT coherence of all pairs of X [batch][M][Fp][Tp] complex (interleaved re, im).
 *   V  [batch][Fp][Np]:          V[f][c T + t] = hypotf(re, im) of channel c (the operation of gccnmf_magnitude); every padding element
 *                                (rows >= F, columns >= M T) is written as 0.
 *   CC [batch][2][P Fp][Tp]      (Re plane, then Im plane): row p Fp + f of pair p = (a, b) is X_a conj(X_b) / |X_a| / |X_b|, exactly
 *                                the arithmetic of gccnmf_coherence (csrc/phat.h) with channel 0 = X_a, channel 1 = X_b, including its rule that a bin
 *                                whose magnitude is zero in either channel gives (0, 0); every other element of both planes is written as 0.
 * Either output may be NULL.  A file's output does not depend on the batch it is in.
 * GCCNMF_ERR_ARG: M outside 2..8, X null, both outputs null, F < 2, T < 1, batch < 1.
 * GCCNMF_ERR_UNSUPPORTED: batch above 65535, P Fp above 65535, M T within 64 of 2^31. */
int gccnmf_array_features(const float* X, int M, int F, int T, int batch, float* V, float* CC, void* stream);

/* Ratio-mask (Wiener-like) reconstruction for M channels: gccnmf_reconstruct(S | GCCNMF_RECONSTRUCT_RATIO) of gccnmf_hip.h with the
 * channel count as an argument.
 *   W [batch][Fp][Kp];  H [batch][Kp][Np], H_c = H[:, c T : (c + 1) T];  X [batch][M][Fp][Tp] complex;
 *   argmax [batch][Kp][Tp] uint8 (one-hot form: M_i = [argmax == i]) or masks [batch][S][Kp][Tp] float (soft form; taken when not NULL);
 *   spec [batch][nsig_pitch][Fp][Tp] complex, target i of channel c in slot i M + c;  nsig_pitch >= S M, slots beyond S M are not touched.
 *     num_i[f,t] = sum_k W[f,k] H_c[k,t] M_i[k,t]     one f32 fma chain in ascending k (v_mfma_f32_32x32x2_f32; the Nyquist row of
 *                                                     F = 32 n + 1 > 32 is the same chain on the VALU)
 *     den[f,t]   = num_0 + num_1 + ... (ascending i)  one-hot form
 *                = sum_k W[f,k] H_c[k,t]              soft form, the same chain
 *     spec[i M + c] = X_c * (num_i / den)             the IEEE quotient, then one real x complex product; 0 for every i where den <= 0
 * Every element of the S M written slots is stored: rows >= F and frames >= T as zeros.  One tile shape whatever F, K, S and the batch:
 * a file's output does not depend on the batch or on its place in it.  At M = 2 the output is gccnmf_reconstruct's, bit for bit: both libraries
 * instantiate the one kernel of csrc/ratio_kernel.h.
 * GCCNMF_ERR_ARG: a null W, H, X or spec, argmax and masks both null, M outside 2..8, F < 2, T < 1, K < 1, batch < 1, nsig_pitch < S M.
 * GCCNMF_ERR_UNSUPPORTED: S outside 1..8, M batch above 65535, M T within 64 of 2^31. */
int gccnmf_array_reconstruct(const float* W, const float* H, const unsigned char* argmax, const float* masks, const float* X, int M, int F,
                             int T, int K, int S, int batch, int nsig_pitch, float* spec, void* stream);

#ifdef __cplusplus
}
#endif
#endif
