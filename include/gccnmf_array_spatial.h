/* libgccnmf_array_spatial.so -- C ABI of the M x M spatial (multichannel Wiener) filter of the microphone-array path for the MI355X
 * (gfx950): the second stage of mask-based separation under the local Gaussian model, run behind gccnmf_array_reconstruct
 * (include/gccnmf_array.h) on its ratio-mode estimates, in place.  The M-channel form of the spatial mode of gccnmf_reconstruct
 * (include/gccnmf_hip.h); gcc_nmf_amd/csrc/array_spatial.hip, gcc_nmf_amd/array.py (GCCNMFArrayEngine(reconstruction='spatial')).
 * DESIGN section 4j.  The EM refinement (spatialIterations) runs between the two launches: include/gccnmf_array_em.h.
 *
 * A library of its own beside libgccnmf_hip.so and libgccnmf_array.so, with their conventions -- every pointer is a DEVICE pointer
 * aligned to 16 bytes, every call is asynchronous on `stream` (a hipStream_t passed as void*), every function returns a status code
 * (0 = GCCNMF_OK) decided BEFORE the first HIP call, nothing throws across the boundary.  gcc_nmf_amd/_array_spatial.py is the ctypes
 * binding.
 *
 * Notation as in gccnmf_array.h: M channels, 2 <= M <= 8;  P = M (M - 1) / 2 pairs (a, b), a < b, in lexicographic order;  S targets,
 * 1 <= S <= 8;  Fp = round_up(F, 16), Tp = round_up(T, 64).
 *
 * Per file.  E_i,c[f,t] is the ratio-mode estimate of target i, channel c: slot i M + c of spec [batch][nsig_pitch][Fp][Tp] complex
 * (interleaved re, im), as gccnmf_array_reconstruct leaves it;  X [batch][M][Fp][Tp] complex;  E_i = (E_i,0 ... E_i,M-1)^T.
 *
 * POWERS.  v_i[f,t] = (sum_c |E_i,c|^2) / M in float32: s = re_0 re_0 + im_0 im_0, then s = s + (re_c re_c + im_c im_c) for
 * c = 1 ... M - 1 (every product and every sum its own rounding), then the IEEE quotient s / M.  At M = 2: the bits of the stereo
 * 1/2 ((|E_i,0|^2) + (|E_i,1|^2)).
 *
 * COVARIANCES.  R_i[f] = sum_{t < T} E_i E_i^H / n,  n = (sum_c p_c) / M with p_c = sum_t |E_i,c|^2 (so tr R_i = M);  R_i = I when
 * n = 0.  Entry (a, b) is q_ab = sum_t E_i,a conj(E_i,b).  The frame sums are float64; a frame's term is formed in float64 from the
 * float32 estimates -- p_c: re re + im im;  Re q_ab: re_a re_b + im_a im_b;  Im q_ab: im_a re_b - re_a im_b (two exact products, one
 * rounded sum or difference).  The order of the sum is that of the stereo covariance launch and depends on T alone: lane l of 64
 * adds the frames 2l, 2l+1, 2l+128, 2l+129, ... to +0.0 in that order, then the 64 partials are combined by x[l] += x[l ^ m],
 * m = 1, 2, 4, 8, 16, 32.  Then, in float64: n = (p_0 + p_1 + ... + p_{M-1}) / M (ascending c), the quotients p_c / n, Re q_ab / n,
 * Im q_ab / n, and R~_i = R_i + GCCNMF_ARRAY_SPATIAL_LOADING I on the diagonal; ONE rounding to float32.  NaN / Inf take the quotients
 * and propagate.
 *
 * cov [batch][S][Fp][M M] float32 (rows f < F are written): the M diagonal entries R~_00 ... R~_{M-1,M-1}, then for the pairs (a, b),
 * a < b, in lexicographic order (Re R~_ab, Im R~_ab) -- pair p at M + 2 p.  At M = 2 this is the stereo (R~00, R~11, Re R~01, Im R~01).
 *
 * FILTER, per (f, t), float32, every product, sum, difference and the reciprocals their own roundings in the order written (the file is
 * built with -ffp-contract=off):
 *   vs  = v_0 + v_1 + ... (ascending j);  e = the binary exponent of vs (frexp; e = 0 for a zero, infinite or NaN vs: what
 *         v_frexp_exp_i32_f32 returns, and what csrc/spatial.h relies on);  w_j = v_j 2^-e  (exact)
 *   Sigma_w = sum_j w_j R~_j per stored component g (the M M floats of a cov row):  s_g = w_0 r_0g, then s_g = s_g + w_j r_jg, ascending j
 *   y = Sigma_w^-1 X;   S'_i = w_i (R~_i y), written over spec in place
 *   every target is 0 where vs == 0 (a NaN vs is not: it propagates);  rows >= F and frames >= T of the S M written slots are zeros;
 *   slots >= S M are not touched.
 * M = 2: the closed 2 x 2 inverse of the stereo filter, the same code (spatial_frame of csrc/spatial.h): cov and spec are then bit for
 * bit what gccnmf_reconstruct leaves in spatial mode on the same inputs.
 * M >= 3: a square-root-free LDL^H factorisation Sigma_w = L D L^H (L unit lower triangular, D real diagonal) WITHOUT pivoting.
 * Sigma_w is positive definite with margin -- every R~_j >= LOADING I and sum_j w_j lies in [1/2, 1), so its smallest eigenvalue is at
 * least 5e-4, against a float32 perturbation of the order of M u ||Sigma_w|| ~ 4e-6 (||Sigma_w|| <= M (1 + LOADING), u = 2^-24) --
 * so every pivot d_k stays positive and pivoting is not needed.  With Sigma_ik = conj(Sigma_ki) for i > k (the negation is exact),
 * a (x) b for the complex product (re: a.re b.re - a.im b.im;  im: a.re b.im + a.im b.re) and a (x) conj(b) (re: a.re b.re + a.im b.im;
 * im: a.im b.re - a.re b.im) -- each the two rounded products and their rounded sum or difference:
 *   for k = 0 ... M - 1:
 *     g_m = (l_km.re d_m, l_km.im d_m)                                             for m < k
 *     d_k = Sigma_kk,  then d_k = d_k - (l_km.re g_m.re + l_km.im g_m.im)          m = 0 ... k - 1 ascending
 *     rd_k = 1 / d_k                                                              the one reciprocal of the column
 *     for i = k + 1 ... M - 1:  c = Sigma_ik,  then c = c - l_im (x) conj(g_m)    m ascending, re and im each their own difference
 *                               l_ik = (c.re rd_k, c.im rd_k)
 *   forward:   z_i = X_i, then z_i = z_i - l_ik (x) z_k                            i = 0 ... M - 1, k = 0 ... i - 1 ascending
 *   scaling:   z_k = (z_k.re rd_k, z_k.im rd_k)
 *   backward:  y_k = z_k, then y_k = y_k - conj(l_ik) (x) y_i                      k = M - 1 ... 0, i = k + 1 ... M - 1 ascending
 *                                                                                 (conj(a) (x) b: re a.re b.re + a.im b.im; im a.re b.im - a.im b.re)
 *   output:    u_a = R~_a0 (x) y_0, then u_a = u_a + R~_ab (x) y_b, b ascending;  R~_aa real (two products), R~_ab the stored pair for
 *              a < b, conj(stored pair (b, a)) (x) y_b for a > b;  S'_i,a = (w_i u_a.re, w_i u_a.im)
 * A file's output does not depend on the batch or on its place in it; there are no atomics.
 *
 * Two launches.  Covariance: one wave per (file, target, bin) -- two at M >= 6, which deal the pairs between them; a sum is always one
 * wave's -- 16 bytes (two frames) per lane, channel and step, the float64 partial sums in registers.  Filter: one wave per (file, bin)
 * row; a lane owns two consecutive frames per step (M <= 4) or one (M >= 5); all loads of a lane's frames come in front of its first
 * store; the row's S M M covariance floats sit in LDS.
 */
#ifndef GCCNMF_ARRAY_SPATIAL_H
#define GCCNMF_ARRAY_SPATIAL_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef GCCNMF_OK
#define GCCNMF_OK 0
#define GCCNMF_ERR_ARG 1
#define GCCNMF_ERR_LAUNCH 2
#define GCCNMF_ERR_UNSUPPORTED 3
#endif

#define GCCNMF_ARRAY_SPATIAL_MIN_CHANNELS 2
#define GCCNMF_ARRAY_SPATIAL_MAX_CHANNELS 8
#define GCCNMF_ARRAY_SPATIAL_MAX_TARGETS 8
#define GCCNMF_ARRAY_SPATIAL_LOADING 1e-3       /* = GCCNMF_SPATIAL_LOADING of gccnmf_hip.h */

int gccnmf_array_spatial_version(void);

/* Floats of `cov`: batch S Fp M M.  -1 for a shape gccnmf_array_spatial rejects (M outside 2..8, S outside 1..8, F < 2, batch < 1,
 * M batch above 65535). */
long gccnmf_array_spatial_workspace_floats(int M, int F, int S, int batch);

/* The covariance launch and the filter launch on `stream`: cov is written (rows f < F), spec is read and overwritten in place.
 * GCCNMF_ERR_ARG: a null X or spec, a null or misaligned (16 bytes) cov, M outside 2..8, F < 2, T < 1, batch < 1, nsig_pitch < S M.
 * GCCNMF_ERR_UNSUPPORTED: S outside 1..8, M batch above 65535, M T within 64 of 2^31. */
int gccnmf_array_spatial(const float* X, int M, int F, int T, int S, int batch, int nsig_pitch, float* cov, float* spec, void* stream);

#ifdef __cplusplus
}
#endif
#endif
