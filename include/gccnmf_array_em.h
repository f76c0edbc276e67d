/* libgccnmf_array_em.so -- C ABI of the EM refinement of the M x M spatial (multichannel Wiener) filter of the microphone-array path for the
 * MI355X (gfx950): n iterations of the local Gaussian model EM (Duong, Vincent & Gribonval 2010) between the covariance launch and the
 * filter launch of gccnmf_array_spatial (include/gccnmf_array_spatial.h, whose notation, buffers, POWERS, COVARIANCES and FILTER this header
 * takes as they are).  The M-channel form of GCCNMF_RECONSTRUCT_SPATIAL_ITERATIONS(n) of gccnmf_reconstruct (include/gccnmf_hip.h);
 * gcc_nmf_amd/csrc/array_spatial_em.hip, gcc_nmf_amd/array.py (GCCNMFArrayEngine(reconstruction='spatial', spatialIterations=n)).
 * DESIGN section 4j.  tests/array_em_restatement.py restates it in NumPy.
 *
 * A library of its own with the conventions of the other four: every pointer is a DEVICE pointer aligned to 16 bytes, every call is
 * asynchronous on `stream` (a hipStream_t passed as void*), every function returns a status code decided BEFORE the first HIP call,
 * nothing throws across the boundary.  gcc_nmf_amd/_array_em.py is the ctypes binding.
 *
 * workspace: cov [batch][S][Fp][M M] float32, then the powers [batch][S][Fp][Tp] float32 (rows f < F, frames t < T are written; at M = 2
 * with an odd T frame T is written too, as a zero: the stereo kernel stores the powers in pairs of frames).
 *
 * Per file and bin f, with lambda = GCCNMF_ARRAY_SPATIAL_LOADING:
 *   start      v_i[t], R~_i: the POWERS and COVARIANCES of gccnmf_array_spatial.h, the covariance launch itself
 *   iteration  against the OLD R~, per frame:  Sigma = sum_j v_j R~_j,  G_i = v_i R~_i Sigma^-1,  s_i = G_i X,
 *              C_i = s_i s_i^H + (I - G_i) v_i R~_i,  v'_i = max(0, (1/M) Re tr(R~_i^-1 C_i)),  v'_i = 0 for every i where sum_j v_j = 0;
 *              then A_i = the sum of C_i / v'_i over the frames with v'_i != 0 (float32 terms, float64 sum),  n_i = their number,
 *              R'_i = A_i / n_i (I when n_i = 0),  R~'_i = R'_i + lambda (tr R'_i / M) I, rounded to float32 ONCE, in the layout of a cov row;
 *              v <- v', R~ <- R~'.  A frame whose v'_i is NaN is counted (its term is NaN too): it stays in its bin and in its file.
 *   output     the FILTER of gccnmf_array_spatial.h on the final v (from the workspace) and R~
 *
 * What is evaluated is the cancellation-free form.  With w_j = v_j 2^-e (e as in the FILTER), Sigma_w = L D L^H, Z = Sigma_w^-1, y = Z X,
 * u_i = R~_i y and N_i = sum_{j != i} w_j R~_j:
 *   M - tr G_i = Re tr(Z N_i) =: k_i;   (I - G_i) v_i R~_i = v_i N_i Z R~_i =: v_i P_i  (P_i Hermitian, = R~_i (Z N_i));
 *   s_i^H R~_i^-1 s_i = w_i^2 Re(y^H u_i)  (no inverse of R~_i);   v'_i = w_i v"_i,  v"_i = (1/M)(w_i Re(y^H u_i) + 2^e k_i);
 *   C_i / v'_i = C"_i / v"_i,  C"_i = w_i u_i u_i^H + 2^e P_i.     With S = 1, N_i, k_i and P_i are exact zeros.
 *
 * M = 2: spatial_em_frame of csrc/spatial.h, the stereo code: cov, the powers and spec are then bit for bit what gccnmf_reconstruct leaves
 * in spatial mode with the same n.
 *
 * M >= 3, one frame and one target i, float32, every product, sum, difference, quotient and reciprocal its own rounding in the order
 * written (the file is built with -ffp-contract=off);  (x) and the component index g of a cov row as in gccnmf_array_spatial.h:
 *   vs, e, w_j, Sigma_w  as in the FILTER.  N_g = w_j r_jg for the first j != i, then N_g = N_g + w_j r_jg, ascending j (the product
 *                        w_j r_jg is the one that enters Sigma_w);  N_g = 0 at S = 1
 *   L, D, rd, y          the factorisation, the forward substitution, the scaling and the back substitution of the FILTER
 *   u_a                  the output row of the FILTER on R~_i and y (without the product by w_i), a = 0 ... M - 1
 *   h                    = y_0.re u_0.re + y_0.im u_0.im, then h = h + (y_a.re u_a.re + y_a.im u_a.im), a ascending
 *   for b = 0 ... M - 1: W_.b = the three substitutions on column b of N_i  (entry c: (N_b, 0) for c = b, the stored pair (c, b) for
 *                        c < b, the conjugate of the stored pair (b, c) for c > b; the negation is exact)
 *                        k = Re W_00, then k = k + Re W_bb
 *                        P_ab = the output row a of the FILTER on R~_i and W_.b, for a <= b;  of P_bb the real part is kept
 *   v"  = (w_i h + ldexp(k, e)) / M        (the IEEE quotient by the float M)
 *   v'  = w_i v";  0 where v' < 0 (a NaN stays);  0 where vs == 0
 *   rv  = 1 / v"
 *   term_aa    = (w_i (u_a.re u_a.re + u_a.im u_a.im) + ldexp(P_aa, e)) rv
 *   Re term_ab = (w_i (u_a.re u_b.re + u_a.im u_b.im) + ldexp(Re P_ab, e)) rv,   Im term_ab = (w_i (u_a.im u_b.re - u_a.re u_b.im) + ldexp(Im P_ab, e)) rv
 * The frame sums: each term converted to float64 and added where v' != 0, in the order of the covariance launch -- lane l of 64 adds the
 * frames 2l, 2l+1, 2l+128, 2l+129, ... to +0.0, then x[l] += x[l ^ m], m = 1, 2, 4, 8, 16, 32: the order depends on T alone, at every M.
 * Then in float64: the quotients A_g / n_i (1 on the diagonal and 0 elsewhere when n_i = 0), tr = R'_00 + R'_11 + ... (ascending),
 * load = lambda (tr / M), R'_aa + load on the diagonal; ONE rounding to float32.
 *
 * Three launches: the covariance kernel of libgccnmf_array_spatial.so's source, the EM kernel (all n iterations; one workgroup per
 * (file, bin) row for the whole launch, at M >= 3 one wave per target), that library's filter kernel taking its powers from the workspace.
 * No atomics, no counters, no cross-workgroup dependency: a file's bits are the same alone and in any batch.
 */
#ifndef GCCNMF_ARRAY_EM_H
#define GCCNMF_ARRAY_EM_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef GCCNMF_OK
#define GCCNMF_OK 0
#define GCCNMF_ERR_ARG 1
#define GCCNMF_ERR_LAUNCH 2
#define GCCNMF_ERR_UNSUPPORTED 3
#endif

#define GCCNMF_ARRAY_EM_MAX_ITERATIONS 255

int gccnmf_array_em_version(void);

/* Floats of `workspace`: batch S Fp M M (cov) + batch S Fp Tp (the powers).  -1 for a shape gccnmf_array_em rejects (those of
 * gccnmf_array_spatial_workspace_floats, T < 1, M T within 64 of 2^31). */
long gccnmf_array_em_workspace_floats(int M, int F, int T, int S, int batch);

/* The covariance launch, n EM iterations in one launch and the filter launch on `stream`: cov and the powers are written, spec is read and
 * overwritten in place.  The rules of gccnmf_array_spatial with `workspace` in the place of cov -- GCCNMF_ERR_ARG: a null X or spec, a
 * null or misaligned (16 bytes) workspace, M outside 2..8, F < 2, T < 1, batch < 1, nsig_pitch < S M.  GCCNMF_ERR_UNSUPPORTED: S outside
 * 1..8, M batch above 65535, M T within 64 of 2^31 -- and n outside 1..255: GCCNMF_ERR_UNSUPPORTED (n = 0 is gccnmf_array_spatial). */
int gccnmf_array_em(const float* X, int M, int F, int T, int S, int batch, int nsig_pitch, int n, float* workspace, float* spec, void* stream);

#ifdef __cplusplus
}
#endif
#endif
