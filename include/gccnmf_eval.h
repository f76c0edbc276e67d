/* libgccnmf_eval.so -- C ABI of the scoring kernels for the MI355X (gfx950): the device part of the BSS Eval 3.0 image criteria
 * (`bss_eval_images`: Vincent, Sawada, Bofill, Makino & Rosca 2007) of gcc_nmf_amd/evaluation.py.  DESIGN section 4i.
 *
 * Scoring is not part of the separation ABI (include/gccnmf_hip.h, libgccnmf_hip.so): it is a library of its own with the same
 * conventions -- every pointer is a DEVICE pointer aligned to 16 bytes, every call is asynchronous on `stream` (a hipStream_t passed as
 * void*), every function returns a status code (0 = GCCNMF_OK) decided BEFORE anything is launched, nothing throws across the boundary.
 * gcc_nmf_amd/_eval.py is the ctypes binding.
 *
 * Limits of both kernels: 1 <= L <= 4096 filter taps, Ma, Mb, Q >= 1 signals, n >= 1 samples, 1 <= batch <= 65535 files
 * (GCCNMF_ERR_ARG; GCCNMF_ERR_UNSUPPORTED for a batch above 65535, more than 65535 (signal pair, 1024-lag chunk) or output rows per
 * file, or n within 8192 of 2^31).
 */
#ifndef GCCNMF_EVAL_H
#define GCCNMF_EVAL_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef GCCNMF_OK
#define GCCNMF_OK 0
#define GCCNMF_ERR_ARG 1
#define GCCNMF_ERR_LAUNCH 2
#define GCCNMF_ERR_UNSUPPORTED 3
#endif

#define GCCNMF_EVAL_SYMMETRIC 1      /* flag of gccnmf_eval_lag_correlations: B is A (the same pointer, Mb == Ma) */
#define GCCNMF_EVAL_BLOCK 1024       /* samples of A per partial sum of gccnmf_eval_lag_correlations: a constant, whatever n, L and batch */

int gccnmf_eval_version(void);

/* Bytes of the workspace of gccnmf_eval_lag_correlations: the per-block partial sums, [batch][Ma][Mb][ceil(n / 1024)][2L - 1] float64.
 * -1 for arguments the call would reject. */
long gccnmf_eval_workspace_bytes(int Ma, int Mb, int n, int L, int batch);

/* Lag correlations of every signal of A with every signal of B, per file:
 *     R[a][b][l + L - 1] = sum_n A_a[n] * B_b[n + l],   -(L - 1) <= l <= L - 1,   signals are zero outside [0, n)
 *   A [batch][Ma][n], B [batch][Mb][n] float32;  R [batch][Ma][Mb][2L - 1] float64.
 * The products of two float32 are exact in float64 and every sum is a chain of float64 fma.  A file's samples are cut into blocks of
 * GCCNMF_EVAL_BLOCK; each block's partial sums go to `workspace`, and a second pass adds them in block order: no atomics, and a file's R is
 * bit for bit the same alone and in any batch.
 * flags: GCCNMF_EVAL_SYMMETRIC -- B is A: only the sums of a <= b and, for a == b, of l >= 0 are used; R[b][a][-l] = R[a][b][l] is
 * written from the same value, so R is symmetric to the bit.  (Pairs a > b are not summed at all; for a == b a chunk of 1024 lags that
 * holds l < 0 alone is skipped, while the l < 0 lanes of a chunk that also holds l >= 0 run and are ignored.) */
int gccnmf_eval_lag_correlations(const float* A, const float* B, int Ma, int Mb, int n, int L, int batch, int flags, void* workspace,
                                 double* R, void* stream);

/* Q filtered sums of the signals of A, per file:
 *     P[q][m] = sum_{a in refs(q)} sum_{tau < L} coef[q][a][tau] * A_a[m - tau],   0 <= m < n + L - 1
 *   A [batch][Ma][n] float32;  coef [batch][Q][Ma][L] float64;  P [batch][Q][n + L - 1] float64;
 *   ref_ranges [Q][2] int32 on the device, the same for every file: refs(q) = [first_ref, first_ref + num_refs), clipped to [0, Ma) --
 *   a projection onto one source's signals alone skips the other sources' (their coefficients are not read).
 * One float64 fma chain per output sample in a fixed (a, tau) order: bit for bit the same alone and in any batch. */
int gccnmf_eval_project(const float* A, const double* coef, const int* ref_ranges, int Ma, int Q, int n, int L, int batch, double* P,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
