// libgccnmf_eval.so -- the two kernels of the BSS Eval image criteria (include/gccnmf_eval.h), gfx950, float64 on the VALU.
//
// Both are the same register tile turned two ways.  A lane owns 16 accumulators 64 apart (lags l, l + 64, ... / output samples m, m + 64, ...)
// and a step takes 8 operands 64 apart on the other axis (samples s0 + 64 i / taps s0 + 64 i): the 128 products of a step read the OTHER
// signal at lane + 64 (j +- i) + const, 23 distinct float64 values that the 64 lanes read from consecutive LDS addresses (ds_read_b64, no
// bank conflict), and 8 values that are the same for every lane (a broadcast read).  31 LDS reads feed 128 fma, which is what keeps the
// LDS (128 bytes per clock and CU) beside the float64 fma rate (64 lanes per clock and CU).  Signals are staged in LDS as float64: a float32
// product is exact in float64, so every sum below is a chain of float64 fma with one rounding per term.
// Built with -ffp-contract=off: every fma is written out, every other operation rounds once.
#include "common.h"
#include "../../include/gccnmf_eval.h"

#define EVAL_JL 16                                   // accumulators per lane
#define EVAL_JN 8                                    // operands of the other axis per step
#define EVAL_SPAN (64 * EVAL_JL)                     // 1024 lags (or output samples) per wave
#define EVAL_STEP (64 * EVAL_JN)                     // 512 samples (or taps) per wave and staging pass
#define EVAL_NV (EVAL_JL + EVAL_JN - 1)              // 23 lane-consecutive values per step

#define EVAL_CORR_WAVES 2
#define EVAL_CORR_THREADS (64 * EVAL_CORR_WAVES)
static_assert(EVAL_CORR_WAVES * EVAL_STEP == GCCNMF_EVAL_BLOCK, "a block is the samples of the workgroup's waves");

#define EVAL_PROJ_WAVES 4
#define EVAL_PROJ_THREADS (64 * EVAL_PROJ_WAVES)
#define EVAL_PROJ_BLOCK (EVAL_PROJ_WAVES * EVAL_SPAN)    // 4096 output samples per workgroup

#define EVAL_MAX_L 4096
#define EVAL_MAX_GRID 65535

// ---- kernel 1: lag correlations --------------------------------------------------------------------------------------------------------
// grid (block of 1024 samples of A, (pair a b) x chunk of 1024 lags, file); 2 waves, each 512 samples of the block against all 1024 lags of
// the chunk; wave 0 adds wave 1's sums to its own and writes the block's partial.  Summation order of one lag inside a wave: s0 = 0 .. 63
// outside, sample s0 + 64 i, i = 0 .. 7 inside.
__global__ __launch_bounds__(EVAL_CORR_THREADS) void eval_lag_partials(const float* __restrict__ A, const float* __restrict__ B,
                                                                        double* __restrict__ part, int Ma, int Mb, int n, int L, int nblk,
                                                                        int nchunk, int symmetric) {
    __shared__ double sA[GCCNMF_EVAL_BLOCK];
    __shared__ double sB[GCCNMF_EVAL_BLOCK + EVAL_SPAN];          // B_b[n0 - (L - 1) + chunk * 1024 + p]: 2047 entries are read
    __shared__ double sR[EVAL_SPAN];
    const int blk = blockIdx.x, file = blockIdx.z;
    const int pair = blockIdx.y / nchunk, chunk = blockIdx.y - pair * nchunk;
    const int a = pair / Mb, b = pair - a * Mb;
    if (symmetric && a > b) return;                                // the whole workgroup: mirrored by eval_lag_reduce
    if (symmetric && a == b && chunk * EVAL_SPAN + (EVAL_SPAN - 1) < L - 1) return;      // a chunk of lags l < 0 only: mirrored too, never read
    const int lags = 2 * L - 1;
    const long n0 = (long)blk * GCCNMF_EVAL_BLOCK;
    const float* Aa = A + ((long)file * Ma + a) * n;
    const float* Bb = B + ((long)file * Mb + b) * n;
    for (int s = threadIdx.x; s < GCCNMF_EVAL_BLOCK; s += EVAL_CORR_THREADS) {
        const long i = n0 + s;
        sA[s] = i < n ? (double)Aa[i] : 0.0;
    }
    const long w0 = n0 - (L - 1) + (long)chunk * EVAL_SPAN;
    for (int p = threadIdx.x; p < GCCNMF_EVAL_BLOCK + EVAL_SPAN; p += EVAL_CORR_THREADS) {
        const long i = w0 + p;
        sB[p] = (i >= 0 && i < n) ? (double)Bb[i] : 0.0;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc[EVAL_JL];
#pragma unroll
    for (int j = 0; j < EVAL_JL; ++j) acc[j] = 0.0;
    // samples of this wave that exist: beyond them A is zero, and a step whose 8 samples are all zero adds nothing
    const long left = (long)n - n0 - (long)wave * EVAL_STEP;
    const int steps = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
    const double* ap = sA + wave * EVAL_STEP;
    const double* bp = sB + wave * EVAL_STEP + lane;
    for (int s0 = 0; s0 < steps; ++s0) {
        double av[EVAL_JN], bv[EVAL_NV];
#pragma unroll
        for (int i = 0; i < EVAL_JN; ++i) av[i] = ap[s0 + 64 * i];
#pragma unroll
        for (int m = 0; m < EVAL_NV; ++m) bv[m] = bp[s0 + 64 * m];
#pragma unroll
        for (int i = 0; i < EVAL_JN; ++i)
#pragma unroll
            for (int j = 0; j < EVAL_JL; ++j) acc[j] = fma(av[i], bv[i + j], acc[j]);
    }
    if (wave == 1) {
#pragma unroll
        for (int j = 0; j < EVAL_JL; ++j) sR[lane + 64 * j] = acc[j];
    }
    __syncthreads();
    if (wave == 0) {
        double* out = part + (((long)file * Ma * Mb + pair) * nblk + blk) * lags;
#pragma unroll
        for (int j = 0; j < EVAL_JL; ++j) {
            const int u = chunk * EVAL_SPAN + lane + 64 * j;
            if (u < lags) out[u] = acc[j] + sR[lane + 64 * j];
        }
    }
}

// grid (256 lags, pair a b, file): the block partials of one lag added in block order; the symmetric call mirrors a < b into b > a and,
// for a == b, the lags l >= 0 into l < 0
__global__ __launch_bounds__(256) void eval_lag_reduce(const double* __restrict__ part, double* __restrict__ R, int Ma, int Mb, int L,
                                                       int nblk, int symmetric) {
    const int lags = 2 * L - 1;
    const int u = blockIdx.x * 256 + threadIdx.x, pair = blockIdx.y, file = blockIdx.z;
    const int a = pair / Mb, b = pair - a * Mb;
    if (u >= lags || (symmetric && a > b)) return;
    const int src = (symmetric && a == b && u < L - 1) ? lags - 1 - u : u;
    const long pairs = (long)Ma * Mb;
    const double* p = part + ((long)file * pairs + pair) * nblk * lags + src;
    double s = 0.0;
    for (int blk = 0; blk < nblk; ++blk) s += p[(long)blk * lags];
    R[((long)file * pairs + pair) * lags + u] = s;
    if (symmetric && a < b) R[((long)file * pairs + (long)b * Mb + a) * lags + (lags - 1 - u)] = s;
}

// ---- kernel 2: projections -------------------------------------------------------------------------------------------------------------
// grid (block of 4096 output samples, output row q, file); 4 waves of 1024 samples each.  Per reference signal a of the row's range and per
// 512 taps: the window of A_a behind the block and the 512 coefficients are staged, then 64 steps of 8 taps s0 + 64 i.  Summation order of
// one output sample: a ascending, taps in chunks of 512 ascending, inside a chunk s0 = 0 .. 63 outside and tap s0 + 64 i, i = 0 .. 7 inside.
__global__ __launch_bounds__(EVAL_PROJ_THREADS) void eval_project(const float* __restrict__ A, const double* __restrict__ coef,
                                                                   const int* __restrict__ ranges, double* __restrict__ P, int Ma, int Q,
                                                                   int n, int L) {
    __shared__ double sX[EVAL_PROJ_BLOCK + EVAL_STEP];            // A_a[m0 - t0 - 511 + p]: 4607 entries are read
    __shared__ double sC[EVAL_STEP];
    const int q = blockIdx.y, file = blockIdx.z;
    const long m0 = (long)blockIdx.x * EVAL_PROJ_BLOCK;
    const long M = (long)n + L - 1;
    int first = ranges[2 * q], num = ranges[2 * q + 1];
    first = first < 0 ? 0 : (first > Ma ? Ma : first);
    num = num < 0 ? 0 : (num > Ma - first ? Ma - first : num);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc[EVAL_JL];
#pragma unroll
    for (int j = 0; j < EVAL_JL; ++j) acc[j] = 0.0;
    const double* xp = sX + wave * EVAL_SPAN + lane + (EVAL_STEP - 1);
    for (int a = first; a < first + num; ++a) {
        const float* Aa = A + ((long)file * Ma + a) * n;
        const double* cq = coef + (((long)file * Q + q) * Ma + a) * L;
        for (int t0 = 0; t0 < L; t0 += EVAL_STEP) {
            __syncthreads();
            const long w0 = m0 - t0 - (EVAL_STEP - 1);
            for (int p = threadIdx.x; p < EVAL_PROJ_BLOCK + EVAL_STEP; p += EVAL_PROJ_THREADS) {
                const long i = w0 + p;
                sX[p] = (i >= 0 && i < n) ? (double)Aa[i] : 0.0;
            }
            for (int t = threadIdx.x; t < EVAL_STEP; t += EVAL_PROJ_THREADS) sC[t] = t0 + t < L ? cq[t0 + t] : 0.0;
            __syncthreads();
            const int steps = L - t0 >= 64 ? 64 : L - t0;        // beyond them every tap of a step is past L: zero coefficients
            for (int s0 = 0; s0 < steps; ++s0) {
                double cv[EVAL_JN], xv[EVAL_NV];
#pragma unroll
                for (int i = 0; i < EVAL_JN; ++i) cv[i] = sC[s0 + 64 * i];
#pragma unroll
                for (int d = 0; d < EVAL_NV; ++d) xv[d] = xp[64 * (d - (EVAL_JN - 1)) - s0];
#pragma unroll
                for (int i = 0; i < EVAL_JN; ++i)
#pragma unroll
                    for (int j = 0; j < EVAL_JL; ++j) acc[j] = fma(cv[i], xv[j - i + (EVAL_JN - 1)], acc[j]);
            }
        }
    }
    double* out = P + ((long)file * Q + q) * M;
#pragma unroll
    for (int j = 0; j < EVAL_JL; ++j) {
        const long m = m0 + wave * EVAL_SPAN + lane + 64 * j;
        if (m < M) out[m] = acc[j];
    }
}

// ---- entry points: every rule is decided before anything is launched --------------------------------------------------------------------
static inline bool eval_aligned(const void* p) { return p != nullptr && ((uintptr_t)p & 15) == 0; }

static int eval_check_common(int n, int L, int batch) {
    if (L < 1 || L > EVAL_MAX_L || n < 1 || batch < 1) return GCCNMF_ERR_ARG;
    if (batch > EVAL_MAX_GRID || n > 0x7fffffff - 2 * EVAL_MAX_L) return GCCNMF_ERR_UNSUPPORTED;
    return GCCNMF_OK;
}

static int eval_check_corr(int Ma, int Mb, int n, int L, int batch) {
    if (Ma < 1 || Mb < 1) return GCCNMF_ERR_ARG;
    const int st = eval_check_common(n, L, batch);
    if (st != GCCNMF_OK) return st;
    if ((long)Ma * Mb * gccnmf_ceil_div(2 * L - 1, EVAL_SPAN) > EVAL_MAX_GRID) return GCCNMF_ERR_UNSUPPORTED;
    return GCCNMF_OK;
}

extern "C" int gccnmf_eval_version(void) { return 100; }

extern "C" long gccnmf_eval_workspace_bytes(int Ma, int Mb, int n, int L, int batch) {
    if (eval_check_corr(Ma, Mb, n, L, batch) != GCCNMF_OK) return -1;
    return (long)batch * Ma * Mb * gccnmf_ceil_div(n, GCCNMF_EVAL_BLOCK) * (2 * L - 1) * (long)sizeof(double);
}

extern "C" int gccnmf_eval_lag_correlations(const float* A, const float* B, int Ma, int Mb, int n, int L, int batch, int flags,
                                            void* workspace, double* R, void* stream) {
    const int st = eval_check_corr(Ma, Mb, n, L, batch);
    if (st != GCCNMF_OK) return st;
    if (flags & ~GCCNMF_EVAL_SYMMETRIC) return GCCNMF_ERR_ARG;
    const int symmetric = flags & GCCNMF_EVAL_SYMMETRIC;
    if (symmetric && (B != A || Mb != Ma)) return GCCNMF_ERR_ARG;
    if (!eval_aligned(A) || !eval_aligned(B) || !eval_aligned(workspace) || !eval_aligned(R)) return GCCNMF_ERR_ARG;
    const int nblk = gccnmf_ceil_div(n, GCCNMF_EVAL_BLOCK), nchunk = gccnmf_ceil_div(2 * L - 1, EVAL_SPAN);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(eval_lag_partials, dim3(nblk, Ma * Mb * nchunk, batch), dim3(EVAL_CORR_THREADS), 0, s, A, B, (double*)workspace, Ma, Mb,
                       n, L, nblk, nchunk, symmetric);
    GCCNMF_CHECK_LAUNCH();
    hipLaunchKernelGGL(eval_lag_reduce, dim3(gccnmf_ceil_div(2 * L - 1, 256), Ma * Mb, batch), dim3(256), 0, s, (const double*)workspace, R, Ma,
                       Mb, L, nblk, symmetric);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

extern "C" int gccnmf_eval_project(const float* A, const double* coef, const int* ref_ranges, int Ma, int Q, int n, int L, int batch,
                                   double* P, void* stream) {
    if (Ma < 1 || Q < 1) return GCCNMF_ERR_ARG;
    const int st = eval_check_common(n, L, batch);
    if (st != GCCNMF_OK) return st;
    if (Q > EVAL_MAX_GRID) return GCCNMF_ERR_UNSUPPORTED;
    if (!eval_aligned(A) || !eval_aligned(coef) || !eval_aligned(ref_ranges) || !eval_aligned(P)) return GCCNMF_ERR_ARG;
    const long M = (long)n + L - 1;
    hipLaunchKernelGGL(eval_project, dim3((unsigned)((M + EVAL_PROJ_BLOCK - 1) / EVAL_PROJ_BLOCK), Q, batch), dim3(EVAL_PROJ_THREADS), 0,
                       (hipStream_t)stream, A, coef, ref_ranges, P, Ma, Q, n, L);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}
