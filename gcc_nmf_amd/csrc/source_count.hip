// numSources='auto': how many talkers a file holds, from the peaks of its mean angular spectrum.
// Reference: gccNMF/gccNMFFunctions.py:105-110 -- KMeans(n_clusters=2) on the peak heights, keep the upper cluster; declared there and
// never run (KMeans is not imported).  In one dimension the 2-means optimum is a threshold on the sorted heights, so the rule here is
// exact: sort the peaks by height, descending (the larger index first among equal heights), and split after the j-th at the smallest j
// that maximises  b_j = c_j^2 / j + (c_P - c_j)^2 / (P - j),  c_j the sequential sum of the j highest -- which minimises the
// within-cluster sum of squares.  Every product, quotient and sum below is a float64 operation rounded on its own, in that order:
// this file is compiled with -ffp-contract=off, and the test restates it in NumPy and compares exactly.
#include "source_count.h"

#define SC_THREADS 256
#define SC_MAX_PEAKS 2048                                  // a power of two >= the 2047 strict local maxima of 4096 values

// the order of the sort: higher first, the larger index first among equal heights; padding (index < 0) last
__device__ __forceinline__ bool sc_before(double ha, int ia, double hb, int ib) {
    if (ia < 0) return false;
    if (ib < 0) return true;
    return ha > hb || (ha == hb && ia > ib);
}

// One 256-thread block per file; 3 <= D <= 4096, 1 <= Smax <= 255.  LDS: the row (32 KB; the prefix sums and the reduction live in it
// once the peaks are out), the peaks' heights (16 KB) and indexes (8 KB).
__global__ __launch_bounds__(SC_THREADS) void count_peaks_kernel(const double* __restrict__ mean_ang, int D, int Dp, int Smax,
                                                                 int* __restrict__ tdoa_idx, int* __restrict__ status) {
#pragma clang fp contract(off)
    __shared__ double v[SOURCE_COUNT_MAX_D];
    __shared__ double h[SC_MAX_PEAKS];
    __shared__ int pi[SC_MAX_PEAKS];
    __shared__ int s_P;
    const int tid = threadIdx.x, b = blockIdx.x;
    const double* m = mean_ang + (long)b * Dp;
    int* out = tdoa_idx + (long)b * Smax;
    for (int i = tid; i < D; i += SC_THREADS) v[i] = m[i];
    if (tid == 0) s_P = 0;
    __syncthreads();
    // strict local maxima, edges never, NaN never greater -- the peaks of pick_peaks_row (gcc.hip); their order in h / pi is whatever
    // the LDS counter hands out, the sort below has one result (no two peaks share an index)
    for (int i = tid; i < D; i += SC_THREADS)
        if (i > 0 && i < D - 1 && v[i] > v[i - 1] && v[i] > v[i + 1]) {
            const int slot = atomicAdd(&s_P, 1);
            h[slot] = v[i];
            pi[slot] = i;
        }
    __syncthreads();
    const int P = s_P;                                          // block-uniform from here on
    if (P == 0) {
        for (int n = tid; n < Smax; n += SC_THREADS) out[n] = -1;
        if (tid == 0) status[b] = 1;
        return;
    }
    int n2 = 1;
    while (n2 < P) n2 <<= 1;
    for (int i = P + tid; i < n2; i += SC_THREADS) {
        h[i] = 0.0;
        pi[i] = -1;
    }
    __syncthreads();
    // bitonic sort of the n2 (height, index) pairs into the order of sc_before
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += SC_THREADS) {
                const int i = 2 * t - (t & (j - 1)), l = i + j;
                const double hi = h[i], hl = h[l];
                const int ii = pi[i], il = pi[l];
                const bool swap = (i & k) == 0 ? sc_before(hl, il, hi, ii) : sc_before(hi, ii, hl, il);
                if (swap) {
                    h[i] = hl; pi[i] = il;
                    h[l] = hi; pi[l] = ii;
                }
            }
            __syncthreads();
        }
    // c_j = h_1 + ... + h_j, added one after the other in that order (one thread: the order IS the rule)
    double* c = v;
    double* red_b = v + SC_MAX_PEAKS;
    int* red_j = (int*)(v + SC_MAX_PEAKS + SC_THREADS);
    if (tid == 0) {
        double acc = 0.0;
        for (int j = 0; j < P; ++j) {
            acc += h[j];
            c[j] = acc;
        }
    }
    __syncthreads();
    const double cP = c[P - 1];
    int count = 1;                                              // one peak is one talker, whatever its height
    if (P > 1) {
        if (!__builtin_isfinite(cP)) {
            for (int n = tid; n < Smax; n += SC_THREADS) out[n] = -1;
            if (tid == 0) status[b] = 1;
            return;
        }
        // the smallest j in [1, P) with the largest b_j (b_j >= 0: a sum of two squares over positive counts)
        double best = -1.0;
        int best_j = 0x7fffffff;
        for (int j = 1 + tid; j < P; j += SC_THREADS) {
            const double cj = c[j - 1], r = cP - cj;
            const double bj = cj * cj / (double)j + r * r / (double)(P - j);
            if (bj > best) {
                best = bj;
                best_j = j;
            }
        }
        red_b[tid] = best;
        red_j[tid] = best_j;
        __syncthreads();
        for (int w = SC_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) {
                const double ob = red_b[tid + w];
                const int oj = red_j[tid + w];
                if (ob > red_b[tid] || (ob == red_b[tid] && oj < red_j[tid])) {
                    red_b[tid] = ob;
                    red_j[tid] = oj;
                }
            }
            __syncthreads();
        }
        count = red_j[0];
    }
    // the cap, and the kept peaks in ascending index order: a kept peak's place is the number of kept peaks to its left
    const int keep = count < Smax ? count : Smax;
    if (tid < keep) {
        const int mine = pi[tid];
        int rank = 0;
        for (int k = 0; k < keep; ++k) rank += pi[k] < mine ? 1 : 0;
        out[rank] = mine;
    }
    for (int n = keep + tid; n < Smax; n += SC_THREADS) out[n] = -1;
    if (tid == 0) status[b] = count > Smax ? 2 : 0;
}

int gccnmf_launch_count_peaks(const double* mean_ang, int D, int Dp, int Smax, int batch, int* tdoa_idx, int* status, hipStream_t s) {
    hipLaunchKernelGGL(count_peaks_kernel, dim3(batch), dim3(SC_THREADS), 0, s, mean_ang, D, Dp, Smax, tdoa_idx, status);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}
