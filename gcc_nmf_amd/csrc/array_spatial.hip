// libgccnmf_array_spatial.so: the M x M spatial (multichannel Wiener) filter of the microphone-array path, behind the ratio-mask
// reconstruction of array.hip on its estimates, in place (include/gccnmf_array_spatial.h states the contract operation by operation;
// DESIGN section 4j).  A library of its own: it takes nothing from the separation library but the status codes of common.h and the
// 2 x 2 arithmetic of spatial.h (M = 2 runs spatial_frame, so that two channels give the stereo filter's bits), and no GEMM header.
//
// Two launches, the shapes of spatial.hip.  array_spatial_cov_kernel<M>: one wave per (file, target, bin) reads the M channel rows once,
// 16 bytes (two frames) per lane, channel and step; lane l adds frames 2l, 2l+1, 2l+128, ... in that order in float64 into M M partial
// sums held in registers, and the 64 partials are combined by a fixed xor butterfly: the order depends on T alone, no atomics.  At
// M >= 6 two waves share a (file, target, bin): each forms the diagonal sums and every other pair's.
// array_spatial_filter_kernel<M, S>: one wave per (file, bin) row; a lane owns two consecutive frames per step (M <= 4) or one (M >= 5),
// loads its S M estimates and X (all loads in front of the first store), keeps only the S powers, solves Sigma_w y = X by an LDL^H
// factorisation in registers and writes the S M filtered values over the estimates.  The row's S M M covariance floats are
// wave-uniform: each wave copies them to its own quarter of the workgroup's LDS once and reads them from there (one address for all lanes).
//
// Built with -ffp-contract=off; every product and sum below is its own float32 rounding, in the order written.
#include "common.h"
#include "spatial.h"
#include "../../include/gccnmf_array_spatial.h"

#define ARRAY_SPATIAL_VERSION 100

// pair (a, b), a < b, of M channels in lexicographic order -> its index
__host__ __device__ constexpr int array_spatial_pair(int M, int a, int b) { return a * M - a * (a + 1) / 2 + (b - a - 1); }

// The M M sums of a (file, target, bin) are shared among PARTS waves: every part keeps the M diagonal sums (each needs the trace), the
// pair sums are dealt out pair by pair (pair q to part q % PARTS).  A sum is formed by one wave alone, so its order is what it is at
// PARTS = 1.  At M >= 6 one wave's 64 float64 sums, their operands and the loads in flight leave one wave a SIMD; halved, three fit.
template <int M, int PARTS, int PART>
__device__ __forceinline__ void array_spatial_cov_add(const float (&re)[M], const float (&im)[M], double (&p)[M],
                                                      double (&qr)[M * (M - 1) / 2], double (&qi)[M * (M - 1) / 2]) {
#pragma clang fp contract(off)
    // both products of a term are exact in float64 (24 + 24 bits), so fma(a, b, c d) is the exact sum rounded once: the bits of
    // a b + c d with its one rounding, in one operation less
    double dr[M], di[M];
#pragma unroll
    for (int c = 0; c < M; ++c) {
        dr[c] = re[c];
        di[c] = im[c];
        p[c] += __builtin_fma(di[c], di[c], dr[c] * dr[c]);
    }
#pragma unroll
    for (int a = 0; a < M; ++a) {
#pragma unroll
        for (int b = a + 1; b < M; ++b) {
            const int q = array_spatial_pair(M, a, b);
            if (q % PARTS == PART) {
                qr[q] += __builtin_fma(di[a], di[b], dr[a] * dr[b]);
                qi[q] += __builtin_fma(-dr[a], di[b], di[a] * dr[b]);
            }
        }
    }
}

template <int M, int PARTS, int PART>
__device__ __forceinline__ void array_spatial_cov_part(const float2* __restrict__ e0, long plane, int lane, int T, float* __restrict__ o) {
#pragma clang fp contract(off)
    constexpr int P = M * (M - 1) / 2;
    double p[M], qr[P], qi[P];
#pragma unroll
    for (int c = 0; c < M; ++c) p[c] = 0.0;
#pragma unroll
    for (int q = 0; q < P; ++q) {
        qr[q] = 0.0;
        qi[q] = 0.0;
    }
    for (int t = 2 * lane; t < T; t += 128) {                  // t even and Tp a multiple of 64: t + 1 < Tp, 16-byte aligned
        float4 e[M];
#pragma unroll
        for (int c = 0; c < M; ++c) e[c] = *(const float4*)(e0 + c * plane + t);
        float re[M], im[M];
#pragma unroll
        for (int c = 0; c < M; ++c) {
            re[c] = e[c].x;
            im[c] = e[c].y;
        }
        array_spatial_cov_add<M, PARTS, PART>(re, im, p, qr, qi);
        if (t + 1 < T) {
#pragma unroll
            for (int c = 0; c < M; ++c) {
                re[c] = e[c].z;
                im[c] = e[c].w;
            }
            array_spatial_cov_add<M, PARTS, PART>(re, im, p, qr, qi);
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {                         // a + b == b + a: every lane ends with the same sums
#pragma unroll
        for (int c = 0; c < M; ++c) p[c] += __shfl_xor(p[c], m);
#pragma unroll
        for (int q = 0; q < P; ++q) {
            if (q % PARTS == PART) {
                qr[q] += __shfl_xor(qr[q], m);
                qi[q] += __shfl_xor(qi[q], m);
            }
        }
    }
    if (lane == 0) {
        double tr = p[0];
#pragma unroll
        for (int c = 1; c < M; ++c) tr = tr + p[c];
        const double n = tr / (double)M, lambda = GCCNMF_ARRAY_SPATIAL_LOADING;
        const bool none = n == 0.0;                            // false for NaN: NaN / Inf take the quotients and propagate
        if (PART == 0) {
#pragma unroll
            for (int c = 0; c < M; ++c) o[c] = (float)((none ? 1.0 : p[c] / n) + lambda);
        }
#pragma unroll
        for (int q = 0; q < P; ++q) {
            if (q % PARTS == PART) {
                o[M + 2 * q] = (float)(none ? 0.0 : qr[q] / n);
                o[M + 2 * q + 1] = (float)(none ? 0.0 : qi[q] / n);
            }
        }
    }
}

// grid = (F / (4 / PARTS) rounded up, S, batch), 4 waves a workgroup: wave w of workgroup x owns part w % PARTS of bin (4 x + w) / PARTS
template <int M>
__global__ __launch_bounds__(256) void array_spatial_cov_kernel(const float2* __restrict__ spec, int nsig_pitch, int F, int Fp, int T, int Tp,
                                                                int S, float* __restrict__ cov) {
    constexpr int PARTS = M >= 6 ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f = w / PARTS, part = w % PARTS;
    const int i = blockIdx.y, b = blockIdx.z;
    if (f >= F) return;                                        // wave-uniform
    const long plane = (long)Fp * Tp;
    const float2* __restrict__ e0 = spec + ((long)b * nsig_pitch + (long)i * M) * plane + (long)f * Tp;
    float* __restrict__ o = cov + (((long)b * S + i) * Fp + f) * (M * M);
    if (PARTS == 1 || part == 0) array_spatial_cov_part<M, PARTS, 0>(e0, plane, lane, T, o);
    else array_spatial_cov_part<M, PARTS, PARTS - 1>(e0, plane, lane, T, o);
}

// The S M M covariance floats of a row are read from LDS where they are used and not kept: a compiler barrier in front of each stage that
// reads them keeps the compiler from hoisting the (loop-invariant) reads out of the frame loop or carrying them from the solve to the
// outputs -- up to 512 registers at S = M = 8.  It orders nothing at run time and emits no instruction.
#define ARRAY_SPATIAL_REREAD() asm volatile("" ::: "memory")

// FR frames of one bin at M >= 3: the S powers v of each, the row's S cov rows r (M M floats each, wave-uniform, in LDS) and X -> the
// scaled powers w, y = Sigma_w^-1 X and whether the frame is silent (sum_j v_j == 0).  include/gccnmf_array_spatial.h states every
// operation below in this order; the frames of a lane share only the reads of r.
template <int M, int S, int FR>
__device__ __forceinline__ void array_spatial_solve(const float* __restrict__ r, const float (&v)[FR][S], const float (&xr)[FR][M],
                                                    const float (&xi)[FR][M], float (&w)[FR][S], float (&yr)[FR][M], float (&yi)[FR][M],
                                                    bool (&silent)[FR]) {
#pragma clang fp contract(off)
    constexpr int MM = M * M;
#pragma unroll
    for (int fr = 0; fr < FR; ++fr) {
        float vs = v[fr][0];
#pragma unroll
        for (int j = 1; j < S; ++j) vs = vs + v[fr][j];
        int e;
        (void)frexpf(vs, &e);                                  // e = 0 for a zero, infinite or NaN vs on gfx950 (the header says so)
#pragma unroll
        for (int j = 0; j < S; ++j) w[fr][j] = ldexpf(v[fr][j], -e);
        silent[fr] = vs == 0.f;                                // false for NaN: those propagate
    }
    float sg[FR][MM];                                          // Sigma_w, the layout of a cov row
#pragma unroll
    for (int g = 0; g < MM; ++g) {
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const float rv = r[j * MM + g];
#pragma unroll
            for (int fr = 0; fr < FR; ++fr) sg[fr][g] = j == 0 ? w[fr][0] * rv : sg[fr][g] + w[fr][j] * rv;
        }
    }
#pragma unroll
    for (int fr = 0; fr < FR; ++fr) {
        // Sigma_w = L D L^H, no pivoting: l[i][k] for i > k, d and its reciprocals
        float lr[M][M], li[M][M], d[M], rd[M];
#pragma unroll
        for (int k = 0; k < M; ++k) {
            float gr[M], gi[M];
#pragma unroll
            for (int m = 0; m < k; ++m) {
                gr[m] = lr[k][m] * d[m];
                gi[m] = li[k][m] * d[m];
            }
            float dk = sg[fr][k];
#pragma unroll
            for (int m = 0; m < k; ++m) dk = dk - (lr[k][m] * gr[m] + li[k][m] * gi[m]);
            d[k] = dk;
            rd[k] = 1.0f / dk;
#pragma unroll
            for (int i = k + 1; i < M; ++i) {
                float cr = sg[fr][M + 2 * array_spatial_pair(M, k, i)], ci = -sg[fr][M + 2 * array_spatial_pair(M, k, i) + 1];
#pragma unroll
                for (int m = 0; m < k; ++m) {
                    cr = cr - (lr[i][m] * gr[m] + li[i][m] * gi[m]);
                    ci = ci - (li[i][m] * gr[m] - lr[i][m] * gi[m]);
                }
                lr[i][k] = cr * rd[k];
                li[i][k] = ci * rd[k];
            }
        }
        float zr[M], zi[M];
#pragma unroll
        for (int i = 0; i < M; ++i) {                          // forward substitution
            float ar = xr[fr][i], ai = xi[fr][i];
#pragma unroll
            for (int k = 0; k < i; ++k) {
                ar = ar - (lr[i][k] * zr[k] - li[i][k] * zi[k]);
                ai = ai - (lr[i][k] * zi[k] + li[i][k] * zr[k]);
            }
            zr[i] = ar;
            zi[i] = ai;
        }
#pragma unroll
        for (int k = 0; k < M; ++k) {
            zr[k] = zr[k] * rd[k];
            zi[k] = zi[k] * rd[k];
        }
#pragma unroll
        for (int k = M - 1; k >= 0; --k) {                     // back substitution
            float ar = zr[k], ai = zi[k];
#pragma unroll
            for (int i = k + 1; i < M; ++i) {
                ar = ar - (lr[i][k] * yr[fr][i] + li[i][k] * yi[fr][i]);
                ai = ai - (lr[i][k] * yi[fr][i] - li[i][k] * yr[fr][i]);
            }
            yr[fr][k] = ar;
            yi[fr][k] = ai;
        }
    }
}

// Row a of u = R~ y for FR frames (ri: the M M floats of one cov row): u_a = R~_a0 y_0, then + R~_ab y_b, b ascending
template <int M, int FR>
__device__ __forceinline__ void array_spatial_row(const float* __restrict__ ri, int a, const float (&yr)[FR][M], const float (&yi)[FR][M],
                                                  float (&ur)[FR], float (&ui)[FR]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int b = 0; b < M; ++b) {
        const int q = b == a ? a : M + 2 * (a < b ? array_spatial_pair(M, a, b) : array_spatial_pair(M, b, a));
        const float pr = ri[q], pi = b == a ? 0.f : ri[q + 1];
#pragma unroll
        for (int fr = 0; fr < FR; ++fr) {
            float tr, ti;
            if (b == a) {
                tr = pr * yr[fr][b];
                ti = pr * yi[fr][b];
            } else if (a < b) {
                tr = pr * yr[fr][b] - pi * yi[fr][b];
                ti = pr * yi[fr][b] + pi * yr[fr][b];
            } else {                                           // conj(stored pair (b, a))
                tr = pr * yr[fr][b] + pi * yi[fr][b];
                ti = pr * yi[fr][b] - pi * yr[fr][b];
            }
            ur[fr] = b == 0 ? tr : ur[fr] + tr;
            ui[fr] = b == 0 ? ti : ui[fr] + ti;
        }
    }
}

template <int FR>
struct ArraySpatialVec;
template <>
struct ArraySpatialVec<1> {
    typedef float2 type;
};
template <>
struct ArraySpatialVec<2> {
    typedef float4 type;
};
__device__ __forceinline__ float2 array_spatial_get(const float2 v, int) { return v; }
__device__ __forceinline__ float2 array_spatial_get(const float4 v, int fr) { return fr ? make_float2(v.z, v.w) : make_float2(v.x, v.y); }
// v = (sum_c |E_c|^2) / M of frame fr of the loaded estimates: the channels ascending, then the IEEE quotient
template <int M, int FR>
__device__ __forceinline__ float array_spatial_power(const typename ArraySpatialVec<FR>::type (&e)[M], int fr) {
#pragma clang fp contract(off)
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < M; ++c) {
        const float2 a = array_spatial_get(e[c], fr);
        const float term = a.x * a.x + a.y * a.y;
        s = c == 0 ? term : s + term;
    }
    return s / (float)M;
}
__device__ __forceinline__ void array_spatial_put(float2* p, const float2 (&o)[1]) { *p = o[0]; }
__device__ __forceinline__ void array_spatial_put(float2* p, const float2 (&o)[2]) {
    *(float4*)p = make_float4(o[0].x, o[0].y, o[1].x, o[1].y);
}

// grid = (Fp / 4, batch), 4 waves a workgroup: wave w of workgroup x owns row 4 x + w (< Fp: Fp is a multiple of 16)
// WS: the powers come from the workspace of the EM refinement (array_spatial_em.hip; [batch][S][Fp][Tp], frames < T) instead of the
// estimates in spec, which is then only written.
template <int M, int S, bool WS>
__global__ __launch_bounds__(256) void array_spatial_filter_kernel(const float2* __restrict__ X, const float* __restrict__ cov,
                                                                   const float* __restrict__ powers, int nsig_pitch, int F, int Fp, int T,
                                                                   int Tp, float2* spec) {
#pragma clang fp contract(off)
    constexpr int MM = M * M, FR = M <= 4 ? 2 : 1;
    typedef typename ArraySpatialVec<FR>::type vec;
    __shared__ __attribute__((aligned(16))) float sR[4][S * MM];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f = blockIdx.x * 4 + wave;
    const int b = blockIdx.y;
    const long plane = (long)Fp * Tp;
    // the row's S cov rows: row f of target i at ((b S + i) Fp + f) M M, inside the buffer for every f < Fp
    if (lane < MM) {
#pragma unroll
        for (int i = 0; i < S; ++i) sR[wave][i * MM + lane] = cov[(((long)b * S + i) * Fp + f) * MM + lane];
    }
    __syncthreads();
    float2* O = spec + (long)b * nsig_pitch * plane + (long)f * Tp;                      // plane i M + c at O + (i M + c) * plane
    if (f >= F) {                                                                         // wave-uniform: the padding rows
        float2 zero[FR];
#pragma unroll
        for (int fr = 0; fr < FR; ++fr) zero[fr] = make_float2(0.f, 0.f);
        for (int t = FR * lane; t < Tp; t += 64 * FR) {
#pragma unroll
            for (int j = 0; j < S * M; ++j) array_spatial_put(O + j * plane + t, zero);
        }
        return;
    }
    const float2* __restrict__ x0 = X + (long)b * M * plane + (long)f * Tp;
    const float* __restrict__ r = sR[wave];
    for (int t = FR * lane; t < Tp; t += 64 * FR) {            // frames t ... t + FR - 1 < Tp
        float v[FR][S], xr[FR][M], xi[FR][M];
        if constexpr (WS) {
            const float* __restrict__ P = powers + (long)b * S * plane + (long)f * Tp + t;
#pragma unroll
            for (int i = 0; i < S; ++i) {
#pragma unroll
                for (int fr = 0; fr < FR; ++fr) v[fr][i] = t + fr < T ? P[i * plane + fr] : 0.f;
            }
        } else {
#pragma unroll
            for (int i = 0; i < S; ++i) {
                vec e[M];
#pragma unroll
                for (int c = 0; c < M; ++c) e[c] = *(const vec*)(O + (i * M + c) * plane + t);
#pragma unroll
                for (int fr = 0; fr < FR; ++fr) {
                    if constexpr (M == 2) {
                        const float2 a = array_spatial_get(e[0], fr), c = array_spatial_get(e[1], fr);
                        v[fr][i] = spatial_power(a.x, a.y, c.x, c.y);
                    } else {
                        v[fr][i] = array_spatial_power<M, FR>(e, fr);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < M; ++c) {
            const vec x = *(const vec*)(x0 + c * plane + t);
#pragma unroll
            for (int fr = 0; fr < FR; ++fr) {
                const float2 a = array_spatial_get(x, fr);
                xr[fr][c] = a.x;
                xi[fr][c] = a.y;
            }
        }
        if constexpr (M == 2) {
            float4 r4[S];
#pragma unroll
            for (int i = 0; i < S; ++i) r4[i] = *(const float4*)(r + 4 * i);
            float2 o[2 * S][FR];
#pragma unroll
            for (int fr = 0; fr < FR; ++fr) {
                float2 o0[S], o1[S];
                spatial_frame<S>(r4, v[fr], xr[fr][0], xi[fr][0], xr[fr][1], xi[fr][1], t + fr < T, o0, o1);
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    o[2 * i][fr] = o0[i];
                    o[2 * i + 1][fr] = o1[i];
                }
            }
#pragma unroll
            for (int j = 0; j < 2 * S; ++j) array_spatial_put(O + j * plane + t, o[j]);
        } else {
            float w[FR][S], yr[FR][M], yi[FR][M];
            bool silent[FR];
            ARRAY_SPATIAL_REREAD();
            array_spatial_solve<M, S, FR>(r, v, xr, xi, w, yr, yi, silent);
#pragma unroll
            for (int i = 0; i < S; ++i) {
                ARRAY_SPATIAL_REREAD();
#pragma unroll
                for (int a = 0; a < M; ++a) {
                    float ur[FR], ui[FR];
                    array_spatial_row<M, FR>(r + i * MM, a, yr, yi, ur, ui);
                    float2 o[FR];
#pragma unroll
                    for (int fr = 0; fr < FR; ++fr) {
                        const bool live = t + fr < T && !silent[fr];
                        o[fr] = live ? make_float2(w[fr][i] * ur[fr], w[fr][i] * ui[fr]) : make_float2(0.f, 0.f);
                    }
                    array_spatial_put(O + (i * M + a) * plane + t, o);
                }
            }
        }
    }
}

// WS is the caller's: a library holds only the form it launches (powers is null, and not read, at WS = false)
template <int M, int S, bool WS>
static void array_spatial_filter_launch(const float* X, const float* cov, const float* powers, int nsig_pitch, int F, int Fp, int T, int Tp,
                                        int batch, float* spec, hipStream_t s) {
    hipLaunchKernelGGL((array_spatial_filter_kernel<M, S, WS>), dim3(Fp / 4, batch), dim3(256), 0, s, (const float2*)X, cov, powers, nsig_pitch,
                       F, Fp, T, Tp, (float2*)spec);
}

// The two launches on their own, for the EM refinement between them (array_spatial_em.hip)
template <int M>
static void array_spatial_cov_launch(int nsig_pitch, int F, int Fp, int T, int Tp, int S, int batch, const float* spec, float* cov,
                                     hipStream_t s) {
    hipLaunchKernelGGL(array_spatial_cov_kernel<M>, dim3(gccnmf_ceil_div(F * (M >= 6 ? 2 : 1), 4), S, batch), dim3(256), 0, s, (const float2*)spec, nsig_pitch, F,
                       Fp, T, Tp, S, cov);
}

template <int M, bool WS>
static void array_spatial_filter_dispatch(const float* X, const float* cov, const float* powers, int nsig_pitch, int F, int Fp, int T, int Tp,
                                          int S, int batch, float* spec, hipStream_t s) {
    switch (S) {
        case 1: array_spatial_filter_launch<M, 1, WS>(X, cov, powers, nsig_pitch, F, Fp, T, Tp, batch, spec, s); break;
        case 2: array_spatial_filter_launch<M, 2, WS>(X, cov, powers, nsig_pitch, F, Fp, T, Tp, batch, spec, s); break;
        case 3: array_spatial_filter_launch<M, 3, WS>(X, cov, powers, nsig_pitch, F, Fp, T, Tp, batch, spec, s); break;
        case 4: array_spatial_filter_launch<M, 4, WS>(X, cov, powers, nsig_pitch, F, Fp, T, Tp, batch, spec, s); break;
        case 5: array_spatial_filter_launch<M, 5, WS>(X, cov, powers, nsig_pitch, F, Fp, T, Tp, batch, spec, s); break;
        case 6: array_spatial_filter_launch<M, 6, WS>(X, cov, powers, nsig_pitch, F, Fp, T, Tp, batch, spec, s); break;
        case 7: array_spatial_filter_launch<M, 7, WS>(X, cov, powers, nsig_pitch, F, Fp, T, Tp, batch, spec, s); break;
        default: array_spatial_filter_launch<M, 8, WS>(X, cov, powers, nsig_pitch, F, Fp, T, Tp, batch, spec, s); break;
    }
}

template <int M>
static void array_spatial_launch(const float* X, int nsig_pitch, int F, int Fp, int T, int Tp, int S, int batch, float* cov, float* spec,
                                 hipStream_t s) {
    array_spatial_cov_launch<M>(nsig_pitch, F, Fp, T, Tp, S, batch, spec, cov, s);
    array_spatial_filter_dispatch<M, false>(X, cov, nullptr, nsig_pitch, F, Fp, T, Tp, S, batch, spec, s);
}

static bool array_spatial_shape_ok(int M, int F, int S, int batch) {
    return M >= GCCNMF_ARRAY_SPATIAL_MIN_CHANNELS && M <= GCCNMF_ARRAY_SPATIAL_MAX_CHANNELS && S >= 1 && S <= GCCNMF_ARRAY_SPATIAL_MAX_TARGETS &&
           F >= 2 && batch >= 1 && (long)M * batch <= 65535;
}

#ifndef ARRAY_SPATIAL_KERNELS_ONLY                             // (array_spatial_em.hip includes this file for its kernels and launches)
extern "C" {

int gccnmf_array_spatial_version(void) { return ARRAY_SPATIAL_VERSION; }

long gccnmf_array_spatial_workspace_floats(int M, int F, int S, int batch) {
    if (!array_spatial_shape_ok(M, F, S, batch)) return -1;
    return (long)batch * S * gccnmf_round_up(F, 16) * M * M;
}

int gccnmf_array_spatial(const float* X, int M, int F, int T, int S, int batch, int nsig_pitch, float* cov, float* spec, void* stream) {
    // every check comes before the first HIP call
    if (!X || !spec || !cov || ((uintptr_t)cov & 15) || M < GCCNMF_ARRAY_SPATIAL_MIN_CHANNELS || M > GCCNMF_ARRAY_SPATIAL_MAX_CHANNELS || F < 2 ||
        T < 1 || batch < 1)
        return GCCNMF_ERR_ARG;
    if (S < 1 || S > GCCNMF_ARRAY_SPATIAL_MAX_TARGETS) return GCCNMF_ERR_UNSUPPORTED;
    if (nsig_pitch < S * M) return GCCNMF_ERR_ARG;
    if ((long)M * T > 0x7fffffffL - 64 || (long)M * batch > 65535) return GCCNMF_ERR_UNSUPPORTED;
    const int Fp = gccnmf_round_up(F, 16), Tp = gccnmf_round_up(T, 64);
    hipStream_t s = (hipStream_t)stream;
    switch (M) {
        case 2: array_spatial_launch<2>(X, nsig_pitch, F, Fp, T, Tp, S, batch, cov, spec, s); break;
        case 3: array_spatial_launch<3>(X, nsig_pitch, F, Fp, T, Tp, S, batch, cov, spec, s); break;
        case 4: array_spatial_launch<4>(X, nsig_pitch, F, Fp, T, Tp, S, batch, cov, spec, s); break;
        case 5: array_spatial_launch<5>(X, nsig_pitch, F, Fp, T, Tp, S, batch, cov, spec, s); break;
        case 6: array_spatial_launch<6>(X, nsig_pitch, F, Fp, T, Tp, S, batch, cov, spec, s); break;
        case 7: array_spatial_launch<7>(X, nsig_pitch, F, Fp, T, Tp, S, batch, cov, spec, s); break;
        default: array_spatial_launch<8>(X, nsig_pitch, F, Fp, T, Tp, S, batch, cov, spec, s); break;
    }
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

}  // extern "C"
#endif
