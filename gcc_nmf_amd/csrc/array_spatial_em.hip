// libgccnmf_array_em.so: EM refinement of the M x M spatial filter of the microphone-array path -- n iterations of the local Gaussian
// model EM (Duong, Vincent & Gribonval 2010) between the two launches of array_spatial.hip, which are its initialisation (v_i, R~_i of the
// ratio-mode estimates) and its output stage.  include/gccnmf_array_em.h states the recursion operation by operation; DESIGN section 4j.
// The M-channel form of spatial_em.hip.  The covariance and filter kernels, the powers and u = R~ y are those of array_spatial.hip,
// included below without its entry points.  Two things are stated a second time, and say so where they stand: the M = 2 kernel is the
// loop of gcc_spatial_em_kernel (spatial_em.hip belongs to the separation library, and its kernel takes that library's spec pitch 2 S;
// sharing the loop would change that file), and the LDL^H solve is array_spatial_solve's in two parts (that function stays as it is, so
// that the filter kernels keep their machine code).
//
// One launch for all n iterations, one workgroup per (file, bin) row for the whole launch: no atomic, no counter, no cross-workgroup
// dependency; a file gives the same bits alone and in any batch.
//
// M = 2 (array_em2_kernel<S>): one wave per row runs spatial_em_frame of spatial.h as gcc_spatial_em_kernel does, so that cov, the powers
// and spec hold the bits of the stereo call.
//
// M >= 3 (array_em_kernel<M>, S a run-time loop): the workgroup has one wave per target.  Wave i keeps only its own M M float64 sums:
// S M M of them (512 at S = M = 8) do not fit one wave.  Every wave factorises Sigma_w of its frames itself (the S waves repeat that
// work; it is the smaller part of a frame -- one factorisation against M + 1 substitutions).  The row's S cov rows sit in LDS and are
// replaced there after every sweep; the powers live in the workspace [batch][S][Fp][Tp]: the waves first write the powers of the
// estimates there (wave i its own target's), and a sweep reads all S powers of a frame and writes its own target's new one.  The sweep
// walks the row in steps of 128 frames -- lane l takes frames 2l and 2l+1 of the step, the order of the covariance launch -- and a
// workgroup barrier between a step's reads and its stores keeps a new power from a wave that has not read the old one yet; a barrier
// after the sweep publishes the new cov rows and powers.  The 64 partials of a sum are combined in the fixed xor butterfly of the
// covariance kernel (a + b == b + a: every lane ends with the same sums, and the order depends on T alone).
//
// Built with -ffp-contract=off; every product and sum below is its own float32 rounding, in the order written.
#define ARRAY_SPATIAL_KERNELS_ONLY
#include "array_spatial.hip"
#include "../../include/gccnmf_array_em.h"

#define ARRAY_EM_VERSION 100

__device__ __forceinline__ float array_em_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// ---- M = 2: gcc_spatial_em_kernel on the array's buffers (spec has nsig_pitch slots a file) ------------------------------------------------
// A copy of that kernel's loop (csrc/spatial_em.hip) with three differences: the file stride of spec, the loading macro, the name of the
// broadcast helper.  The arithmetic of a frame is shared (spatial_em_frame of spatial.h); tests/test_gpu_array_em_stages.py holds the two
// kernels together bit for bit in all three buffers.
// grid = (F / 4 rounded up, batch), 4 waves a workgroup, a wave a row
template <int S>
__global__ __launch_bounds__(256) void array_em2_kernel(const float2* __restrict__ X, const float2* __restrict__ spec, int nsig_pitch, int F,
                                                        int Fp, int T, int Tp, int n, float4* cov, float* powers) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    if (f >= F) return;                                        // wave-uniform: the padding rows have no covariance
    const long plane = (long)Fp * Tp;
    const float2* __restrict__ E = spec + (long)b * nsig_pitch * plane + (long)f * Tp;    // plane i*2+c at E + (i*2+c) * plane
    const float2* __restrict__ x0 = X + (long)b * 2 * plane + (long)f * Tp;
    const float2* __restrict__ x1 = x0 + plane;
    float* P = powers + (long)b * S * plane + (long)f * Tp;                               // target i at P + i * plane
    float4 r[S];
#pragma unroll
    for (int i = 0; i < S; ++i) r[i] = cov[((long)b * S + i) * Fp + f];
    for (int m = 0; m < n; ++m) {
        double acc[S][4];
        int cnt[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0;
            cnt[i] = 0;
        }
        for (int t = 2 * lane; t < T; t += 128) {              // t even and Tp a multiple of 64: t + 1 < Tp, 16-byte aligned
            const float4 xa = *(const float4*)(x0 + t);
            const float4 xb = *(const float4*)(x1 + t);
            float va[S], vb[S];
            if (m == 0) {                                      // wave-uniform
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    const float4 e0 = *(const float4*)(E + (2 * i) * plane + t);
                    const float4 e1 = *(const float4*)(E + (2 * i + 1) * plane + t);
                    va[i] = spatial_power(e0.x, e0.y, e1.x, e1.y);
                    vb[i] = spatial_power(e0.z, e0.w, e1.z, e1.w);
                }
            } else {                                           // each float2 is read back by the lane that wrote it
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    const float2 p = *(const float2*)(P + i * plane + t);
                    va[i] = p.x;
                    vb[i] = p.y;
                }
            }
            float na[S], nb[S];
            float4 term[S];
            spatial_em_frame<S>(r, va, xa.x, xa.y, xb.x, xb.y, na, term);
#pragma unroll
            for (int i = 0; i < S; ++i) {
                if (!(na[i] == 0.f)) {                         // a NaN power counts: its term is NaN too
                    acc[i][0] += (double)term[i].x;
                    acc[i][1] += (double)term[i].y;
                    acc[i][2] += (double)term[i].z;
                    acc[i][3] += (double)term[i].w;
                    cnt[i] += 1;
                }
            }
            if (t + 1 < T) {
                spatial_em_frame<S>(r, vb, xa.z, xa.w, xb.z, xb.w, nb, term);
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    if (!(nb[i] == 0.f)) {
                        acc[i][0] += (double)term[i].x;
                        acc[i][1] += (double)term[i].y;
                        acc[i][2] += (double)term[i].z;
                        acc[i][3] += (double)term[i].w;
                        cnt[i] += 1;
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < S; ++i) nb[i] = 0.f;
            }
#pragma unroll
            for (int i = 0; i < S; ++i) *(float2*)(P + i * plane + t) = make_float2(na[i], nb[i]);
        }
#pragma unroll
        for (int i = 0; i < S; ++i) {
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) {
                acc[i][0] += __shfl_xor(acc[i][0], k);
                acc[i][1] += __shfl_xor(acc[i][1], k);
                acc[i][2] += __shfl_xor(acc[i][2], k);
                acc[i][3] += __shfl_xor(acc[i][3], k);
                cnt[i] += __shfl_xor(cnt[i], k);
            }
            double r00 = 1.0, r11 = 1.0, r01r = 0.0, r01i = 0.0;
            if (cnt[i] != 0) {                                 // NaN / Inf take the quotients and propagate
                const double c = (double)cnt[i];
                r00 = acc[i][0] / c;
                r11 = acc[i][1] / c;
                r01r = acc[i][2] / c;
                r01i = acc[i][3] / c;
            }
            const double load = GCCNMF_ARRAY_SPATIAL_LOADING * (0.5 * (r00 + r11));
            r[i] = make_float4(array_em_uniform((float)(r00 + load)), array_em_uniform((float)(r11 + load)), array_em_uniform((float)r01r),
                               array_em_uniform((float)r01i));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < S; ++i) cov[((long)b * S + i) * Fp + f] = r[i];
    }
}

// ---- M >= 3 ------------------------------------------------------------------------------------------------------------------------------
// The LDL^H solve of array_spatial_solve (array_spatial.hip) in two parts, so that one factorisation serves the M + 1 right-hand sides of a
// frame: the same operations in the same order, stated here a second time because that function, and with it the machine code of the
// filter kernels, stays as it is.
// Sigma_w = L D L^H of one frame, no pivoting (sg: the layout of a cov row): l[i][k] for i > k and the reciprocals of the pivots
template <int M>
__device__ __forceinline__ void array_spatial_factor(const float (&sg)[M * M], float (&lr)[M][M], float (&li)[M][M], float (&rd)[M]) {
#pragma clang fp contract(off)
    float d[M];
#pragma unroll
    for (int k = 0; k < M; ++k) {
        float gr[M], gi[M];
#pragma unroll
        for (int m = 0; m < k; ++m) {
            gr[m] = lr[k][m] * d[m];
            gi[m] = li[k][m] * d[m];
        }
        float dk = sg[k];
#pragma unroll
        for (int m = 0; m < k; ++m) dk = dk - (lr[k][m] * gr[m] + li[k][m] * gi[m]);
        d[k] = dk;
        rd[k] = 1.0f / dk;
#pragma unroll
        for (int i = k + 1; i < M; ++i) {
            float cr = sg[M + 2 * array_spatial_pair(M, k, i)], ci = -sg[M + 2 * array_spatial_pair(M, k, i) + 1];
#pragma unroll
            for (int m = 0; m < k; ++m) {
                cr = cr - (lr[i][m] * gr[m] + li[i][m] * gi[m]);
                ci = ci - (li[i][m] * gr[m] - lr[i][m] * gi[m]);
            }
            lr[i][k] = cr * rd[k];
            li[i][k] = ci * rd[k];
        }
    }
}

// y = (L D L^H)^-1 x of one frame: the forward substitution, the scaling and the back substitution
template <int M>
__device__ __forceinline__ void array_spatial_substitute(const float (&lr)[M][M], const float (&li)[M][M], const float (&rd)[M],
                                                         const float (&xr)[M], const float (&xi)[M], float (&yr)[M], float (&yi)[M]) {
#pragma clang fp contract(off)
    float zr[M], zi[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {                              // forward substitution
        float ar = xr[i], ai = xi[i];
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
    for (int k = M - 1; k >= 0; --k) {                         // back substitution
        float ar = zr[k], ai = zi[k];
#pragma unroll
        for (int i = k + 1; i < M; ++i) {
            ar = ar - (lr[i][k] * yr[i] + li[i][k] * yi[i]);
            ai = ai - (lr[i][k] * yi[i] - li[i][k] * yr[i]);
        }
        yr[k] = ar;
        yi[k] = ai;
    }
}

// One frame of one iteration for target i (wave-uniform): the row's S cov rows sR (LDS), the S old powers of the frame at Pt + j * plane
// and X -> the new power vn (unscaled; 0 where sum_j v_j = 0) and, where vn is not 0, the M M components of the frame's term C_i / v'_i
// in the layout of a cov row.  The header states every operation below in this order.
template <int M>
__device__ __forceinline__ void array_em_frame(const float* sR, const float* Pt, long plane, int S, int i, const float (&xr)[M],
                                               const float (&xi)[M], float& vn, float (&term)[M * M]) {
#pragma clang fp contract(off)
    constexpr int MM = M * M;
    float vs = Pt[0];
    for (int j = 1; j < S; ++j) vs = vs + Pt[j * plane];
    int e;
    (void)frexpf(vs, &e);                                      // e = 0 for a zero, infinite or NaN vs on gfx950
    const bool dead = vs == 0.f;                               // false for NaN
    // Sigma_w and N_i = sum_{j != i} w_j R~_j, ascending j: one product serves both sums
    float sg[MM], N[MM], wi = 0.f;
#pragma unroll
    for (int g = 0; g < MM; ++g) N[g] = 0.f;                   // S = 1: exact zeros
    bool first = true;
    for (int j = 0; j < S; ++j) {
        const float wj = ldexpf(Pt[j * plane], -e);
        const bool other = j != i;                             // wave-uniform
        if (!other) wi = wj;
#pragma unroll
        for (int g = 0; g < MM; ++g) {
            const float p = wj * sR[j * MM + g];
            sg[g] = j == 0 ? p : sg[g] + p;
            if (other) N[g] = first ? p : N[g] + p;
        }
        if (other) first = false;
    }
    float lr[M][M], li[M][M], rd[M];
    array_spatial_factor<M>(sg, lr, li, rd);
    float yr[1][M], yi[1][M];
    array_spatial_substitute<M>(lr, li, rd, xr, xi, yr[0], yi[0]);
    ARRAY_SPATIAL_REREAD();
    const float* __restrict__ ri = sR + i * MM;
    // u = R~_i y and h = Re(y^H u)
    float ur[M], ui[M], h = 0.f;
#pragma unroll
    for (int a = 0; a < M; ++a) {
        float tr[1], ti[1];
        array_spatial_row<M, 1>(ri, a, yr, yi, tr, ti);
        ur[a] = tr[0];
        ui[a] = ti[0];
        const float q = yr[0][a] * ur[a] + yi[0][a] * ui[a];
        h = a == 0 ? q : h + q;
    }
    // W = Sigma_w^-1 N_i column by column;  k = Re tr W;  P = R~_i W, its stored components (P is Hermitian)
    float P[MM], k = 0.f;
#pragma unroll
    for (int b = 0; b < M; ++b) {
        float cr[M], ci[M], wr[1][M], wim[1][M];
#pragma unroll
        for (int c = 0; c < M; ++c) {                          // N_cb: the stored pair for c < b, its conjugate for c > b
            if (c == b) {
                cr[c] = N[b];
                ci[c] = 0.f;
            } else if (c < b) {
                cr[c] = N[M + 2 * array_spatial_pair(M, c, b)];
                ci[c] = N[M + 2 * array_spatial_pair(M, c, b) + 1];
            } else {
                cr[c] = N[M + 2 * array_spatial_pair(M, b, c)];
                ci[c] = -N[M + 2 * array_spatial_pair(M, b, c) + 1];
            }
        }
        array_spatial_substitute<M>(lr, li, rd, cr, ci, wr[0], wim[0]);
        k = b == 0 ? wr[0][b] : k + wr[0][b];
        ARRAY_SPATIAL_REREAD();
#pragma unroll
        for (int a = 0; a <= b; ++a) {
            float pr[1], pi[1];
            array_spatial_row<M, 1>(ri, a, wr, wim, pr, pi);
            if (a == b) {
                P[a] = pr[0];
            } else {
                P[M + 2 * array_spatial_pair(M, a, b)] = pr[0];
                P[M + 2 * array_spatial_pair(M, a, b) + 1] = pi[0];
            }
        }
    }
    const float v2 = (wi * h + ldexpf(k, e)) / (float)M;
    float vi = wi * v2;
    vi = vi < 0.f ? 0.f : vi;                                  // NaN stays
    vn = dead ? 0.f : vi;
    const float rv = 1.0f / v2;
#pragma unroll
    for (int a = 0; a < M; ++a) term[a] = (wi * (ur[a] * ur[a] + ui[a] * ui[a]) + ldexpf(P[a], e)) * rv;
#pragma unroll
    for (int a = 0; a < M; ++a) {
#pragma unroll
        for (int b = a + 1; b < M; ++b) {
            const int q = M + 2 * array_spatial_pair(M, a, b);
            term[q] = (wi * (ur[a] * ur[b] + ui[a] * ui[b]) + ldexpf(P[q], e)) * rv;
            term[q + 1] = (wi * (ui[a] * ur[b] - ur[a] * ui[b]) + ldexpf(P[q + 1], e)) * rv;
        }
    }
}

// grid = (F, batch), S waves a workgroup: the workgroup owns row f of file b, wave i its target i.  WAVES bounds S (4 or 8): a
// workgroup of at most 4 waves leaves a wave 512 registers, one of 8 leaves it 256.
template <int M, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void array_em_kernel(const float2* __restrict__ X, const float2* __restrict__ spec, int nsig_pitch, int Fp,
                                                       int T, int Tp, int S, int n, float* cov, float* powers) {
#pragma clang fp contract(off)
    constexpr int MM = M * M;
    __shared__ float sR[GCCNMF_ARRAY_SPATIAL_MAX_TARGETS * MM];
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f = blockIdx.x, b = blockIdx.y;
    const long plane = (long)Fp * Tp;
    const float2* __restrict__ E = spec + ((long)b * nsig_pitch + (long)i * M) * plane + (long)f * Tp;   // channel c of target i at E + c * plane
    const float2* __restrict__ x0 = X + (long)b * M * plane + (long)f * Tp;
    float* P = powers + (long)b * S * plane + (long)f * Tp;                                // target j at P + j * plane
    float* row = cov + (((long)b * S + i) * Fp + f) * MM;
    if (lane < MM) sR[i * MM + lane] = row[lane];
    for (int t = lane; t < T; t += 64) {                       // the powers of the estimates: array_spatial_filter_kernel's
        float2 e[M];
#pragma unroll
        for (int c = 0; c < M; ++c) e[c] = E[c * plane + t];
        P[i * plane + t] = array_spatial_power<M, 1>(e, 0);
    }
    __syncthreads();
    for (int m = 0; m < n; ++m) {
        double acc[MM];
#pragma unroll
        for (int g = 0; g < MM; ++g) acc[g] = 0.0;
        int cnt = 0;
        for (int t0 = 0; t0 < T; t0 += 128) {                  // workgroup-uniform: every wave meets the barrier of every step
            float va = 0.f, vb = 0.f;
#pragma unroll 1
            for (int fr = 0; fr < 2; ++fr) {                   // (one copy of the frame's code)
                const int t = t0 + 2 * lane + fr;
                if (t < T) {
                    float xr[M], xi[M], term[MM];
#pragma unroll
                    for (int c = 0; c < M; ++c) {
                        const float2 x = x0[c * plane + t];
                        xr[c] = x.x;
                        xi[c] = x.y;
                    }
                    float v;
                    array_em_frame<M>(sR, P + t, plane, S, i, xr, xi, v, term);
                    if (fr == 0) va = v;
                    else vb = v;
                    if (!(v == 0.f)) {                         // a NaN power counts: its term is NaN too
#pragma unroll
                        for (int g = 0; g < MM; ++g) acc[g] += (double)term[g];
                        cnt += 1;
                    }
                }
            }
            __syncthreads();                                   // every wave has read the old powers of this step's frames
            const int t = t0 + 2 * lane;
            if (t < T) P[i * plane + t] = va;
            if (t + 1 < T) P[i * plane + t + 1] = vb;
        }
        // (the last step's barrier stands behind every read of sR in this sweep)
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
#pragma unroll
            for (int g = 0; g < MM; ++g) acc[g] += __shfl_xor(acc[g], k);
            cnt += __shfl_xor(cnt, k);
        }
        const double c = (double)cnt;
        const bool none = cnt == 0;                            // NaN / Inf take the quotients and propagate
        double d[M], tr = 0.0;
#pragma unroll
        for (int a = 0; a < M; ++a) {
            d[a] = none ? 1.0 : acc[a] / c;
            tr = a == 0 ? d[a] : tr + d[a];
        }
        const double load = GCCNMF_ARRAY_SPATIAL_LOADING * (tr / (double)M);
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < M; ++a) sR[i * MM + a] = (float)(d[a] + load);
#pragma unroll
            for (int g = M; g < MM; ++g) sR[i * MM + g] = (float)(none ? 0.0 : acc[g] / c);
        }
        __syncthreads();                                       // the new cov rows and the new powers, for every wave
    }
    if (lane < MM) row[lane] = sR[i * MM + lane];
}

template <int S>
static void array_em2_launch(const float* X, const float* spec, int nsig_pitch, int F, int Fp, int T, int Tp, int batch, int n, float* cov,
                             float* powers, hipStream_t s) {
    hipLaunchKernelGGL((array_em2_kernel<S>), dim3(gccnmf_ceil_div(F, 4), batch), dim3(256), 0, s, (const float2*)X, (const float2*)spec,
                       nsig_pitch, F, Fp, T, Tp, n, (float4*)cov, powers);
}

// the three launches: the covariances of the estimates, n iterations, the filter on the refined powers and covariances
template <int M>
static void array_em_launch(const float* X, int nsig_pitch, int F, int Fp, int T, int Tp, int S, int batch, int n, float* cov, float* powers,
                            float* spec, hipStream_t s) {
    array_spatial_cov_launch<M>(nsig_pitch, F, Fp, T, Tp, S, batch, spec, cov, s);
    if constexpr (M == 2) {
        switch (S) {
            case 1: array_em2_launch<1>(X, spec, nsig_pitch, F, Fp, T, Tp, batch, n, cov, powers, s); break;
            case 2: array_em2_launch<2>(X, spec, nsig_pitch, F, Fp, T, Tp, batch, n, cov, powers, s); break;
            case 3: array_em2_launch<3>(X, spec, nsig_pitch, F, Fp, T, Tp, batch, n, cov, powers, s); break;
            case 4: array_em2_launch<4>(X, spec, nsig_pitch, F, Fp, T, Tp, batch, n, cov, powers, s); break;
            case 5: array_em2_launch<5>(X, spec, nsig_pitch, F, Fp, T, Tp, batch, n, cov, powers, s); break;
            case 6: array_em2_launch<6>(X, spec, nsig_pitch, F, Fp, T, Tp, batch, n, cov, powers, s); break;
            case 7: array_em2_launch<7>(X, spec, nsig_pitch, F, Fp, T, Tp, batch, n, cov, powers, s); break;
            default: array_em2_launch<8>(X, spec, nsig_pitch, F, Fp, T, Tp, batch, n, cov, powers, s); break;
        }
    } else {
        if (S <= 4)
            hipLaunchKernelGGL((array_em_kernel<M, 4>), dim3(F, batch), dim3(64 * S), 0, s, (const float2*)X, (const float2*)spec, nsig_pitch, Fp,
                               T, Tp, S, n, cov, powers);
        else
            hipLaunchKernelGGL((array_em_kernel<M, 8>), dim3(F, batch), dim3(64 * S), 0, s, (const float2*)X, (const float2*)spec, nsig_pitch, Fp,
                               T, Tp, S, n, cov, powers);
    }
    array_spatial_filter_dispatch<M, true>(X, cov, powers, nsig_pitch, F, Fp, T, Tp, S, batch, spec, s);
}

extern "C" {

int gccnmf_array_em_version(void) { return ARRAY_EM_VERSION; }

long gccnmf_array_em_workspace_floats(int M, int F, int T, int S, int batch) {
    if (!array_spatial_shape_ok(M, F, S, batch) || T < 1 || (long)M * T > 0x7fffffffL - 64) return -1;
    const long Fp = gccnmf_round_up(F, 16), Tp = gccnmf_round_up(T, 64);
    return (long)batch * S * Fp * M * M + (long)batch * S * Fp * Tp;
}

int gccnmf_array_em(const float* X, int M, int F, int T, int S, int batch, int nsig_pitch, int n, float* workspace, float* spec, void* stream) {
    // every check comes before the first HIP call: the rules of gccnmf_array_spatial, then n
    if (!X || !spec || !workspace || ((uintptr_t)workspace & 15) || M < GCCNMF_ARRAY_SPATIAL_MIN_CHANNELS || M > GCCNMF_ARRAY_SPATIAL_MAX_CHANNELS ||
        F < 2 || T < 1 || batch < 1)
        return GCCNMF_ERR_ARG;
    if (S < 1 || S > GCCNMF_ARRAY_SPATIAL_MAX_TARGETS) return GCCNMF_ERR_UNSUPPORTED;
    if (nsig_pitch < S * M) return GCCNMF_ERR_ARG;
    if ((long)M * T > 0x7fffffffL - 64 || (long)M * batch > 65535) return GCCNMF_ERR_UNSUPPORTED;
    if (n < 1 || n > GCCNMF_ARRAY_EM_MAX_ITERATIONS) return GCCNMF_ERR_UNSUPPORTED;
    const int Fp = gccnmf_round_up(F, 16), Tp = gccnmf_round_up(T, 64);
    float* cov = workspace;
    float* powers = workspace + (long)batch * S * Fp * M * M;  // Fp is a multiple of 16: 16-byte aligned
    hipStream_t s = (hipStream_t)stream;
    switch (M) {
        case 2: array_em_launch<2>(X, nsig_pitch, F, Fp, T, Tp, S, batch, n, cov, powers, spec, s); break;
        case 3: array_em_launch<3>(X, nsig_pitch, F, Fp, T, Tp, S, batch, n, cov, powers, spec, s); break;
        case 4: array_em_launch<4>(X, nsig_pitch, F, Fp, T, Tp, S, batch, n, cov, powers, spec, s); break;
        case 5: array_em_launch<5>(X, nsig_pitch, F, Fp, T, Tp, S, batch, n, cov, powers, spec, s); break;
        case 6: array_em_launch<6>(X, nsig_pitch, F, Fp, T, Tp, S, batch, n, cov, powers, spec, s); break;
        case 7: array_em_launch<7>(X, nsig_pitch, F, Fp, T, Tp, S, batch, n, cov, powers, spec, s); break;
        default: array_em_launch<8>(X, nsig_pitch, F, Fp, T, Tp, S, batch, n, cov, powers, spec, s); break;
    }
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

}  // extern "C"
