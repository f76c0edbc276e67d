// EM refinement of the spatial (multichannel Wiener) filter: n iterations of the local Gaussian model EM (Duong, Vincent & Gribonval 2010)
// between the two launches of spatial.hip, which are its initialisation (v_i, R~_i of the ratio-mode estimates) and its output stage
// (S'_i = v_i R~_i Sigma^-1 X).  include/gccnmf_hip.h states the recursion; spatial.h holds the arithmetic of one (bin, frame).
//
// One launch for all n iterations.  A (file, bin) row is independent of every other row -- R~_i[f] and v_i[f, .] depend on that row
// alone -- and belongs to ONE wave for the whole launch: the wave sweeps the row's frames, two consecutive frames per lane and step as
// the filter kernel does (16-byte loads of X), keeps the new powers in the workspace [batch][S][Fp][Tp] (each float2 is read back, in
// the next sweep, by the lane that wrote it: no barrier, no fence), adds the float32 terms C_i / v'_i of its frames in float64 -- lane l
// frames 2l, 2l+1, 2l+128, ... in that order -- combines the 64 partials of the 4 S sums and the S counts in the fixed xor butterfly
// of the covariance kernel (a + b == b + a: every lane ends with the same sums, and the order depends on T alone), forms R~' and
// sweeps again.  No atomic, no counter, no cross-workgroup dependency; a file gives the same bits alone and in any batch.  The first
// sweep takes the powers from the estimates in spec (the filter kernel's spatial_power), the later ones from the workspace.
//
// R~ is wave-uniform: read through the scalar cache before the first sweep, broadcast from lane 0 after every reduction.
//
// Built with -ffp-contract=off, as spatial.hip: every product and sum is its own float32 rounding in the order written.
#include "spatial.h"
#include "../../include/gccnmf_hip.h"

__device__ __forceinline__ float spatial_em_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

template <int S>
__global__ __launch_bounds__(256) void gcc_spatial_em_kernel(const float2* __restrict__ X, const float2* __restrict__ spec,
                                                             int F, int Fp, int T, int Tp, int n, float4* cov, float* powers) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    if (f >= F) return;                                        // wave-uniform: the padding rows have no covariance
    const long plane = (long)Fp * Tp;
    const float2* __restrict__ E = spec + (long)b * 2 * S * plane + (long)f * Tp;         // plane i*2+c at E + (i*2+c) * plane
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
            } else {
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
            const double load = GCCNMF_SPATIAL_LOADING * (0.5 * (r00 + r11));
            r[i] = make_float4(spatial_em_uniform((float)(r00 + load)), spatial_em_uniform((float)(r11 + load)),
                               spatial_em_uniform((float)r01r), spatial_em_uniform((float)r01i));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < S; ++i) cov[((long)b * S + i) * Fp + f] = r[i];
    }
}

template <int S>
static void spatial_em_launch(const float* X, const float* spec, int F, int Fp, int T, int Tp, int batch, int n, float* cov, float* powers,
                              hipStream_t s) {
    hipLaunchKernelGGL((gcc_spatial_em_kernel<S>), dim3(gccnmf_ceil_div(F, 4), batch), dim3(256), 0, s, (const float2*)X, (const float2*)spec,
                       F, Fp, T, Tp, n, (float4*)cov, powers);
}

int gccnmf_launch_spatial_em(const float* X, int F, int T, int S, int batch, int n, float* cov, float* powers, float* spec, hipStream_t s) {
    if (S < 1 || S > GCCNMF_SPATIAL_MAX_TARGETS || batch > 65535 || n < 1) return GCCNMF_ERR_UNSUPPORTED;
    GccNmfPitches p = gccnmf_make_pitches(F, T, 1);
    int rc = gccnmf_launch_spatial_cov(F, T, S, batch, spec, cov, s);
    if (rc != GCCNMF_OK) return rc;
    switch (S) {
        case 1: spatial_em_launch<1>(X, spec, F, p.Fp, T, p.Tp, batch, n, cov, powers, s); break;
        case 2: spatial_em_launch<2>(X, spec, F, p.Fp, T, p.Tp, batch, n, cov, powers, s); break;
        case 3: spatial_em_launch<3>(X, spec, F, p.Fp, T, p.Tp, batch, n, cov, powers, s); break;
        case 4: spatial_em_launch<4>(X, spec, F, p.Fp, T, p.Tp, batch, n, cov, powers, s); break;
        case 5: spatial_em_launch<5>(X, spec, F, p.Fp, T, p.Tp, batch, n, cov, powers, s); break;
        case 6: spatial_em_launch<6>(X, spec, F, p.Fp, T, p.Tp, batch, n, cov, powers, s); break;
        case 7: spatial_em_launch<7>(X, spec, F, p.Fp, T, p.Tp, batch, n, cov, powers, s); break;
        default: spatial_em_launch<8>(X, spec, F, p.Fp, T, p.Tp, batch, n, cov, powers, s); break;
    }
    GCCNMF_CHECK_LAUNCH();
    return gccnmf_launch_spatial_filter(X, cov, powers, F, T, S, batch, spec, s);
}
