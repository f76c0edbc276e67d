// Spatial (multichannel Wiener) filter: the second stage of mask-based stereo separation under the local Gaussian model, run behind the
// ratio-mask reconstruction (ratio.hip) on its estimates S_i,c[f,t], in place.  With X[f,t] = (X_0, X_1)^T:
//
//   v_i[f,t] = 1/2 (|S_i,0|^2 + |S_i,1|^2)
//   R_i[f]   = [[p_0, q], [conj q, p_1]] / n,   p_c = sum_t |S_i,c|^2,  q = sum_t S_i,0 conj(S_i,1),  n = (p_0 + p_1) / 2   (float64;
//              R_i = I when n = 0);  R~_i = R_i + lambda I, rounded to float32 once
//   Sigma    = sum_j v_j R~_j (ascending j),  y = Sigma^-1 X (closed 2 x 2 Hermitian inverse),  S'_i = v_i R~_i y
//   every target 0 where sum_j v_j = 0;  rows >= F and frames >= T are written as zeros
//
// Two launches.  gcc_spatial_cov_kernel: one wave per (file, target, bin) reads the two channel rows once, 16 bytes (two frames) per lane
// and step; lane l adds frames 2l, 2l+1, 2l+128, ... in that order in float64 and the 64 partials are combined by a fixed xor butterfly,
// so the order of the sum depends on T alone: no atomics, and a file gives the same bits alone and in any batch.  gcc_spatial_filter_kernel:
// one wave per (file, bin) row; a lane owns two consecutive frames per step, loads its 2 S estimates and X (all loads in front of the
// first store: the S outputs need every v_j), keeps only the S powers v_j and writes the S filtered pairs over the estimates.  The R~ of
// a row are wave-uniform: their address is formed from blockIdx and a readfirstlane, so they arrive through the scalar cache.
//
// Built with -ffp-contract=off; every product and sum below is its own float32 rounding, in the order written.  The filter evaluates
// the formulas on w_j = v_j 2^-e, e the binary exponent of sum_j v_j.  While every intermediate of the unscaled form is a normal float32
// number the power of two changes no rounding (Sigma, its determinant and y scale exactly, and w_i (R~_i y 2^e) = v_i (R~_i y)); where
// the unscaled determinant would be subnormal or underflow (a nearly silent frame, |X| ~ 1e-10: det ~ 1e-43) the two forms differ, and
// the scaled one is the accurate one -- which is why it is used.
#include "spatial.h"
#include "../../include/gccnmf_hip.h"

__global__ __launch_bounds__(256) void gcc_spatial_cov_kernel(const float2* __restrict__ spec, int F, int Fp, int T, int Tp, int S,
                                                              float4* __restrict__ cov) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int i = blockIdx.y, b = blockIdx.z;
    if (f >= F) return;                                        // wave-uniform
    const long plane = (long)Fp * Tp;
    const float2* __restrict__ s0 = spec + ((long)b * 2 * S + 2 * i) * plane + (long)f * Tp;
    const float2* __restrict__ s1 = s0 + plane;
    double p0 = 0.0, p1 = 0.0, qr = 0.0, qi = 0.0;
    for (int t = 2 * lane; t < T; t += 128) {                  // t even and Tp a multiple of 64: t + 1 < Tp, 16-byte aligned
        const float4 a = *(const float4*)(s0 + t);
        const float4 c = *(const float4*)(s1 + t);
        {
            const double ar = a.x, ai = a.y, cr = c.x, ci = c.y;
            p0 += ar * ar + ai * ai;
            p1 += cr * cr + ci * ci;
            qr += ar * cr + ai * ci;
            qi += ai * cr - ar * ci;
        }
        if (t + 1 < T) {
            const double ar = a.z, ai = a.w, cr = c.z, ci = c.w;
            p0 += ar * ar + ai * ai;
            p1 += cr * cr + ci * ci;
            qr += ar * cr + ai * ci;
            qi += ai * cr - ar * ci;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {                         // a + b == b + a: every lane ends with the same four sums
        p0 += __shfl_xor(p0, m);
        p1 += __shfl_xor(p1, m);
        qr += __shfl_xor(qr, m);
        qi += __shfl_xor(qi, m);
    }
    if (lane == 0) {
        const double n = 0.5 * (p0 + p1), lambda = GCCNMF_SPATIAL_LOADING;
        double r00 = 1.0, r11 = 1.0, r01r = 0.0, r01i = 0.0;
        if (!(n == 0.0)) {                                     // NaN / Inf take the quotients and propagate
            r00 = p0 / n;
            r11 = p1 / n;
            r01r = qr / n;
            r01i = qi / n;
        }
        cov[((long)b * S + i) * Fp + f] = make_float4((float)(r00 + lambda), (float)(r11 + lambda), (float)r01r, (float)r01i);
    }
}

// WS: the powers come from the workspace of the EM refinement (spatial_em.hip) instead of the estimates in spec, which is then only written.
template <int S, bool WS>
__global__ __launch_bounds__(256) void gcc_spatial_filter_kernel(const float2* __restrict__ X, const float4* __restrict__ cov,
                                                                 const float* __restrict__ powers, int F, int Fp, int T, int Tp, float2* spec) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // < Fp: Fp is a multiple of 16
    const int b = blockIdx.y;
    const long plane = (long)Fp * Tp;
    float2* O = spec + (long)b * 2 * S * plane + (long)f * Tp;                            // plane i*2+c at O + (i*2+c) * plane
    if (f >= F) {                                                                         // wave-uniform: the padding rows
        for (int t = 2 * lane; t < Tp; t += 128) {
#pragma unroll
            for (int j = 0; j < 2 * S; ++j) *(float4*)(O + j * plane + t) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    const float2* __restrict__ x0 = X + (long)b * 2 * plane + (long)f * Tp;
    const float2* __restrict__ x1 = x0 + plane;
    float4 r[S];
#pragma unroll
    for (int i = 0; i < S; ++i) r[i] = cov[((long)b * S + i) * Fp + f];
    for (int t = 2 * lane; t < Tp; t += 128) {                 // frames t, t + 1 < Tp
        float va[S], vb[S];
        float4 xa, xb;
        if constexpr (WS) {
            const float* __restrict__ P = powers + (long)b * S * plane + (long)f * Tp + t;
#pragma unroll
            for (int i = 0; i < S; ++i) {                      // written for the frames t < T only (t even: the pair of T - 1 too)
                const float2 p = t < T ? *(const float2*)(P + i * plane) : make_float2(0.f, 0.f);
                va[i] = p.x;
                vb[i] = p.y;
            }
            xa = *(const float4*)(x0 + t);
            xb = *(const float4*)(x1 + t);
        } else {
            float4 e0[S], e1[S];
#pragma unroll
            for (int i = 0; i < S; ++i) {
                e0[i] = *(const float4*)(O + (2 * i) * plane + t);
                e1[i] = *(const float4*)(O + (2 * i + 1) * plane + t);
            }
            xa = *(const float4*)(x0 + t);
            xb = *(const float4*)(x1 + t);
#pragma unroll
            for (int i = 0; i < S; ++i) {
                va[i] = spatial_power(e0[i].x, e0[i].y, e1[i].x, e1[i].y);
                vb[i] = spatial_power(e0[i].z, e0[i].w, e1[i].z, e1[i].w);
            }
        }
        float2 a0[S], a1[S], b0[S], b1[S];
        spatial_frame<S>(r, va, xa.x, xa.y, xb.x, xb.y, t < T, a0, a1);
        spatial_frame<S>(r, vb, xa.z, xa.w, xb.z, xb.w, t + 1 < T, b0, b1);
#pragma unroll
        for (int i = 0; i < S; ++i) {
            *(float4*)(O + (2 * i) * plane + t) = make_float4(a0[i].x, a0[i].y, b0[i].x, b0[i].y);
            *(float4*)(O + (2 * i + 1) * plane + t) = make_float4(a1[i].x, a1[i].y, b1[i].x, b1[i].y);
        }
    }
}

template <int S>
static void spatial_filter_launch(const float* X, const float* cov, const float* powers, int F, int Fp, int T, int Tp, int batch, float* spec,
                                  hipStream_t s) {
    if (powers)
        hipLaunchKernelGGL((gcc_spatial_filter_kernel<S, true>), dim3(Fp / 4, batch), dim3(256), 0, s, (const float2*)X, (const float4*)cov,
                           powers, F, Fp, T, Tp, (float2*)spec);
    else
        hipLaunchKernelGGL((gcc_spatial_filter_kernel<S, false>), dim3(Fp / 4, batch), dim3(256), 0, s, (const float2*)X, (const float4*)cov,
                           powers, F, Fp, T, Tp, (float2*)spec);
}

int gccnmf_launch_spatial_cov(int F, int T, int S, int batch, const float* spec, float* cov, hipStream_t s) {
    if (S < 1 || S > GCCNMF_SPATIAL_MAX_TARGETS || batch > 65535) return GCCNMF_ERR_UNSUPPORTED;
    GccNmfPitches p = gccnmf_make_pitches(F, T, 1);
    hipLaunchKernelGGL(gcc_spatial_cov_kernel, dim3(gccnmf_ceil_div(F, 4), S, batch), dim3(256), 0, s, (const float2*)spec, F, p.Fp, T, p.Tp,
                       S, (float4*)cov);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

int gccnmf_launch_spatial_filter(const float* X, const float* cov, const float* powers, int F, int T, int S, int batch, float* spec,
                                 hipStream_t s) {
    if (S < 1 || S > GCCNMF_SPATIAL_MAX_TARGETS || batch > 65535) return GCCNMF_ERR_UNSUPPORTED;
    GccNmfPitches p = gccnmf_make_pitches(F, T, 1);
    switch (S) {
        case 1: spatial_filter_launch<1>(X, cov, powers, F, p.Fp, T, p.Tp, batch, spec, s); break;
        case 2: spatial_filter_launch<2>(X, cov, powers, F, p.Fp, T, p.Tp, batch, spec, s); break;
        case 3: spatial_filter_launch<3>(X, cov, powers, F, p.Fp, T, p.Tp, batch, spec, s); break;
        case 4: spatial_filter_launch<4>(X, cov, powers, F, p.Fp, T, p.Tp, batch, spec, s); break;
        case 5: spatial_filter_launch<5>(X, cov, powers, F, p.Fp, T, p.Tp, batch, spec, s); break;
        case 6: spatial_filter_launch<6>(X, cov, powers, F, p.Fp, T, p.Tp, batch, spec, s); break;
        case 7: spatial_filter_launch<7>(X, cov, powers, F, p.Fp, T, p.Tp, batch, spec, s); break;
        default: spatial_filter_launch<8>(X, cov, powers, F, p.Fp, T, p.Tp, batch, spec, s); break;
    }
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

int gccnmf_launch_spatial(const float* X, int F, int T, int S, int batch, float* cov, float* spec, hipStream_t s) {
    const int rc = gccnmf_launch_spatial_cov(F, T, S, batch, spec, cov, s);
    return rc != GCCNMF_OK ? rc : gccnmf_launch_spatial_filter(X, cov, nullptr, F, T, S, batch, spec, s);
}
