// GCC-NONLIN localisation (Blandin, Ozerov & Vincent 2012): the nonlinearity of the angular spectrum, shared by the offline kernel
// (angular_nl.hip) and the streaming localisation (rt.hip), so that both evaluate the same instructions.
#pragma once
#include "common.h"

// phi(re) = 1 - tanh(alpha * sqrt(max(0, 1 - re))) = 2 / (1 + e^{2 alpha sqrt(.)}), k2 = 2 alpha log2(e) so that the exponential is
// ONE v_exp_f32.  Three transcendental issues per evaluation (v_sqrt_f32, v_exp_f32, v_rcp_f32, each within 1 ulp) and seven plain
// VALU instructions with the steering product.  e^{..} = inf (alpha beyond ~30) gives rcp(inf) = 0, the limit; re > 1 by a rounding
// error gives sqrt(0) and phi = 1.  The factor 2 is applied by the caller to the finished sum (exact).
__device__ __forceinline__ float gccnmf_nl_half_phi(float re, float k2) {
    const float y = __builtin_amdgcn_sqrtf(fmaxf(0.f, 1.f - re));
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(k2 * y));
}

// k2 of the function above: the product in double, rounded to float32 once (host launcher and streaming kernel alike)
__host__ __device__ static inline float gccnmf_nl_k2(float alpha) { return (float)(2.0 * (double)alpha * 1.4426950408889634); }

// alpha > 0, finite and a normal float32 (the packed form of gccnmf_angular_spectrogram reads an all-zero upper half as "PHAT")
__host__ __device__ static inline bool gccnmf_nl_alpha_ok(float alpha) { return alpha >= 1.17549435e-38f && alpha <= 3.40282347e+38f; }

// ang[b][tau][t] = sum_f phi(Cr cos + Ci sin), the buffers, pitches and padding rules of gccnmf_angular_spectrogram (only tau < D,
// t < T is written).  Arguments are checked by the caller.
int gccnmf_launch_angular_nl(const float* CC, const float* trig, int F, int T, int D, int batch, float alpha, float* ang, hipStream_t s);
