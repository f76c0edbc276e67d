// GCC-NONLIN angular spectrogram  A[tau,t] = sum_f phi(Re(C[f,t] e^{-j 2 pi f tau}))  (angular_nl.h; gccPHATNLEnabled / gccPHATNLAlpha of
// gccNMF/realtime/config.py:42-43, which the reference declares and never evaluates).
//
// The nonlinearity sits inside the sum over frequency, so this is not a GEMM: batch * D * T * F evaluations of sqrt, exp and a
// reciprocal on the VALU / transcendental pipe.  Register tiling: a lane owns TD x TT (tau x t) accumulators and per frequency row loads
// TD cos, TD sin, TT Re C and TT Im C (one vector load each), i.e. 4 loads for TD * TT evaluations of ~8 instructions.  A wave is 4 tau
// groups x 16 t groups (the t groups read 16 * TT consecutive frames: coalesced; the tau groups share them).
//
// Summation order.  The four waves of a workgroup split the frequency rows into four fixed chunks of ceil(F / 4), each walked in
// ascending order; the partial sums meet in LDS and are added as ((w0 + w1) + w2) + w3.  That order depends on F alone -- not on the
// batch, the grid or the block a lane owns -- and fp contraction is off in this file (the steering product is written as the explicit
// fma it is), so a file alone and the same file in a batch agree bit for bit although they take different blocks.
#include "angular_nl.h"

#define NL_WAVES 4

template <int TD, int TT>
struct NlRow {
    float c[TD], s[TD], cr[TT], ci[TT];
};

template <int N>
__device__ __forceinline__ void nl_load(const float* __restrict__ p, float (&v)[N]) {
    static_assert(N == 2 || N == 4, "vector width");
    if constexpr (N == 4) {
        const float4 q = *(const float4*)p;
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        const float2 q = *(const float2*)p;
        v[0] = q.x; v[1] = q.y;
    }
}

// grid = (Tp / (16 * TT), Dp / (4 * TD), batch), 256 threads.  Tp and Dp are multiples of 64, so every load stays inside the padded
// images (zero there: phi of 0, never stored).
template <int TD, int TT>
__global__ __launch_bounds__(64 * NL_WAVES) void angular_nl_kernel(const float* __restrict__ CC, const float* __restrict__ trig, int F,
                                                                    int Fp, int T, int Tp, int D, int Dp, float k2,
                                                                    float* __restrict__ ang) {
#pragma clang fp contract(off)
    __shared__ float s_part[NL_WAVES - 1][TD * TT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t0 = (blockIdx.x * 16 + (lane & 15)) * TT, d0 = (blockIdx.y * 4 + (lane >> 4)) * TD;
    const long plane = (long)Fp * Tp;
    const float* Cr = CC + (long)blockIdx.z * 2 * plane + t0;
    const float* Ci = Cr + plane;
    const float* cosT = trig + d0;
    const float* sinT = cosT + (long)Fp * Dp;
    const int per = (F + NL_WAVES - 1) / NL_WAVES;
    const int f_lo = wave * per, f_hi = min(F, f_lo + per);
    float acc[TD][TT];
#pragma unroll
    for (int i = 0; i < TD; ++i)
#pragma unroll
        for (int j = 0; j < TT; ++j) acc[i][j] = 0.f;
    auto load = [&](int f, NlRow<TD, TT>& r) {
        nl_load<TD>(cosT + (long)f * Dp, r.c);
        nl_load<TD>(sinT + (long)f * Dp, r.s);
        nl_load<TT>(Cr + (long)f * Tp, r.cr);
        nl_load<TT>(Ci + (long)f * Tp, r.ci);
    };
    NlRow<TD, TT> cur, nxt;
    if (f_lo < f_hi) load(f_lo, cur);
    for (int f = f_lo; f < f_hi; ++f) {
        load(min(f + 1, f_hi - 1), nxt);                  // the next row's operands are in flight while this one is evaluated
#pragma unroll
        for (int i = 0; i < TD; ++i)
#pragma unroll
            for (int j = 0; j < TT; ++j) {
                const float re = __builtin_fmaf(cur.ci[j], cur.s[i], cur.cr[j] * cur.c[i]);
                acc[i][j] += gccnmf_nl_half_phi(re, k2);
            }
        cur = nxt;
    }
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < TD; ++i)
#pragma unroll
            for (int j = 0; j < TT; ++j) s_part[wave - 1][i * TT + j][lane] = acc[i][j];
    }
    __syncthreads();
    if (wave != 0) return;
    float* out = ang + ((long)blockIdx.z * Dp + d0) * Tp + t0;
#pragma unroll
    for (int i = 0; i < TD; ++i)
#pragma unroll
        for (int j = 0; j < TT; ++j) {
            float v = acc[i][j];                          // fixed order: ((w0 + w1) + w2) + w3, then the factor 2 of phi (exact)
#pragma unroll
            for (int w = 0; w < NL_WAVES - 1; ++w) v += s_part[w][i * TT + j][lane];
            if (d0 + i < D && t0 + j < T) out[(long)i * Tp + j] = 2.f * v;
        }
}

int gccnmf_launch_angular_nl(const float* CC, const float* trig, int F, int T, int D, int batch, float alpha, float* ang, hipStream_t s) {
    GccNmfPitches p = gccnmf_make_pitches(F, T, 1);
    const int Dp = gccnmf_round_up(D, 64);
    const float k2 = gccnmf_nl_k2(alpha);
    // 4 x 4 accumulators per lane where that gives every SIMD of the chip (1024) a wave; below that 2 x 2, four times the waves: one
    // file of 128 x 622 outputs is 320 waves in the first form and 1280 in the second
    const long waves44 = (long)batch * (p.Tp / 64) * (Dp / 16) * NL_WAVES;
    if (waves44 >= 1024)
        hipLaunchKernelGGL((angular_nl_kernel<4, 4>), dim3(p.Tp / 64, Dp / 16, batch), dim3(64 * NL_WAVES), 0, s, CC, trig, F, p.Fp, T, p.Tp,
                           D, Dp, k2, ang);
    else
        hipLaunchKernelGGL((angular_nl_kernel<2, 2>), dim3(p.Tp / 32, Dp / 8, batch), dim3(64 * NL_WAVES), 0, s, CC, trig, F, p.Fp, T, p.Tp,
                           D, Dp, k2, ang);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}
