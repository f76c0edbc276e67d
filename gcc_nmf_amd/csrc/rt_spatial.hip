// Online spatial (multichannel Wiener) filter of the real-time block call: the streaming form of spatial.hip, run between the mask
// kernel (rt_tfmask / rt_tfmask_h of rt.hip) and the synthesis kernel when the call asks for it (GCCNMF_RT_SEPARATION_SPATIAL).  The local
// Gaussian model is the offline one; the covariance of a component is a trace-normalised exponential average carried across blocks as
// per-stream state, because a stream has no "every frame of the file".  Per stream and bin f, components j < NC, frames in ascending order:
//
//   E_j,c      multi-target layout: the masked spectrum Y_j,c as the mask kernel wrote it (NC = N)
//              single-target layouts: E_0 = Y (the talker), E_1 = X - E_0 (the residual), component-wise (NC = 2)
//   c_j        = (|E_j,0|^2, |E_j,1|^2, Re E_j,0 conj E_j,1, Im E_j,0 conj E_j,1),   v_j = 1/2 (c_j.p0 + c_j.p1)
//   P_j       <- a P_j + b c_j,  b = 1 / tau, a = 1 - b, BEFORE use -- only when X and every c_j of this (bin, frame) are finite; else the
//              state of the bin stays as it is, bit for bit (a NaN block cannot poison a stream)
//   R_j        = P_j / n_j, n_j = 1/2 (P_j.p0 + P_j.p1);  R_j = I when n_j < 2^-126;  R~_j = R_j + GCCNMF_SPATIAL_LOADING I
//   Y'_j       = v_j R~_j (sum_i v_i R~_i)^-1 X: spatial_frame of spatial.h, the arithmetic of the offline filter statement for statement
//              (0 where sum_j v_j = 0; NaN / Inf propagate for that frame only)
//   written    multi-target: Y_j <- Y'_j for every j;  single-target: Y <- Y'_0.  In place: the synthesis kernels read Y as before.
//
// One thread per (stream, bin), grid = (ceil(F / 64), 1, S): the recursion is serial in t and independent across bins, and a block has few
// frames (Tc = 1 in the low-latency configuration), so there is nothing to reduce across lanes.  The 4 NC state words stay in registers
// over the frame loop; they are read once and written once per call as float4.  Every load of a frame comes in front of its first
// store (the outputs need every v_j).  Stream s is blockIdx.z and the base pointers move to its images, as in rt.hip.
//
// Built with -ffp-contract=off; every product and sum is its own float32 rounding in the order written; 1 / tau and 1 / n_j are one IEEE
// division each, followed by products.
#include "rt_spatial.h"
#include "spatial.h"
#include "../../include/gccnmf_hip.h"

__device__ __forceinline__ bool rt_spatial_finite(float a, float b, float c, float d) {
    return fabsf(a) < INFINITY && fabsf(b) < INFINITY && fabsf(c) < INFINITY && fabsf(d) < INFINITY;
}

// NC components; RESID: the single-target layouts (NC = 2: Y and the residual X - Y; only Y is written)
template <int NC, bool RESID>
__global__ __launch_bounds__(64) void rt_spatial_kernel(const float2* __restrict__ X, float2* Y, const float* __restrict__ rows,
                                                        int row_len, int bank, float4* state, int F, int Tc) {
#pragma clang fp contract(off)
    const long sid = blockIdx.z;
    rows += sid * row_len;
    const float tau = rows[7];
    if (!(tau >= 1.f && tau < INFINITY)) return;              // word 7: a finite float >= 1 switches the stream's filter on (NaN: off)
    if (bank && rows[4] == 0.f) return;                       // this stream's separation is off: no masked spectra, state left alone
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    const long plane = (long)F * Tc;                          // one channel of one spectrum
    constexpr int NY = RESID ? 1 : NC;                        // spectra in the stream's Y image
    X += sid * 2 * plane;
    Y += sid * NY * 2 * plane;
    state += sid * NC * F;
    const float b = 1.f / tau, a = 1.f - b;
    const float lambda = (float)GCCNMF_SPATIAL_LOADING;
    float4 P[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) P[j] = state[(long)j * F + f];
    for (int t = 0; t < Tc; ++t) {
        const long at0 = (long)f * Tc + t, at1 = at0 + plane;
        const float2 x0 = X[at0], x1 = X[at1];
        float2 e0[NC], e1[NC];
#pragma unroll
        for (int j = 0; j < NY; ++j) {
            e0[j] = Y[2 * j * plane + at0];
            e1[j] = Y[2 * j * plane + at1];
        }
        if constexpr (RESID) {
            e0[1] = make_float2(x0.x - e0[0].x, x0.y - e0[0].y);
            e1[1] = make_float2(x1.x - e1[0].x, x1.y - e1[0].y);
        }
        float4 c[NC];
        float v[NC];
        bool fin = rt_spatial_finite(x0.x, x0.y, x1.x, x1.y);
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const float ar = e0[j].x, ai = e0[j].y, cr = e1[j].x, ci = e1[j].y;
            c[j] = make_float4(ar * ar + ai * ai, cr * cr + ci * ci, ar * cr + ai * ci, ai * cr - ar * ci);
            v[j] = spatial_power(ar, ai, cr, ci);
            fin = fin && rt_spatial_finite(c[j].x, c[j].y, c[j].z, c[j].w);
        }
        float4 r[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            if (fin) P[j] = make_float4(a * P[j].x + b * c[j].x, a * P[j].y + b * c[j].y, a * P[j].z + b * c[j].z, a * P[j].w + b * c[j].w);
            const float n = 0.5f * (P[j].x + P[j].y);
            if (n < 1.17549435e-38f) {                        // nothing averaged yet (or subnormal): R = I.  NaN takes the quotient
                r[j] = make_float4(1.f + lambda, 1.f + lambda, 0.f, 0.f);
            } else {
                const float rn = 1.f / n;
                r[j] = make_float4(P[j].x * rn + lambda, P[j].y * rn + lambda, P[j].z * rn, P[j].w * rn);
            }
        }
        float2 o0[NC], o1[NC];
        spatial_frame<NC>(r, v, x0.x, x0.y, x1.x, x1.y, true, o0, o1);
#pragma unroll
        for (int j = 0; j < NY; ++j) {
            Y[2 * j * plane + at0] = o0[j];
            Y[2 * j * plane + at1] = o1[j];
        }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) state[(long)j * F + f] = P[j];
}

template <int NC, bool RESID>
static void rt_spatial_launch(const float* X, float* Y, const float* rows, int row_len, int bank, float* state, int F, int Tc, int S,
                              hipStream_t s) {
    hipLaunchKernelGGL((rt_spatial_kernel<NC, RESID>), dim3(gccnmf_ceil_div(F, 64), 1, S), dim3(64), 0, s, (const float2*)X, (float2*)Y, rows,
                       row_len, bank, (float4*)state, F, Tc);
}

int gccnmf_launch_rt_spatial(const float* X, float* Y, const float* rows, int row_len, int bank, float* state, int F, int Tc, bool multi,
                             int NT, int S, hipStream_t s) {
    if (!multi) {
        rt_spatial_launch<2, true>(X, Y, rows, row_len, bank, state, F, Tc, S, s);
    } else {
        switch (NT) {
            case 1: rt_spatial_launch<1, false>(X, Y, rows, row_len, bank, state, F, Tc, S, s); break;
            case 2: rt_spatial_launch<2, false>(X, Y, rows, row_len, bank, state, F, Tc, S, s); break;
            case 3: rt_spatial_launch<3, false>(X, Y, rows, row_len, bank, state, F, Tc, S, s); break;
            case 4: rt_spatial_launch<4, false>(X, Y, rows, row_len, bank, state, F, Tc, S, s); break;
            case 5: rt_spatial_launch<5, false>(X, Y, rows, row_len, bank, state, F, Tc, S, s); break;
            case 6: rt_spatial_launch<6, false>(X, Y, rows, row_len, bank, state, F, Tc, S, s); break;
            case 7: rt_spatial_launch<7, false>(X, Y, rows, row_len, bank, state, F, Tc, S, s); break;
            default: rt_spatial_launch<8, false>(X, Y, rows, row_len, bank, state, F, Tc, S, s); break;
        }
    }
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}
