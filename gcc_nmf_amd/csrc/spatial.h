// Spatial (multichannel Wiener) filter behind the ratio-mask reconstruction, two launches (spatial.hip).
#pragma once
#include "common.h"

#define GCCNMF_SPATIAL_MAX_TARGETS 8

// cov [batch][S][Fp][4] float32 = (R~00, R~11, Re R~01, Im R~01) of every (file, target, bin < F); spec [batch][S*2][Fp][Tp] complex is
// read (the ratio-mode estimates) and overwritten in place with the filtered estimates; X [batch][2][Fp][Tp] complex.  Arguments are
// checked by the caller (gccnmf_reconstruct); 1 <= S <= 8, cov 16-byte aligned.
int gccnmf_launch_spatial(const float* X, int F, int T, int S, int batch, float* cov, float* spec, hipStream_t s);

// The 2 x 2 arithmetic of the filter, shared by the offline kernel (spatial.hip) and the real-time one (rt_spatial.hip): both files are
// built with -ffp-contract=off, and every product and sum below is its own float32 rounding in the order written.
// One (bin, frame): the S powers v, the row's R~ (x = R~00, y = R~11, z + j w = R~01) and X -> the S filtered pairs.
template <int S>
__device__ __forceinline__ void spatial_frame(const float4 (&r)[S], const float (&v)[S], float x0r, float x0i, float x1r, float x1i,
                                              bool inside, float2 (&o0)[S], float2 (&o1)[S]) {
#pragma clang fp contract(off)
    float vs = v[0];
#pragma unroll
    for (int j = 1; j < S; ++j) vs = vs + v[j];
    int e;
    (void)frexpf(vs, &e);
    float w[S];
#pragma unroll
    for (int j = 0; j < S; ++j) w[j] = ldexpf(v[j], -e);
    float a = w[0] * r[0].x, d = w[0] * r[0].y, br = w[0] * r[0].z, bi = w[0] * r[0].w;
#pragma unroll
    for (int j = 1; j < S; ++j) {
        a = a + w[j] * r[j].x;
        d = d + w[j] * r[j].y;
        br = br + w[j] * r[j].z;
        bi = bi + w[j] * r[j].w;
    }
    const float det = a * d - (br * br + bi * bi);
    const float rdet = 1.0f / det;
    const float y0r = (d * x0r - (br * x1r - bi * x1i)) * rdet;
    const float y0i = (d * x0i - (br * x1i + bi * x1r)) * rdet;
    const float y1r = (a * x1r - (br * x0r + bi * x0i)) * rdet;
    const float y1i = (a * x1i - (br * x0i - bi * x0r)) * rdet;
    const bool live = inside && !(vs == 0.f);                  // false for NaN: those propagate
#pragma unroll
    for (int i = 0; i < S; ++i) {
        o0[i] = make_float2(0.f, 0.f);
        o1[i] = make_float2(0.f, 0.f);
        if (live) {
            o0[i].x = w[i] * (r[i].x * y0r + (r[i].z * y1r - r[i].w * y1i));
            o0[i].y = w[i] * (r[i].x * y0i + (r[i].z * y1i + r[i].w * y1r));
            o1[i].x = w[i] * ((r[i].z * y0r + r[i].w * y0i) + r[i].y * y1r);
            o1[i].y = w[i] * ((r[i].z * y0i - r[i].w * y0r) + r[i].y * y1i);
        }
    }
}

__device__ __forceinline__ float spatial_power(float ar, float ai, float cr, float ci) {
#pragma clang fp contract(off)
    return 0.5f * ((ar * ar + ai * ai) + (cr * cr + ci * ci));
}
