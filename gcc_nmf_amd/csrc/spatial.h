// Spatial (multichannel Wiener) filter behind the ratio-mask reconstruction, two launches (spatial.hip).
#pragma once
#include "common.h"

#define GCCNMF_SPATIAL_MAX_TARGETS 8

// cov [batch][S][Fp][4] float32 = (R~00, R~11, Re R~01, Im R~01) of every (file, target, bin < F); spec [batch][S*2][Fp][Tp] complex is
// read (the ratio-mode estimates) and overwritten in place with the filtered estimates; X [batch][2][Fp][Tp] complex.  Arguments are
// checked by the caller (gccnmf_reconstruct); 1 <= S <= 8, cov 16-byte aligned.
int gccnmf_launch_spatial(const float* X, int F, int T, int S, int batch, float* cov, float* spec, hipStream_t s);

// The two launches on their own, for the EM refinement between them (spatial_em.hip).  powers == NULL: the filter takes v_i from the
// estimates in spec (the call above); else from powers [batch][S][Fp][Tp] float32 (frames < T), and spec is only written.
int gccnmf_launch_spatial_cov(int F, int T, int S, int batch, const float* spec, float* cov, hipStream_t s);
int gccnmf_launch_spatial_filter(const float* X, const float* cov, const float* powers, int F, int T, int S, int batch, float* spec,
                                 hipStream_t s);

// n >= 1 EM iterations between the two (spatial_em.hip, one launch): cov in / out, powers [batch][S][Fp][Tp] out (16-byte aligned).
int gccnmf_launch_spatial_em(const float* X, int F, int T, int S, int batch, int n, float* cov, float* powers, float* spec, hipStream_t s);

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

// The front half of spatial_frame with its intermediates kept, for the EM refinement (spatial_em.hip): Sigma_w = sum_j w_j R~_j on
// w_j = v_j 2^-e (e the binary exponent of sum_j v_j) and y = Sigma_w^-1 X, the same roundings in the same order.  spatial_frame is not
// rewritten on top of it: its text, and with it the device code of the filter kernels that use it, stays what it was.
template <int S>
struct SpatialSolve {
    float w[S];
    float vs, a, d, br, bi, rdet, y0r, y0i, y1r, y1i;
    int e;
};

template <int S>
__device__ __forceinline__ void spatial_solve(const float4 (&r)[S], const float (&v)[S], float x0r, float x0i, float x1r, float x1i,
                                              SpatialSolve<S>& g) {
#pragma clang fp contract(off)
    float vs = v[0];
#pragma unroll
    for (int j = 1; j < S; ++j) vs = vs + v[j];
    int e;
    (void)frexpf(vs, &e);
#pragma unroll
    for (int j = 0; j < S; ++j) g.w[j] = ldexpf(v[j], -e);
    float a = g.w[0] * r[0].x, d = g.w[0] * r[0].y, br = g.w[0] * r[0].z, bi = g.w[0] * r[0].w;
#pragma unroll
    for (int j = 1; j < S; ++j) {
        a = a + g.w[j] * r[j].x;
        d = d + g.w[j] * r[j].y;
        br = br + g.w[j] * r[j].z;
        bi = bi + g.w[j] * r[j].w;
    }
    const float det = a * d - (br * br + bi * bi);
    const float rdet = 1.0f / det;
    g.y0r = (d * x0r - (br * x1r - bi * x1i)) * rdet;
    g.y0i = (d * x0i - (br * x1i + bi * x1r)) * rdet;
    g.y1r = (a * x1r - (br * x0r + bi * x0i)) * rdet;
    g.y1i = (a * x1i - (br * x0i - bi * x0r)) * rdet;
    g.vs = vs; g.e = e; g.a = a; g.d = d; g.br = br; g.bi = bi; g.rdet = rdet;
}

// u = R~ y, in the association of the filter's output
__device__ __forceinline__ void spatial_apply(const float4 r, float y0r, float y0i, float y1r, float y1i, float& u0r, float& u0i,
                                              float& u1r, float& u1i) {
#pragma clang fp contract(off)
    u0r = r.x * y0r + (r.z * y1r - r.w * y1i);
    u0i = r.x * y0i + (r.z * y1i + r.w * y1r);
    u1r = (r.z * y0r + r.w * y0i) + r.y * y1r;
    u1i = (r.z * y0i - r.w * y0r) + r.y * y1i;
}

// One (bin, frame) of one EM iteration of the local Gaussian model (spatial_em.hip; include/gccnmf_hip.h states the recursion) against
// the row's current R~: the S new powers vn (unscaled; 0 for every target where sum_j v_j = 0) and, for every target whose vn is not 0,
// the frame's term C_i / v'_i of the new covariance as (00, 11, Re 01, Im 01).  With u_i = R~_i y and N_i = sum_{j != i} w_j R~_j:
//   k_i = tr(Sigma_w^-1 N_i) = 2 - tr G_i,  P_i = N_i Sigma_w^-1 R~_i = (I - G_i) R~_i,
//   v"_i = 1/2 (w_i Re(y^H u_i) + 2^e k_i),  vn_i = max(0, w_i v"_i),  C"_i = w_i u_i u_i^H + 2^e P_i,  term_i = C"_i / v"_i
// (C_i = w_i C"_i and v'_i = w_i v"_i: both of the magnitude of |X|^2 whatever the target's share, sums of non-negative parts).
template <int S>
__device__ __forceinline__ void spatial_em_frame(const float4 (&r)[S], const float (&v)[S], float x0r, float x0i, float x1r, float x1i,
                                                 float (&vn)[S], float4 (&term)[S]) {
#pragma clang fp contract(off)
    SpatialSolve<S> g;
    spatial_solve<S>(r, v, x0r, x0i, x1r, x1i, g);
    const float a = g.a, d = g.d, br = g.br, bi = g.bi, rdet = g.rdet;
    const bool dead = g.vs == 0.f;                             // false for NaN
#pragma unroll
    for (int i = 0; i < S; ++i) {
        float u0r, u0i, u1r, u1i;
        spatial_apply(r[i], g.y0r, g.y0i, g.y1r, g.y1i, u0r, u0i, u1r, u1i);
        float n0 = 0.f, n1 = 0.f, nr = 0.f, ni = 0.f;
        bool first = true;
#pragma unroll
        for (int j = 0; j < S; ++j) {
            if (j == i) continue;
            if (first) {
                n0 = g.w[j] * r[j].x; n1 = g.w[j] * r[j].y; nr = g.w[j] * r[j].z; ni = g.w[j] * r[j].w;
                first = false;
            } else {
                n0 = n0 + g.w[j] * r[j].x; n1 = n1 + g.w[j] * r[j].y; nr = nr + g.w[j] * r[j].z; ni = ni + g.w[j] * r[j].w;
            }
        }
        const float k = ((d * n0 + a * n1) - 2.0f * (br * nr + bi * ni)) * rdet;
        const float h = (g.y0r * u0r + g.y0i * u0i) + (g.y1r * u1r + g.y1i * u1i);
        const float v2 = 0.5f * (g.w[i] * h + ldexpf(k, g.e));
        float vi = g.w[i] * v2;
        vi = vi < 0.f ? 0.f : vi;                              // NaN stays
        vn[i] = dead ? 0.f : vi;
        const float kk = br * r[i].z + bi * r[i].w, ll = bi * r[i].z - br * r[i].w;
        const float m00r = d * r[i].x - kk;
        const float m11r = a * r[i].y - kk, m11i = ll;
        const float m01r = d * r[i].z - br * r[i].y, m01i = d * r[i].w - bi * r[i].y;
        const float m10r = a * r[i].z - br * r[i].x, m10i = bi * r[i].x - a * r[i].w;
        const float p00 = (n0 * m00r + (nr * m10r - ni * m10i)) * rdet;
        const float p11 = ((nr * m01r + ni * m01i) + n1 * m11r) * rdet;
        const float p01r = (n0 * m01r + (nr * m11r - ni * m11i)) * rdet;
        const float p01i = (n0 * m01i + (nr * m11i + ni * m11r)) * rdet;
        const float rv = 1.0f / v2;
        term[i].x = (g.w[i] * (u0r * u0r + u0i * u0i) + ldexpf(p00, g.e)) * rv;
        term[i].y = (g.w[i] * (u1r * u1r + u1i * u1i) + ldexpf(p11, g.e)) * rv;
        term[i].z = (g.w[i] * (u0r * u1r + u0i * u1i) + ldexpf(p01r, g.e)) * rv;
        term[i].w = (g.w[i] * (u0i * u1r - u0r * u1i) + ldexpf(p01i, g.e)) * rv;
    }
}

__device__ __forceinline__ float spatial_power(float ar, float ai, float cr, float ci) {
#pragma clang fp contract(off)
    return 0.5f * ((ar * ar + ai * ai) + (cr * cr + ci * ci));
}
