// Ratio-mask (Wiener-like) reconstruction: S[i,c] = X_c * (W . (H_c o M_i)) / den, every target of a (bin, frame) in ONE launch, for the
// M channels of a recording.  The one kernel of both callers: ratio.hip (the separation library, M = 2) and array.hip (the microphone-array
// library, 2 <= M <= 8); each library compiles its own instantiations.
// The direct reconstruction (gcc.hip: gcc_masked_h_kernel + a GEMM with the phase epilogue) writes 2 S masked copies of H so that a plain
// GEMM can read them back; here H_c is fetched once per tile and the mask is applied to the B fragment in registers.
//
//   num_i[f,t] = sum_k W[f,k] H_c[k,t] M_i[k,t]      exact-f32 fma chain in k order (v_mfma_f32_32x32x2_f32)
//   den[f,t]   = num_0 + num_1 + ... (ascending i)   one-hot form: M_i = [argmax == i]; a masked-out term is fma(w, 0, acc) = acc
//              = sum_k W[f,k] H_c[k,t]               soft form: arbitrary float masks, one more accumulator tile
//   S[i,c]     = X_c * (num_i / den)                 IEEE quotient, then one real x complex product; 0 for every i where den <= 0
//
// A 256-thread workgroup owns 128 bins x 64 frames of one (file, channel); each of its 2 x 2 waves owns 64 x 32 = two 32 x 32 MFMA tiles
// per target (32 S accumulator registers, + 32 for den in the soft form).  The tile shape is the same for every (F, K, S, M, batch), so a
// file's output does not depend on the batch it is in.  Per 16-deep k chunk the W tile, the H_c tile and the arg-max bytes (soft form:
// the S products h * m_i, and h) are staged once, global -> registers -> LDS, with the next chunk's loads in flight under the MFMAs; the A
// fragments are read once per k pair and reused by all S targets.
//
// F = n_fft/2 + 1 is one row more than a multiple of 32: as in gemm_mfma.h that last (Nyquist) row stays off the matrix cores -- the
// workgroups of bin tile 0 carry it on the VALU as the same k-ordered fmaf chains, from the H tile that is in LDS anyway.
//
// Only the (file, channel) of a workgroup, the column offset c T of H_c and the slot i M + c of an output plane know about M.
// Every element of spec[b][i*M+c][0..Fp)[0..Tp), i < S, is written: rows >= F and frames >= T as zeros.
#pragma once
#include "common.h"

typedef float ratio_f32x16 __attribute__((ext_vector_type(16)));

#define RATIO_BM 128
#define RATIO_BN 64
#define RATIO_BK 16
#define RATIO_LDW 17      // W tile row pitch in LDS: the 32 rows of an A-fragment read fall in 32 different banks

struct RatioArgs {
    const float* W;               // [batch][Fp][Kp]
    const float* H;               // [batch][Kp][Np], channel c at columns c*T ..
    const unsigned char* argmax;  // [batch][Kp][Tp]
    const float* masks;           // [batch][S][Kp][Tp]
    const float2* X;              // [batch][M][Fp][Tp]
    float2* spec;                 // [batch][nsig_pitch][Fp][Tp], slot i*M + c
    int M, nsig_pitch;
    int F, Fp, T, Tp, Np, K, Kp;
    int mrows;                    // rows the MFMA tiles own: Fp, or F - 1 when the last row is the VALU tail (ratio_launch fills it)
    int tail;                     // (ratio_launch fills it)
};

template <int S, bool SOFT>
__global__ __launch_bounds__(256) void ratio_kernel(const RatioArgs p) {
    constexpr int NB = SOFT ? S + 1 : 1;              // B tiles in LDS: h (one-hot) | h * m_0 .. h * m_{S-1}, h (soft)
    __shared__ float sW[RATIO_BM * RATIO_LDW];
    __shared__ float sB[NB][RATIO_BK * RATIO_BN];
    __shared__ unsigned char sAm[RATIO_BK * RATIO_BN];
    __shared__ float sWt[RATIO_BK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const int t0 = blockIdx.x * RATIO_BN, row0 = blockIdx.y * RATIO_BM;
    const int b = blockIdx.z / p.M, c = blockIdx.z - b * p.M;
    const bool do_tail = p.tail && blockIdx.y == 0;   // workgroup-uniform

    const float* __restrict__ W = p.W + (long)b * p.Fp * p.Kp;
    const float* __restrict__ H = p.H + (long)b * p.Kp * p.Np + (long)c * p.T;
    const unsigned char* __restrict__ AM = SOFT ? nullptr : p.argmax + (long)b * p.Kp * p.Tp;
    const float* __restrict__ MK = SOFT ? p.masks + (long)b * S * p.Kp * p.Tp : nullptr;

    // staging maps: W tile = 128 rows x 4 float4 (two per thread); H / arg-max / mask tiles = 16 atoms x 16 groups of 4 frames (one per thread)
    int w_off[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int u = tid + 256 * j;
        w_off[j] = min(row0 + (u >> 2), p.Fp - 1) * p.Kp + 4 * (u & 3);
    }
    const int hk = tid >> 4, ht = 4 * (tid & 15);
    const int tg = t0 + ht;                                    // first of this thread's four frames (< Tp)

    float4 rw[2], rwt = make_float4(0.f, 0.f, 0.f, 0.f);
    float rh[4];
    uchar4 ram = make_uchar4(0, 0, 0, 0);
    float4 rm[SOFT ? S : 1];
    bool rk = false;                                           // this thread's atom of the chunk in flight is < K

    auto load_chunk = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) rw[j] = *(const float4*)(W + w_off[j] + k0);
        if (do_tail && tid < 4) rwt = *(const float4*)(W + (long)(p.F - 1) * p.Kp + k0 + 4 * tid);
        const int k = k0 + hk;                                 // < Kp: the loop runs to round_up(K, 16) <= Kp
        const float* h = H + (long)k * p.Np;
        rk = k < p.K;
        // H_c starts at column c*T, which is only 4-byte aligned: scalar loads; atoms >= K and frames >= T enter as zeros
#pragma unroll
        for (int j = 0; j < 4; ++j) rh[j] = (rk && tg + j < p.T) ? h[tg + j] : 0.f;
        if (SOFT) {
#pragma unroll
            for (int i = 0; i < S; ++i) rm[i] = *(const float4*)(MK + ((long)i * p.Kp + k) * p.Tp + tg);
        } else {
            ram = *(const uchar4*)(AM + (long)k * p.Tp + tg);
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int u = tid + 256 * j;
            float* d = sW + (u >> 2) * RATIO_LDW + 4 * (u & 3);
            d[0] = rw[j].x;
            d[1] = rw[j].y;
            d[2] = rw[j].z;
            d[3] = rw[j].w;
        }
        if (do_tail && tid < 4) *(float4*)(sWt + 4 * tid) = rwt;
        const int o = hk * RATIO_BN + ht;
        if (SOFT) {
            // atoms >= K, frames >= T: h is 0 there, but a mask buffer's padding is the caller's -- keep 0 * m out of the products
#pragma unroll
            for (int i = 0; i < S; ++i)
                *(float4*)(&sB[i][o]) = make_float4(rk && tg < p.T ? rh[0] * rm[i].x : 0.f, rk && tg + 1 < p.T ? rh[1] * rm[i].y : 0.f,
                                                    rk && tg + 2 < p.T ? rh[2] * rm[i].z : 0.f, rk && tg + 3 < p.T ? rh[3] * rm[i].w : 0.f);
            *(float4*)(&sB[S][o]) = make_float4(rh[0], rh[1], rh[2], rh[3]);
        } else {
            *(float4*)(&sB[0][o]) = make_float4(rh[0], rh[1], rh[2], rh[3]);
            *(uchar4*)(sAm + o) = ram;
        }
    };

    ratio_f32x16 acc[S][2], accd[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma unroll
            for (int i = 0; i < S; ++i) acc[i][m][r] = 0.f;
            accd[m][r] = 0.f;
        }
    }
    // the VALU tail row: thread (column tid & 63, group tid >> 6) carries targets g and g + 4 (and, soft form, its own copy of den)
    const int tcol = tid & 63, g = wave;
    float tacc0 = 0.f, tacc1 = 0.f, tden = 0.f;

    const int Kr = (p.K + RATIO_BK - 1) / RATIO_BK * RATIO_BK;
    const int arow = wm * 64 + l31, bcol = wn * 32 + l31;
    load_chunk(0);
    for (int k0 = 0; k0 < Kr; k0 += RATIO_BK) {
        __syncthreads();                                       // the previous chunk's fragment reads are done
        store_chunk();
        __syncthreads();
        if (k0 + RATIO_BK < Kr) load_chunk(k0 + RATIO_BK);
#pragma unroll
        for (int kk = 0; kk < RATIO_BK; kk += 2) {
            // lane (l31, hh) supplies A[i = l31][k = hh] and B[k = hh][j = l31]
            float a[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) a[m] = sW[(arow + 32 * m) * RATIO_LDW + kk + hh];
            const int bo = (kk + hh) * RATIO_BN + bcol;
            if (SOFT) {
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    const float bi = sB[i][bo];
#pragma unroll
                    for (int m = 0; m < 2; ++m) acc[i][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bi, acc[i][m], 0, 0, 0);
                }
                const float bd = sB[S][bo];
#pragma unroll
                for (int m = 0; m < 2; ++m) accd[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bd, accd[m], 0, 0, 0);
            } else {
                const float h = sB[0][bo];
                const int am = sAm[bo];
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    const float bi = (am == i) ? h : 0.f;
#pragma unroll
                    for (int m = 0; m < 2; ++m) acc[i][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bi, acc[i][m], 0, 0, 0);
                }
            }
        }
        if (do_tail) {
#pragma unroll
            for (int kk = 0; kk < RATIO_BK; ++kk) {
                const float w = sWt[kk];
                const int bo = kk * RATIO_BN + tcol;
                if (SOFT) {
                    if (g < S) tacc0 = fmaf(w, sB[g < S ? g : 0][bo], tacc0);
                    if (g + 4 < S) tacc1 = fmaf(w, sB[g + 4 < S ? g + 4 : 0][bo], tacc1);
                    tden = fmaf(w, sB[S][bo], tden);
                } else {
                    const float h = sB[0][bo];
                    const int am = sAm[bo];
                    tacc0 = fmaf(w, am == g ? h : 0.f, tacc0);
                    tacc1 = fmaf(w, am == g + 4 ? h : 0.f, tacc1);
                }
            }
        }
    }

    // ---- epilogue: den, quotient, x X_c; per target one 256-byte run per row and lane half -------------------------------------------
    const long plane = (long)p.Fp * p.Tp;
    const float2* __restrict__ X = p.X + ((long)b * p.M + c) * plane;
    float2* __restrict__ O = p.spec + ((long)b * p.nsig_pitch + c) * plane;      // target i at O + i * M * plane
    const long planeM = (long)p.M * plane;
    {
        const int t = t0 + bcol;                               // < Tp
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int rb = row0 + wm * 64 + 32 * m + 4 * hh;
            float2 x[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) x[r] = X[(long)min(rb + (r & 3) + 8 * (r >> 2), p.Fp - 1) * p.Tp + t];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rb + (r & 3) + 8 * (r >> 2);
                float den;
                if (SOFT) {
                    den = accd[m][r];
                } else {
                    den = acc[0][m][r];
#pragma unroll
                    for (int i = 1; i < S; ++i) den += acc[i][m][r];
                }
                // (den <= 0 is false for NaN: a NaN coefficient propagates; padding stays zero whatever the operands hold)
                const bool live = !(den <= 0.f) && row < p.F && t < p.T;
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    const float q = acc[i][m][r] / den;
                    float2 o = make_float2(0.f, 0.f);
                    if (live) {
                        o.x = x[r].x * q;
                        o.y = x[r].y * q;
                    }
                    if (row < p.mrows) O[i * planeM + (long)row * p.Tp + t] = o;
                }
            }
        }
    }
    if (do_tail) {
        float* sT = sW;                                        // [S][64] numerators of the tail row (the W tile is no longer read)
        __syncthreads();
        if (g < S) sT[g * 64 + tcol] = tacc0;
        if (g + 4 < S) sT[(g + 4) * 64 + tcol] = tacc1;
        __syncthreads();
        float den;
        if (SOFT) {
            den = tden;
        } else {
            den = sT[tcol];
#pragma unroll
            for (int i = 1; i < S; ++i) den += sT[i * 64 + tcol];
        }
        const int t = t0 + tcol, row = p.F - 1;
        const float2 x = X[(long)row * p.Tp + t];
        const bool live = !(den <= 0.f) && t < p.T;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = g + 4 * j;
            if (i < S) {
                const float q = (j ? tacc1 : tacc0) / den;
                float2 o = make_float2(0.f, 0.f);
                if (live) {
                    o.x = x.x * q;
                    o.y = x.y * q;
                }
                O[i * planeM + (long)row * p.Tp + t] = o;
                for (int rz = p.F; rz < p.Fp; ++rz) O[i * planeM + (long)rz * p.Tp + t] = make_float2(0.f, 0.f);
            }
        }
    }
}

template <int S>
static void ratio_launch_s(const RatioArgs& a, dim3 grid, hipStream_t s) {
    if (a.masks) hipLaunchKernelGGL((ratio_kernel<S, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((ratio_kernel<S, false>), grid, dim3(256), 0, s, a);
}

// One launch for `batch` files of a.M channels and S targets, the soft form when a.masks is given.  The caller has checked its arguments
// (1 <= S <= 8, a.M * batch <= 65535, a.nsig_pitch >= S * a.M) and filled every field of `a` but tail and mrows.
static int ratio_launch(RatioArgs a, int S, int batch, hipStream_t s) {
    a.tail = (a.F > 32 && (a.F % 32) == 1) ? 1 : 0;
    a.mrows = a.tail ? a.F - 1 : a.Fp;
    const dim3 grid(a.Tp / RATIO_BN, gccnmf_ceil_div(a.mrows, RATIO_BM), a.M * batch);
    switch (S) {
        case 1: ratio_launch_s<1>(a, grid, s); break;
        case 2: ratio_launch_s<2>(a, grid, s); break;
        case 3: ratio_launch_s<3>(a, grid, s); break;
        case 4: ratio_launch_s<4>(a, grid, s); break;
        case 5: ratio_launch_s<5>(a, grid, s); break;
        case 6: ratio_launch_s<6>(a, grid, s); break;
        case 7: ratio_launch_s<7>(a, grid, s); break;
        default: ratio_launch_s<8>(a, grid, s); break;
    }
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}
