// libgccnmf_array.so: the two stages of M-channel (microphone-array) GCC-NMF that the stereo kernels cannot serve (include/gccnmf_array.h,
// DESIGN section 4j).  A library of its own: it takes nothing from the separation library but the status codes of common.h and includes
// no GEMM header.
//
//   gccnmf_array_features     V = the magnitudes of all M channels side by side, CC = the PHAT coherence of all P = M (M - 1) / 2
//                             microphone pairs STACKED along the bin axis (pair p owns rows p Fp .. p Fp + F - 1), the arithmetic of
//                             gcc_magnitude_kernel / gcc_coherence_kernel (gcc.hip) per element, every padding element written as 0
//   gccnmf_array_reconstruct  the ratio-mask reconstruction of ratio.hip for M channels: the same tile, the same k-ordered f32 fma chains on
//                             v_mfma_f32_32x32x2_f32, the same VALU Nyquist row, the same epilogue; only the (file, channel) of a workgroup,
//                             the column pitch of H and the slot of an output plane know about M
#include "common.h"
#include "../../include/gccnmf_array.h"

#define ARRAY_VERSION 100

// pair p -> (a, b), a < b, lexicographic: (0,1), (0,2), ..., (M-2,M-1)
__device__ __forceinline__ void array_pair(int p, int M, int& a, int& b) {
    a = 0;
    while (p >= M - 1 - a) {
        p -= M - 1 - a;
        ++a;
    }
    b = a + 1 + p;
}

// V[f][c*T + t] = |X[c][f][t]|, zero in rows >= F and columns >= M*T.  grid = (Np / 256 rounded up, Fp, batch)
__global__ __launch_bounds__(256) void array_magnitude_kernel(const float2* __restrict__ X, int M, int F, int Fp, int T, int Tp, int Np,
                                                              float* __restrict__ V) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int f = blockIdx.y, b = blockIdx.z;
    if (n >= Np) return;
    float v = 0.f;
    if (f < F && n < M * T) {
        const int c = n / T, t = n - c * T;
        const float2 x = X[((long)b * M + c) * Fp * Tp + (long)f * Tp + t];
        v = hypotf(x.x, x.y);
    }
    V[(long)b * Fp * Np + (long)f * Np + n] = v;
}

// Row p*Fp + f of CC = X_a conj(X_b) / |X_a| / |X_b| of pair p = (a, b): gcc_coherence_kernel's expressions with xl = X_a, xr = X_b,
// zero in rows >= F of a pair's block and frames >= T.  grid = (Tp / 256 rounded up, P * Fp, batch)
__global__ __launch_bounds__(256) void array_coherence_kernel(const float2* __restrict__ X, int M, int P, int F, int Fp, int T, int Tp,
                                                              float* __restrict__ CC) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int row = blockIdx.y, b = blockIdx.z;
    if (t >= Tp) return;
    const int p = row / Fp, f = row - p * Fp;
    const long plane = (long)Fp * Tp;
    float re = 0.f, im = 0.f;
    if (f < F && t < T) {
        int ca, cb;
        array_pair(p, M, ca, cb);
        const float2 xl = X[((long)b * M + ca) * plane + (long)f * Tp + t];
        const float2 xr = X[((long)b * M + cb) * plane + (long)f * Tp + t];
        const float aL = hypotf(xl.x, xl.y), aR = hypotf(xr.x, xr.y);
        // gcc_coherence_kernel writes re = xl.x xr.x + xl.y xr.y, im = xl.y xr.x - xl.x xr.y and leaves the contraction to the compiler,
        // which rounds the SECOND product of each and fuses the first.  Stated here, so that these bits do not depend on how the
        // surrounding code steers that choice (tests/test_gpu_array_stages.py compares the two kernels bit for bit).
        re = fmaf(xl.x, xr.x, xl.y * xr.y);
        im = fmaf(xl.y, xr.x, -(xl.x * xr.y));
        if (aL > 0.f && aR > 0.f) {
            re = re / aL / aR;
            im = im / aL / aR;
        } else {
            re = 0.f;   // a bin that is exactly 0 in f32 carries no phase: it contributes nothing
            im = 0.f;
        }
    }
    float* Cb = CC + (long)b * 2 * P * plane + (long)row * Tp + t;
    Cb[0] = re;
    Cb[(long)P * plane] = im;
}

// ---- ratio-mask reconstruction for M channels (the kernel of ratio.hip; see there for the tile) ---------------------------------------
typedef float array_f32x16 __attribute__((ext_vector_type(16)));

#define ARRAY_BM 128
#define ARRAY_BN 64
#define ARRAY_BK 16
#define ARRAY_LDW 17      // W tile row pitch in LDS: the 32 rows of an A-fragment read fall in 32 different banks

struct ArrayRatioArgs {
    const float* W;               // [batch][Fp][Kp]
    const float* H;               // [batch][Kp][Np], channel c at columns c*T ..
    const unsigned char* argmax;  // [batch][Kp][Tp]
    const float* masks;           // [batch][S][Kp][Tp]
    const float2* X;              // [batch][M][Fp][Tp]
    float2* spec;                 // [batch][nsig_pitch][Fp][Tp], slot i*M + c
    int M, nsig_pitch;
    int F, Fp, T, Tp, Np, K, Kp;
    int mrows;                    // rows the MFMA tiles own: Fp, or F - 1 when the last row is the VALU tail
    int tail;
};

template <int S, bool SOFT>
__global__ __launch_bounds__(256) void array_ratio_kernel(const ArrayRatioArgs p) {
    constexpr int NB = SOFT ? S + 1 : 1;              // B tiles in LDS: h (one-hot) | h * m_0 .. h * m_{S-1}, h (soft)
    __shared__ float sW[ARRAY_BM * ARRAY_LDW];
    __shared__ float sB[NB][ARRAY_BK * ARRAY_BN];
    __shared__ unsigned char sAm[ARRAY_BK * ARRAY_BN];
    __shared__ float sWt[ARRAY_BK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5, wm = wave >> 1, wn = wave & 1;
    const int t0 = blockIdx.x * ARRAY_BN, row0 = blockIdx.y * ARRAY_BM;
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
            float* d = sW + (u >> 2) * ARRAY_LDW + 4 * (u & 3);
            d[0] = rw[j].x;
            d[1] = rw[j].y;
            d[2] = rw[j].z;
            d[3] = rw[j].w;
        }
        if (do_tail && tid < 4) *(float4*)(sWt + 4 * tid) = rwt;
        const int o = hk * ARRAY_BN + ht;
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

    array_f32x16 acc[S][2], accd[2];
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

    const int Kr = (p.K + ARRAY_BK - 1) / ARRAY_BK * ARRAY_BK;
    const int arow = wm * 64 + l31, bcol = wn * 32 + l31;
    load_chunk(0);
    for (int k0 = 0; k0 < Kr; k0 += ARRAY_BK) {
        __syncthreads();                                       // the previous chunk's fragment reads are done
        store_chunk();
        __syncthreads();
        if (k0 + ARRAY_BK < Kr) load_chunk(k0 + ARRAY_BK);
#pragma unroll
        for (int kk = 0; kk < ARRAY_BK; kk += 2) {
            // lane (l31, hh) supplies A[i = l31][k = hh] and B[k = hh][j = l31]
            float a[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) a[m] = sW[(arow + 32 * m) * ARRAY_LDW + kk + hh];
            const int bo = (kk + hh) * ARRAY_BN + bcol;
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
            for (int kk = 0; kk < ARRAY_BK; ++kk) {
                const float w = sWt[kk];
                const int bo = kk * ARRAY_BN + tcol;
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
static void array_ratio_launch(const ArrayRatioArgs& a, bool soft, dim3 grid, hipStream_t s) {
    if (soft) hipLaunchKernelGGL((array_ratio_kernel<S, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((array_ratio_kernel<S, false>), grid, dim3(256), 0, s, a);
}

extern "C" {

int gccnmf_array_version(void) { return ARRAY_VERSION; }

int gccnmf_array_features(const float* X, int M, int F, int T, int batch, float* V, float* CC, void* stream) {
    // every check comes before the first HIP call
    if (M < GCCNMF_ARRAY_MIN_CHANNELS || M > GCCNMF_ARRAY_MAX_CHANNELS || !X || (!V && !CC) || F < 2 || T < 1 || batch < 1)
        return GCCNMF_ERR_ARG;
    const int P = M * (M - 1) / 2;
    const int Fp = gccnmf_round_up(F, 16), Tp = gccnmf_round_up(T, 64);
    if ((long)M * T > 0x7fffffffL - 64 || batch > 65535 || P * Fp > 65535) return GCCNMF_ERR_UNSUPPORTED;
    const int Np = gccnmf_round_up(M * T, 64);
    hipStream_t s = (hipStream_t)stream;
    if (V) {
        hipLaunchKernelGGL(array_magnitude_kernel, dim3(gccnmf_ceil_div(Np, 256), Fp, batch), dim3(256), 0, s, (const float2*)X, M, F, Fp, T,
                           Tp, Np, V);
        GCCNMF_CHECK_LAUNCH();
    }
    if (CC) {
        hipLaunchKernelGGL(array_coherence_kernel, dim3(gccnmf_ceil_div(Tp, 256), P * Fp, batch), dim3(256), 0, s, (const float2*)X, M, P, F,
                           Fp, T, Tp, CC);
        GCCNMF_CHECK_LAUNCH();
    }
    return GCCNMF_OK;
}

int gccnmf_array_reconstruct(const float* W, const float* H, const unsigned char* argmax, const float* masks, const float* X, int M, int F,
                             int T, int K, int S, int batch, int nsig_pitch, float* spec, void* stream) {
    // every check comes before the first HIP call
    if (!W || !H || (!argmax && !masks) || !X || !spec || M < GCCNMF_ARRAY_MIN_CHANNELS || M > GCCNMF_ARRAY_MAX_CHANNELS || F < 2 || T < 1 ||
        K < 1 || batch < 1)
        return GCCNMF_ERR_ARG;
    if (S < 1 || S > GCCNMF_ARRAY_MAX_TARGETS) return GCCNMF_ERR_UNSUPPORTED;
    if (nsig_pitch < S * M) return GCCNMF_ERR_ARG;
    if ((long)M * T > 0x7fffffffL - 64 || (long)M * batch > 65535) return GCCNMF_ERR_UNSUPPORTED;
    ArrayRatioArgs a;
    a.W = W; a.H = H; a.argmax = argmax; a.masks = masks; a.X = (const float2*)X; a.spec = (float2*)spec;
    a.M = M; a.nsig_pitch = nsig_pitch;
    a.F = F; a.Fp = gccnmf_round_up(F, 16); a.T = T; a.Tp = gccnmf_round_up(T, 64); a.Np = gccnmf_round_up(M * T, 64);
    a.K = K; a.Kp = gccnmf_round_up(K, 64);
    a.tail = (F > 32 && (F % 32) == 1) ? 1 : 0;
    a.mrows = a.tail ? F - 1 : a.Fp;
    const bool soft = masks != nullptr;
    const dim3 grid(a.Tp / ARRAY_BN, gccnmf_ceil_div(a.mrows, ARRAY_BM), M * batch);
    hipStream_t s = (hipStream_t)stream;
    switch (S) {
        case 1: array_ratio_launch<1>(a, soft, grid, s); break;
        case 2: array_ratio_launch<2>(a, soft, grid, s); break;
        case 3: array_ratio_launch<3>(a, soft, grid, s); break;
        case 4: array_ratio_launch<4>(a, soft, grid, s); break;
        case 5: array_ratio_launch<5>(a, soft, grid, s); break;
        case 6: array_ratio_launch<6>(a, soft, grid, s); break;
        case 7: array_ratio_launch<7>(a, soft, grid, s); break;
        default: array_ratio_launch<8>(a, soft, grid, s); break;
    }
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

}  // extern "C"
