// D(V || W.H) = sum_{f < F, n < N} V log(V / R) - V + R with R = W.H: the objective of performKLNMF (gccNMF/gccNMFFunctions.py:69-83),
// which the reference never evaluates.  Stage 7 of gccnmf_klnmf_stage.
//
// The GEMM is K3's (R = V / (W.H)): the register-staged f32-MFMA tile of gemm_mfma.h -- its staging, fragment and MFMA helpers -- as ONE
// fixed form, 128 x 64 outputs per workgroup of four waves (32 x 64 per wave), whatever the batch: a file's tiles, and with them every
// bit of its sum, depend on (F, N, K) alone.  R is never stored: the epilogue forms each term in registers (gccnmf_kl_term, divergence.h)
// and adds the tile's terms up in float64.
//   lane       its 32 terms in accumulator order (column half, then register), each converted to double first
//   wave       xor-butterfly over the 64 lanes (32, 16, ... 1)
//   workgroup  (w0 + w1) + (w2 + w3) through LDS -> partials[file][tile], tile = row tile * column tiles + column tile
//   file       kl_divergence_sum_kernel: thread t adds tiles t, t + 256, ... in ascending order, then a binary tree over the 256 threads
// No atomics: the order is fixed by (F, N), so a file alone, in any batch, and from run to run gives the same double.
// Everything outside f < F, n < N, k < K is masked by predicate: rows and columns beyond F / N are clamped on load and dropped from
// the sum, reduction indexes beyond K are replaced by zeros while staging -- the padding may hold anything, NaN included.
#include "gemm_mfma.h"
#include "divergence.h"

#define KLD_BM 128
#define KLD_BN 64
#define KLD_BK 16
#define KLD_NT 256

struct KlDivArgs {
    const float* V;
    const float* W;
    const float* H;
    long sV, sW, sH;
    int ldv, ldw, ldh;
    int F, N, K;
    int h_clamp;               // last addressable float4 start column of H
    int tiles_m, tiles_n;
    double* partials;
    long s_partials;
};

// TERM: which divergence the epilogue sums -- 0 KL (gccnmf_kl_term), 1 Itakura-Saito (gccnmf_is_term; a V = 0 element contributes nothing),
// 2 Euclidean (gccnmf_euclidean_term); the GEMM, the masks and the order of the sums are the same for all three.
template <int TERM>
__device__ __forceinline__ float kl_divergence_term(float v, float r) {
    return TERM == 1 ? gccnmf_is_term(v, r) : TERM == 2 ? gccnmf_euclidean_term(v, r) : gccnmf_kl_term(v, r);
}

template <int TERM>
__global__ __launch_bounds__(KLD_NT, 2) void kl_divergence_tile_kernel(KlDivArgs p) {
    constexpr int BM = KLD_BM, BN = KLD_BN, BK = KLD_BK, NT = KLD_NT;
    constexpr int LDA = BK + 1;
    constexpr int SA = BM * LDA, SB = BK * BN, SBUF = SA + SB;
    constexpr int UA = BM * 4 / NT, UB = BN * 4 / NT;
    static_assert(UA == 2 && UB == 1 && SA % 4 == 0 && SBUF % 4 == 0, "tile / thread mismatch");
    __shared__ __attribute__((aligned(16))) float smem[2 * SBUF];
    __shared__ double s_wave[4];

    const int tiles = p.tiles_m * p.tiles_n;
    const int file = __builtin_amdgcn_readfirstlane((int)blockIdx.x / tiles);
    const int tile = __builtin_amdgcn_readfirstlane((int)blockIdx.x - file * tiles);
    const int tm = tile / p.tiles_n, tn = tile - tm * p.tiles_n;
    const int row0 = tm * BM, col0 = tn * BN;
    const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int arow = wm * 32 + l31, bcol = l31;

    const float* __restrict__ A = p.W + file * p.sW;
    const float* __restrict__ B = p.H + file * p.sH;
    const bool wave_active = (row0 + wm * 32) < p.F;

    f32x16 acc[1][2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][n][r] = 0.f;

    int offA[UA], offB[UB];
    gemm_operand_offsets<BM, NT, UA, true>(offA, p.ldw, row0, p.F - 1, tid);        // rows beyond F are never read
    gemm_operand_offsets<BN, NT, UB, false>(offB, p.ldh, col0, p.h_clamp, tid);
    float4 ra[UA], rb[UB];
    const int ka = 4 * (tid & 3), kb = tid / (BN / 4);      // this thread's reduction indexes inside a k-tile: W columns ka .. ka + 3, H row kb

    // reduction indexes >= K come in as zeros (selected, not multiplied: the padding may hold NaN)
#define KLD_LOAD_TILE(k0_)                                                                      \
    do {                                                                                        \
        gemm_load_operand<UA>(ra, A + (long)(k0_), offA);                                       \
        gemm_load_operand<UB>(rb, B + (long)(k0_) * p.ldh, offB);                               \
        const int left_ = p.K - (k0_);                                                          \
        _Pragma("unroll") for (int i_ = 0; i_ < UA; ++i_) {                                     \
            ra[i_].x = ka + 0 < left_ ? ra[i_].x : 0.f;                                         \
            ra[i_].y = ka + 1 < left_ ? ra[i_].y : 0.f;                                         \
            ra[i_].z = ka + 2 < left_ ? ra[i_].z : 0.f;                                         \
            ra[i_].w = ka + 3 < left_ ? ra[i_].w : 0.f;                                         \
        }                                                                                       \
        if (!(kb < left_)) rb[0] = make_float4(0.f, 0.f, 0.f, 0.f);                             \
    } while (0)
#define KLD_STORE_TILE(buf_)                                                                    \
    do {                                                                                        \
        float* sbuf_ = smem + (buf_) * SBUF;                                                    \
        gemm_store_operand<BM, NT, UA, true, LDA>(ra, sbuf_, tid);                              \
        gemm_store_operand<BN, NT, UB, false, BN>(rb, sbuf_ + SA, tid);                         \
    } while (0)

    // the k loop of gccnmf_gemm_kernel: tile kt from buffer kt & 1, tile kt + 1 on its way into the other one, tile kt + 2 into registers
    const int nkt = (p.K + BK - 1) / BK;
    KLD_LOAD_TILE(0);
    KLD_STORE_TILE(0);
    if (nkt > 1) KLD_LOAD_TILE(BK);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nkt) KLD_STORE_TILE(cur ^ 1);
        if (kt + 2 < nkt) KLD_LOAD_TILE((kt + 2) * BK);
        const float* __restrict__ sA = smem + cur * SBUF;
        const float* __restrict__ sB = sA + SA;
        if (wave_active) {
#pragma unroll
            for (int pp = 0; pp < BK / 2; ++pp) {
                float a[1], b[2];
                gemm_read_frags<BM, BN, true, false, LDA, BN, 1>(a, b, sA, sB, arow, bcol, 2 * pp + hh);
                gemm_mma8<1>(acc, a, b);
            }
        }
        __syncthreads();
    }
#undef KLD_LOAD_TILE
#undef KLD_STORE_TILE

    // ---- epilogue: MFMA C/D layout col = lane & 31 (+ 32), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) -----------------------------
    double sum = 0.0;
    if (wave_active) {
        const float* __restrict__ V = p.V + file * p.sV;
        const int row_base = row0 + wm * 32 + 4 * hh;
        const int col_a = col0 + l31, col_b = col_a + 32;
        const bool ok_a = col_a < p.N, ok_b = col_b < p.N;
        const int ca = min(col_a, p.N - 1), cb = min(col_b, p.N - 1);
        float va[16], vb[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {          // every load up front, from clamped (valid) addresses
            const long ro = (long)min(row_base + (r & 3) + 8 * (r >> 2), p.F - 1) * p.ldv;
            va[r] = V[ro + ca];
            vb[r] = V[ro + cb];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool ok = (row_base + (r & 3) + 8 * (r >> 2)) < p.F;
            if (ok && ok_a) sum += (double)kl_divergence_term<TERM>(va[r], acc[0][0][r]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool ok = (row_base + (r & 3) + 8 * (r >> 2)) < p.F;
            if (ok && ok_b) sum += (double)kl_divergence_term<TERM>(vb[r], acc[0][1][r]);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) s_wave[wm] = sum;
    __syncthreads();
    if (tid == 0) p.partials[file * p.s_partials + tile] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

// out[b] = the file's tile partials: strided per-thread sums in ascending tile order, then a binary tree.  grid = batch.
__global__ __launch_bounds__(256) void kl_divergence_sum_kernel(const double* __restrict__ partials, long s_partials, int tiles,
                                                                double* __restrict__ out) {
    __shared__ double red[256];
    const double* pb = partials + blockIdx.x * s_partials;
    double s = 0.0;
    for (int i = threadIdx.x; i < tiles; i += 256) s += pb[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

int gccnmf_kl_divergence_tiles(int F, int N) { return gccnmf_ceil_div(F, KLD_BM) * gccnmf_ceil_div(N, KLD_BN); }

int gccnmf_kl_divergence_launch(const float* V, const float* W, long sW, const float* H, int F, int N, int K, int Fp, int Kp, int Np,
                                int batch, double* partials, long s_partials, double* out, hipStream_t stream, int divergence) {
    if (divergence < 0 || divergence > 2) return GCCNMF_ERR_ARG;
    if (!V || !W || !H || !partials || !out || F < 1 || N < 1 || K < 1 || batch < 1) return GCCNMF_ERR_ARG;
    if ((Kp & 3) || (Np & 3) || Fp < F || Kp < gccnmf_round_up(K, KLD_BK) || Np < gccnmf_round_up(N, 4)) return GCCNMF_ERR_ARG;      // float4 staging inside the pitches
    KlDivArgs p = {};
    p.V = V; p.W = W; p.H = H;
    p.sV = (long)Fp * Np; p.sW = sW; p.sH = (long)Kp * Np;
    p.ldv = Np; p.ldw = Kp; p.ldh = Np;
    p.F = F; p.N = N; p.K = K;
    p.h_clamp = Np - 4;
    p.tiles_m = gccnmf_ceil_div(F, KLD_BM);
    p.tiles_n = gccnmf_ceil_div(N, KLD_BN);
    p.partials = partials; p.s_partials = s_partials;
    const long tiles = (long)p.tiles_m * p.tiles_n;
    if (tiles > s_partials || tiles * batch > 0x7fffffffL) return GCCNMF_ERR_ARG;
    const dim3 grid((unsigned)(tiles * batch)), block(KLD_NT);
    if (divergence == 1) hipLaunchKernelGGL(kl_divergence_tile_kernel<1>, grid, block, 0, stream, p);
    else if (divergence == 2) hipLaunchKernelGGL(kl_divergence_tile_kernel<2>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(kl_divergence_tile_kernel<0>, grid, block, 0, stream, p);
    GCCNMF_CHECK_LAUNCH();
    hipLaunchKernelGGL(kl_divergence_sum_kernel, dim3(batch), dim3(256), 0, stream, (const double*)partials, s_partials, (int)tiles, out);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}
