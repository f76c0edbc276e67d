// Itakura-Saito and Euclidean NMF (gccnmf_klnmf / gccnmf_klnmf_stage with GCCNMF_FLAG_DIVERGENCE_IS / _EUCLIDEAN): the beta-divergence
// iteration beside KL, beta = 0 (IS) and beta = 2 (Euclid), plain multiplicative updates in the structure of gccNMFFunctions.py:75-81:
//
//   stage 1   P = W . (s * H);   IS: Q = 1 / P, R = (V * Q) * Q      Euclid: Q = P, R = V            (s: the lazy atom scale, hscale)
//   stage 2   H <- (s * H) * ((W^T . R) / ((W^T . Q + alpha) + eps))
//   stage 3   stage 1 with the new H and no scale (H carries it)
//   stage 4   Un = R . H^T,  Ud = Q . H^T
//   stage 5   Wt = W * (Un / Ud),  s = sqrt(sum_f Wt^2),  W = Wt / s,  colsumW = sum_f W
//   (stages 0 and 6 -- colsumW, s = 1, R = Q = 0 | H *= s -- are the KL call's kernels, nmf.hip)
//
// EVERY element-wise operation is a float32 operation rounded on its own, in the order written above: 1 / P and Un / Ud, accR / den are IEEE
// quotients, s * H one product, (V * Q) * Q two products left to right, (W^T.Q + alpha) + eps two additions, sum_f Wt^2 an fmaf chain, s an
// IEEE square root.  P = 0 inside the matrix gives Q = Inf and R = Inf or NaN, which propagate, like KL's V / 0; V = 0 gives R = 0 * Q * Q = 0
// for every finite Q.
//
// THE GEMMS.  One fixed form whatever the batch, the tuning keys or the shape: a workgroup of four waves owns a 128 x 64 output tile (a wave
// 32 x 64 = two blocks of v_mfma_f32_32x32x2_f32, exact-f32 fma chains), reduction tiles of 16 staged global -> registers -> LDS with the
// helpers of gemm_mfma.h, double buffered -- the loop of divergence.hip.  Stage 2 and stage 4 run their numerator and denominator GEMMs in ONE
// launch: the two products share an operand (W^T in stage 2, H^T in stage 4), which is staged once and feeds two accumulator sets.
// Every output element is one fma chain over the reduction index in ascending order (k in stage 1/3, f in stage 2, n in stage 4) from a zero
// accumulator: the order is fixed by (F, N, K) alone -- no atomics, no split reductions -- so a file's factors are bit for bit the same alone,
// in any batch and at any place in it.  Stage 5's two column reductions are 32 row phases (f = q, q + 32, ...) added in phase order.
//
// PADDING.  Rows and columns beyond an operand's valid extent are clamped on load (always in bounds) and reach only outputs that are never
// stored; reduction indexes beyond the valid extent are replaced by zeros while staging (selected, not multiplied: the padding may hold NaN,
// and 1 / P of a padded element never reaches a reduction).  Stages 1 and 3 write R and Q over the WHOLE padded [Fp][Np] block: the values
// inside f < F, n < N, exact zeros outside.  The padding of W and H is never written.
#include "gemm_mfma.h"
#include "../../include/gccnmf_hip.h"

#define BETA_BM 128
#define BETA_BN 64
#define BETA_BK 16
#define BETA_NT 256

enum BetaGemm { BETA_GEMM_P = 0, BETA_GEMM_H = 1, BETA_GEMM_U = 2 };

struct BetaGemmArgs {
    const float *A0, *A1;      // A1: the second left operand of stage 4 (Q beside R)
    const float *B0, *B1;      // B1: the second right operand of stage 2 (Q beside R)
    long sA, sB;               // per-file strides
    int lda, ldb;
    int M, N, Kd;              // valid output rows, output columns, reduction length
    int a_clamp, b_clamp;      // KC operand: last valid row; other operand: last addressable float4 start column
    int Mp, Np;                // stage 1/3: the padded extent of R and Q that is written (zeros outside M x N)
    int tiles_m, tiles_n;
    const float* bscale;       // stage 1: s, applied to H's rows while staging (nullptr: stage 3)
    const float* V;            // stage 1/3
    long sV;
    float *C0, *C1;            // stage 1/3: R, Q   stage 2: H (C0)   stage 4: Un, Ud
    long sC;
    int ldc;
    const float* hscale;       // stage 2: s
    int Kp;                    // per-file stride of the K-vectors
    float alpha, eps;
    int divergence;            // 1 = IS, 2 = Euclid
};

template <int GEMM>
__global__ __launch_bounds__(BETA_NT, 2) void nmf_beta_gemm_kernel(BetaGemmArgs p) {
    constexpr int BM = BETA_BM, BN = BETA_BN, BK = BETA_BK, NT = BETA_NT;
    constexpr bool A_KC = GEMM != BETA_GEMM_H, B_KC = GEMM == BETA_GEMM_U;      // W.H | W^T.R | R.H^T
    constexpr int NA = GEMM == BETA_GEMM_U ? 2 : 1, NB = GEMM == BETA_GEMM_H ? 2 : 1, NACC = NA * NB;
    constexpr int LDA = A_KC ? BK + 1 : BM, LDB = B_KC ? BK + 1 : BN;
    constexpr int SA = A_KC ? BM * LDA : BK * BM, SB = B_KC ? BN * LDB : BK * BN, SBUF = NA * SA + NB * SB;
    constexpr int UA = BM * 4 / NT, UB = BN * 4 / NT;
    static_assert(UA == 2 && UB == 1 && SA % 4 == 0 && SB % 4 == 0, "tile / thread mismatch");
    __shared__ __attribute__((aligned(16))) float smem[2 * SBUF];

    const int tiles = p.tiles_m * p.tiles_n;
    const int file = __builtin_amdgcn_readfirstlane((int)blockIdx.x / tiles);
    const int tile = __builtin_amdgcn_readfirstlane((int)blockIdx.x - file * tiles);
    const int tm = tile / p.tiles_n, tn = tile - tm * p.tiles_n;
    const int row0 = tm * BM, col0 = tn * BN;
    const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int arow = wm * 32 + l31, bcol = l31;

    const float* __restrict__ A0 = p.A0 + file * p.sA;
    const float* __restrict__ A1 = NA == 2 ? p.A1 + file * p.sA : nullptr;
    const float* __restrict__ B0 = p.B0 + file * p.sB;
    const float* __restrict__ B1 = NB == 2 ? p.B1 + file * p.sB : nullptr;
    const float* __restrict__ bsc = (GEMM == BETA_GEMM_P && p.bscale) ? p.bscale + (long)file * p.Kp : nullptr;
    // (stages 1 and 3 also write the zero padding of R and Q: their waves are active up to the padded row count)
    const bool wave_active = (row0 + wm * 32) < (GEMM == BETA_GEMM_P ? p.Mp : p.M);

    f32x16 acc[NACC][2];
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][n][r] = 0.f;

    int offA[UA], offB[UB];
    gemm_operand_offsets<BM, NT, UA, A_KC>(offA, p.lda, row0, p.a_clamp, tid);
    gemm_operand_offsets<BN, NT, UB, B_KC>(offB, p.ldb, col0, p.b_clamp, tid);
    float4 ra[NA][UA], rb[NB][UB];
    // this thread's reduction indexes inside a k-tile: a KC unit holds ks .. ks + 3 of one row, another unit one index (kna + 8 i | knb) of four rows / columns
    const int ks = 4 * (tid & 3), kna = tid / (BM / 4), knb = tid / (BN / 4);

#define BETA_MASK4(v_, left_)                       \
    do {                                            \
        (v_).x = ks + 0 < (left_) ? (v_).x : 0.f;   \
        (v_).y = ks + 1 < (left_) ? (v_).y : 0.f;   \
        (v_).z = ks + 2 < (left_) ? (v_).z : 0.f;   \
        (v_).w = ks + 3 < (left_) ? (v_).w : 0.f;   \
    } while (0)
    // reduction indexes >= Kd come in as zeros (selected, not multiplied: the padding may hold NaN or Inf)
#define BETA_LOAD_TILE(k0_)                                                                                 \
    do {                                                                                                    \
        const long ao_ = A_KC ? (long)(k0_) : (long)(k0_) * p.lda;                                          \
        const long bo_ = B_KC ? (long)(k0_) : (long)(k0_) * p.ldb;                                          \
        gemm_load_operand<UA>(ra[0], A0 + ao_, offA);                                                       \
        if (NA == 2) gemm_load_operand<UA>(ra[NA - 1], A1 + ao_, offA);                                     \
        gemm_load_operand<UB>(rb[0], B0 + bo_, offB);                                                       \
        if (NB == 2) gemm_load_operand<UB>(rb[NB - 1], B1 + bo_, offB);                                     \
        const int left_ = p.Kd - (k0_);                                                                     \
        if (GEMM == BETA_GEMM_P && bsc) {                                                                   \
            const float sc_ = bsc[(k0_) + knb];                                                             \
            rb[0][0].x *= sc_; rb[0][0].y *= sc_; rb[0][0].z *= sc_; rb[0][0].w *= sc_;                     \
        }                                                                                                   \
        _Pragma("unroll") for (int j_ = 0; j_ < NA; ++j_)                                                   \
            _Pragma("unroll") for (int i_ = 0; i_ < UA; ++i_) {                                             \
                if (A_KC) BETA_MASK4(ra[j_][i_], left_);                                                    \
                else if (!(kna + (NT / (BM / 4)) * i_ < left_)) ra[j_][i_] = make_float4(0.f, 0.f, 0.f, 0.f); \
            }                                                                                               \
        _Pragma("unroll") for (int j_ = 0; j_ < NB; ++j_) {                                                 \
            if (B_KC) BETA_MASK4(rb[j_][0], left_);                                                         \
            else if (!(knb < left_)) rb[j_][0] = make_float4(0.f, 0.f, 0.f, 0.f);                           \
        }                                                                                                   \
    } while (0)
#define BETA_STORE_TILE(buf_)                                                                               \
    do {                                                                                                    \
        float* sbuf_ = smem + (buf_) * SBUF;                                                                \
        _Pragma("unroll") for (int j_ = 0; j_ < NA; ++j_)                                                   \
            gemm_store_operand<BM, NT, UA, A_KC, LDA>(ra[j_], sbuf_ + j_ * SA, tid);                        \
        _Pragma("unroll") for (int j_ = 0; j_ < NB; ++j_)                                                   \
            gemm_store_operand<BN, NT, UB, B_KC, LDB>(rb[j_], sbuf_ + NA * SA + j_ * SB, tid);              \
    } while (0)

    // the k loop of divergence.hip: tile kt from buffer kt & 1, tile kt + 1 on its way into the other one, tile kt + 2 into registers
    const int nkt = (p.Kd + BK - 1) / BK;
    BETA_LOAD_TILE(0);
    BETA_STORE_TILE(0);
    if (nkt > 1) BETA_LOAD_TILE(BK);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nkt) BETA_STORE_TILE(cur ^ 1);
        if (kt + 2 < nkt) BETA_LOAD_TILE((kt + 2) * BK);
        const float* __restrict__ sA = smem + cur * SBUF;
        const float* __restrict__ sB = sA + NA * SA;
        if (wave_active) {
#pragma unroll
            for (int pp = 0; pp < BK / 2; ++pp) {
                const int kk = 2 * pp + hh;      // lane (l31, hh) supplies A[i = l31][k = hh] and B[k = hh][j = l31] of the k-pair
                float a[NA], b[NB][2];
#pragma unroll
                for (int j = 0; j < NA; ++j) a[j] = A_KC ? sA[j * SA + arow * LDA + kk] : sA[j * SA + kk * BM + arow];
#pragma unroll
                for (int j = 0; j < NB; ++j)
#pragma unroll
                    for (int n = 0; n < 2; ++n) b[j][n] = B_KC ? sB[j * SB + (bcol + n * 32) * LDB + kk] : sB[j * SB + kk * BN + bcol + n * 32];
#pragma unroll
                for (int j = 0; j < NACC; ++j)
#pragma unroll
                    for (int n = 0; n < 2; ++n)
                        acc[j][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[NA == 2 ? j : 0], b[NB == 2 ? j : 0][n], acc[j][n], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#undef BETA_LOAD_TILE
#undef BETA_STORE_TILE
#undef BETA_MASK4

    // ---- epilogue: MFMA C/D layout col = lane & 31 (+ 32), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) -----------------------------
    if (!wave_active) return;
    const int row_base = row0 + wm * 32 + 4 * hh;
    const int col_a = col0 + l31, col_b = col_a + 32;
    const bool ok_a = col_a < p.N, ok_b = col_b < p.N;
    const int ca = min(col_a, p.N - 1), cb = min(col_b, p.N - 1);
    if (GEMM == BETA_GEMM_P) {
        const float* __restrict__ V = p.V + file * p.sV;
        float* __restrict__ R = p.C0 + file * p.sC;
        float* __restrict__ Q = p.C1 + file * p.sC;
        float va[16], vb[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {          // every load up front, from clamped (valid) addresses
            const long ro = (long)min(row_base + (r & 3) + 8 * (r >> 2), p.M - 1) * p.ldc;
            va[r] = V[ro + ca];
            vb[r] = V[ro + cb];
        }
        const bool is = p.divergence == 1;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row_base + (r & 3) + 8 * (r >> 2);
            const bool in = row < p.M;
            const float pa = acc[0][0][r], pb = acc[0][1][r];
            float qa = pa, qb = pb, xa = va[r], xb = vb[r];
            if (is) {
                qa = 1.f / pa;
                qb = 1.f / pb;
                xa = (va[r] * qa) * qa;
                xb = (vb[r] * qb) * qb;
            }
            if (row < p.Mp) {
                const long ro = (long)row * p.ldc;
                if (col_a < p.Np) {
                    R[ro + col_a] = (in && ok_a) ? xa : 0.f;
                    Q[ro + col_a] = (in && ok_a) ? qa : 0.f;
                }
                if (col_b < p.Np) {
                    R[ro + col_b] = (in && ok_b) ? xb : 0.f;
                    Q[ro + col_b] = (in && ok_b) ? qb : 0.f;
                }
            }
        }
    } else if (GEMM == BETA_GEMM_H) {
        float* H = p.C0 + file * p.sC;          // read-modify-write: all reads first
        const float* __restrict__ hs = p.hscale + (long)file * p.Kp;
        float ha[16], hb[16], sc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rc = min(row_base + (r & 3) + 8 * (r >> 2), p.M - 1);
            ha[r] = H[(long)rc * p.ldc + ca];
            hb[r] = H[(long)rc * p.ldc + cb];
            sc[r] = hs[rc];
        }
        float ua[16], ub[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float da = (acc[1][0][r] + p.alpha) + p.eps, db = (acc[1][1][r] + p.alpha) + p.eps;
            ua[r] = (ha[r] * sc[r]) * (acc[0][0][r] / da);
            ub[r] = (hb[r] * sc[r]) * (acc[0][1][r] / db);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row_base + (r & 3) + 8 * (r >> 2);
            if (row < p.M) {
                if (ok_a) H[(long)row * p.ldc + col_a] = ua[r];
                if (ok_b) H[(long)row * p.ldc + col_b] = ub[r];
            }
        }
    } else {
        float* __restrict__ Un = p.C0 + file * p.sC;
        float* __restrict__ Ud = p.C1 + file * p.sC;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row_base + (r & 3) + 8 * (r >> 2);
            if (row < p.M) {
                const long ro = (long)row * p.ldc;
                if (ok_a) {
                    Un[ro + col_a] = acc[0][0][r];
                    Ud[ro + col_a] = acc[1][0][r];
                }
                if (ok_b) {
                    Un[ro + col_b] = acc[0][1][r];
                    Ud[ro + col_b] = acc[1][1][r];
                }
            }
        }
    }
}

// Stage 5: the arithmetic of nmf_semi_update_w_kernel with a denominator per element (Wt = W * (Un / Ud), an fmaf sum of squares, sqrtf, the
// division by the norm, the column sum of the normalised atom), any F.  grid = batch x ceil(K / 8), 256 threads = 8 atoms x 32 row phases; W,
// Un and Ud are read twice (L2-resident).  An element whose denominator is 0 takes the path KL's stage 5 takes (u / 0).  Atoms >= K are not
// touched: the padding of W stays zero, their hscale 1 and their colsumW 0 from stage 0.
#define BETA_AT 8
__global__ __launch_bounds__(256) void nmf_beta_update_w_kernel(float* __restrict__ W, const float* __restrict__ Un, const float* __restrict__ Ud,
                                                                float* __restrict__ colsumW, float* __restrict__ hscale, int F, int K, int Fp,
                                                                int Kp, int chunks) {
    constexpr int PH = 256 / BETA_AT;
    __shared__ float red[256];
    __shared__ float s_norm[BETA_AT];
    const int b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;
    const int c = threadIdx.x % BETA_AT, q = threadIdx.x / BETA_AT;
    const int j = ch * BETA_AT + c;
    const bool valid = j < K;
    const int k = valid ? j : K - 1;
    float* Wb = W + (long)b * Fp * Kp;
    const float* Nb = Un + (long)b * Fp * Kp;
    const float* Db = Ud + (long)b * Fp * Kp;
    float ss = 0.f;
    if (valid)
#pragma unroll 4
        for (int f = q; f < F; f += PH) {
            const long i = (long)f * Kp + k;
            const float wt = Wb[i] * (Nb[i] / Db[i]);
            ss = fmaf(wt, wt, ss);
        }
    red[threadIdx.x] = ss;
    __syncthreads();
    if (q == 0) {
        float t = 0.f;
#pragma unroll
        for (int ph = 0; ph < PH; ++ph) t += red[c + BETA_AT * ph];
        s_norm[c] = sqrtf(t);
    }
    __syncthreads();
    const float norm = s_norm[c];
    float cs = 0.f;
    if (valid)
#pragma unroll 4
        for (int f = q; f < F; f += PH) {
            const long i = (long)f * Kp + k;
            const float wn = (Wb[i] * (Nb[i] / Db[i])) / norm;
            Wb[i] = wn;
            cs += wn;
        }
    red[threadIdx.x] = cs;
    __syncthreads();
    if (q == 0 && valid) {
        float t = 0.f;
#pragma unroll
        for (int ph = 0; ph < PH; ++ph) t += red[c + BETA_AT * ph];
        colsumW[(long)b * Kp + k] = t;
        hscale[(long)b * Kp + k] = norm;
    }
}

// The envelope of the IS / Euclidean call: every shape the four-launch KL form accepts up to F = 2049 bins and K = 1024 atoms, any N.
bool gccnmf_klnmf_beta_supported(int F, int K) { return F >= 2 && F <= 2049 && K >= 1 && K <= 1024; }

// Stages 1-5 of the IS (divergence = 1) / Euclidean (2) iteration.  V, R, Q [batch][Fp][Np], W, Un, Ud [batch][Fp][Kp], H [batch][Kp][Np],
// colsumW, hscale [batch][Kp]; Np = round_up(N, 64).
int gccnmf_klnmf_beta_stage_launch(int stage, int divergence, const float* V, float* W, float* H, float* R, float* Q, float* Un, float* Ud,
                                   float* colsumW, float* hscale, int F, int N, int K, int batch, float alpha, float eps, hipStream_t s) {
    if (!gccnmf_klnmf_beta_supported(F, K) || N < 1 || batch < 1 || (divergence != 1 && divergence != 2)) return GCCNMF_ERR_UNSUPPORTED;
    const GccNmfPitches pt = gccnmf_make_pitches(F, 1, K);
    const int Fp = pt.Fp, Kp = pt.Kp, Np = gccnmf_round_up(N, 64);
    const long sV = (long)Fp * Np, sW = (long)Fp * Kp, sH = (long)Kp * Np;
    BetaGemmArgs a = {};
    a.Kp = Kp; a.alpha = alpha; a.eps = eps; a.divergence = divergence;
    long tiles = 0;
    switch (stage) {
        case 1:
        case 3:
            a.A0 = W; a.sA = sW; a.lda = Kp; a.a_clamp = F - 1;
            a.B0 = H; a.sB = sH; a.ldb = Np; a.b_clamp = Np - 4;
            a.M = F; a.N = N; a.Kd = K; a.Mp = Fp; a.Np = Np;
            a.bscale = stage == 1 ? hscale : nullptr;
            a.V = V; a.sV = sV;
            a.C0 = R; a.C1 = Q; a.sC = sV; a.ldc = Np;
            a.tiles_m = gccnmf_ceil_div(Fp, BETA_BM); a.tiles_n = Np / BETA_BN;
            tiles = (long)a.tiles_m * a.tiles_n * batch;
            if (tiles > 0x7fffffffL) return GCCNMF_ERR_UNSUPPORTED;
            hipLaunchKernelGGL(nmf_beta_gemm_kernel<BETA_GEMM_P>, dim3((unsigned)tiles), dim3(BETA_NT), 0, s, a);
            break;
        case 2:
            a.A0 = W; a.sA = sW; a.lda = Kp; a.a_clamp = Kp - 4;
            a.B0 = R; a.B1 = Q; a.sB = sV; a.ldb = Np; a.b_clamp = Np - 4;
            a.M = K; a.N = N; a.Kd = F;
            a.C0 = H; a.sC = sH; a.ldc = Np;
            a.hscale = hscale;
            a.tiles_m = gccnmf_ceil_div(K, BETA_BM); a.tiles_n = gccnmf_ceil_div(N, BETA_BN);
            tiles = (long)a.tiles_m * a.tiles_n * batch;
            if (tiles > 0x7fffffffL) return GCCNMF_ERR_UNSUPPORTED;
            hipLaunchKernelGGL(nmf_beta_gemm_kernel<BETA_GEMM_H>, dim3((unsigned)tiles), dim3(BETA_NT), 0, s, a);
            break;
        case 4:
            a.A0 = R; a.A1 = Q; a.sA = sV; a.lda = Np; a.a_clamp = F - 1;
            a.B0 = H; a.sB = sH; a.ldb = Np; a.b_clamp = K - 1;
            a.M = F; a.N = K; a.Kd = N;
            a.C0 = Un; a.C1 = Ud; a.sC = sW; a.ldc = Kp;
            a.tiles_m = gccnmf_ceil_div(F, BETA_BM); a.tiles_n = gccnmf_ceil_div(K, BETA_BN);
            tiles = (long)a.tiles_m * a.tiles_n * batch;
            if (tiles > 0x7fffffffL) return GCCNMF_ERR_UNSUPPORTED;
            hipLaunchKernelGGL(nmf_beta_gemm_kernel<BETA_GEMM_U>, dim3((unsigned)tiles), dim3(BETA_NT), 0, s, a);
            break;
        case 5: {
            const int chunks = gccnmf_ceil_div(K, BETA_AT);
            hipLaunchKernelGGL(nmf_beta_update_w_kernel, dim3((unsigned)batch * chunks), dim3(256), 0, s, W, Un, Ud, colsumW, hscale, F, K, Fp, Kp, chunks);
            break;
        }
        default: return GCCNMF_ERR_ARG;
    }
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}
