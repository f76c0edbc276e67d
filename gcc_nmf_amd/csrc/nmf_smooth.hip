// Temporal-continuity KL-NMF (gccnmf_klnmf / gccnmf_klnmf_stage with GCCNMF_FLAG_CONTINUITY): KL-NMF whose H update carries Virtanen's
// temporal-continuity term (IEEE TASLP 2007), the first stage of the iteration that couples a column of H to its neighbours.
//
// THE UPDATE.  The columns are `segments` equal runs of T = N / segments frames (1: a plain matrix, 2: the GCC-NMF layout [L | R]); nothing
// couples across a segment boundary or into the padding.  Per file, atom k and segment, with h = s * H the materialised gains (s: the lazy
// atom scale, hscale):
//
//   E = sum_t h_t^2        D = sum_{t >= 1} (h_t - h_{t-1})^2        cost c = T * D / E          (scale invariant: the atom normalisation leaves it alone)
//   Gp_t = 2 T n_t h_t / E                                   n_t = the neighbours inside the segment (2, at the ends 1, T = 1: 0)
//   Gm_t = 2 T (h_{t-1} + h_{t+1}) / E + 2 T h_t D / E^2     a missing neighbour adds 0;   E = 0  ->  Gp = Gm = 0
//   H <- h * ((W^T (V / (W h)) + beta Gm) / (((colsumW + alpha) + beta Gp) + eps))
//
// Gp - Gm is dc / dh_t.  The update is Jacobi: every neighbour is the value from before the stage, which is why stage 2 is TWO launches -- a
// column tile's edge columns belong to another workgroup that overwrites them in the same launch, so the H update cannot read neighbours in place.
//
//   stage 1, 3   R = V / (W . (s * H))   (3: no scale)              the whole padded [Fp][Np] block is written, exact zeros outside F x N
//   stage 2      launch A (rows):  E, D, Gm, Gp from H and s;       launch B (GEMM): W^T . R with the update above in the epilogue
//   stage 4      U = R . H^T (GEMM);  rowsumH = sum_n H (rows)
//   (stages 0, 5, 6 -- colsumW, s = 1, R = 0 | the W update and normalisation | H *= s -- are the KL call's kernels, nmf.hip; stage 5 always
//   the two-pass kernel on 16 atoms per workgroup)
//
// THE ROW LAUNCH.  One wave owns one (file, atom, segment) row: lane l takes the frames l, l + 64, ... of it, so a pass of the wave is 64
// frames and every row is read twice (the sums, then the terms; a row is a few KB, so the second read should hit L2): there is no
// register-resident form and so no capacity at which the path changes.
// ROUNDINGS of the row launch: h_t = (double)s * (double)H_t is EXACT (48 bits), the differences, squares, sums and the terms are float64
// operations; E and D are a lane's ascending partial sums joined by a six-step xor butterfly (32, 16, ..., 1) -- an order fixed by
// (N, segments) alone, no atomics -- and are stored rounded ONCE to float32, as are Gm and Gp (from the float64 E and D, not from the stored
// ones).  ROUNDINGS of the epilogue, all float32, each rounded on its own in this order: h = s * H; num = acc + beta * Gm (a product, a
// sum); den = ((colsumW + alpha) + beta * Gp) + eps (a product, three sums); the IEEE quotient num / den; the product with h.  R = V / P is an
// IEEE quotient; rowsumH is a lane's ascending float32 partial sums joined by the same butterfly.
//
// THE GEMMS are the register-staging form of nmf_beta.hip with one operand pair: a workgroup of four waves owns a 128 x 64 output tile (a wave
// 32 x 64 = two blocks of v_mfma_f32_32x32x2_f32), reduction tiles of 16 staged global -> registers -> LDS with the helpers of gemm_mfma.h,
// double buffered.  ONE form whatever the batch, the tuning keys or the shape: every output element is one fma chain over its reduction index
// in ascending order from a zero accumulator, so a file's factors are bit for bit the same alone, in any batch and at any place in it.
//
// PADDING.  Rows and columns beyond an operand's valid extent are clamped on load (always in bounds) and reach only outputs that are never
// stored; reduction indexes beyond the valid extent are replaced by zeros while staging (selected, not multiplied: the padding may hold NaN).
// The row launch reads H inside k < K, n < N alone -- column T - 1 of a segment has no right neighbour -- and writes Gm, Gp there alone; the
// H update writes +0 into the padding columns n >= N of the rows k < K (rows k >= K are not touched).
#include "gemm_mfma.h"
#include "../../include/gccnmf_hip.h"

#define SMOOTH_BM 128
#define SMOOTH_BN 64
#define SMOOTH_BK 16
#define SMOOTH_NT 256

enum SmoothGemm { SMOOTH_GEMM_P = 0, SMOOTH_GEMM_H = 1, SMOOTH_GEMM_U = 2 };

struct SmoothGemmArgs {
    const float *A, *B;
    long sA, sB;               // per-file strides
    int lda, ldb;
    int M, N, Kd;              // valid output rows, output columns, reduction length
    int a_clamp, b_clamp;      // KC operand: last valid row; other operand: last addressable float4 start column
    int Mp, Np;                // stage 1/3: the padded extent of R that is written (zeros outside M x N); stage 2: Np, the padded columns of H
    int tiles_m, tiles_n;
    const float* bscale;       // stage 1: s, applied to H's rows while staging (nullptr: stage 3)
    const float* V;            // stage 1/3
    long sV;
    float* C;                  // stage 1/3: R   stage 2: H   stage 4: U
    long sC;
    int ldc;
    const float *hscale, *colsumW;      // stage 2
    const float *Gm, *Gp;               // stage 2: [batch][Kp][Np], the pitch and stride of H
    int Kp;                    // per-file stride of the K-vectors
    float alpha, eps, weight;
};

template <int GEMM>
__global__ __launch_bounds__(SMOOTH_NT, 2) void nmf_smooth_gemm_kernel(SmoothGemmArgs p) {
    constexpr int BM = SMOOTH_BM, BN = SMOOTH_BN, BK = SMOOTH_BK, NT = SMOOTH_NT;
    constexpr bool A_KC = GEMM != SMOOTH_GEMM_H, B_KC = GEMM == SMOOTH_GEMM_U;      // W.H | W^T.R | R.H^T
    constexpr int LDA = A_KC ? BK + 1 : BM, LDB = B_KC ? BK + 1 : BN;
    constexpr int SA = A_KC ? BM * LDA : BK * BM, SB = B_KC ? BN * LDB : BK * BN, SBUF = SA + SB;
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

    const float* __restrict__ A = p.A + file * p.sA;
    const float* __restrict__ B = p.B + file * p.sB;
    const float* __restrict__ bsc = (GEMM == SMOOTH_GEMM_P && p.bscale) ? p.bscale + (long)file * p.Kp : nullptr;
    // (stages 1 and 3 also write the zero padding of R: their waves are active up to the padded row count)
    const bool wave_active = (row0 + wm * 32) < (GEMM == SMOOTH_GEMM_P ? p.Mp : p.M);

    f32x16 acc[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;

    int offA[UA], offB[UB];
    gemm_operand_offsets<BM, NT, UA, A_KC>(offA, p.lda, row0, p.a_clamp, tid);
    gemm_operand_offsets<BN, NT, UB, B_KC>(offB, p.ldb, col0, p.b_clamp, tid);
    float4 ra[UA], rb[UB];
    // this thread's reduction indexes inside a k-tile: a KC unit holds ks .. ks + 3 of one row, another unit one index (kna + 8 i | knb) of four rows / columns
    const int ks = 4 * (tid & 3), kna = tid / (BM / 4), knb = tid / (BN / 4);

#define SMOOTH_MASK4(v_, left_)                     \
    do {                                            \
        (v_).x = ks + 0 < (left_) ? (v_).x : 0.f;   \
        (v_).y = ks + 1 < (left_) ? (v_).y : 0.f;   \
        (v_).z = ks + 2 < (left_) ? (v_).z : 0.f;   \
        (v_).w = ks + 3 < (left_) ? (v_).w : 0.f;   \
    } while (0)
    // reduction indexes >= Kd come in as zeros (selected, not multiplied: the padding may hold NaN or Inf)
#define SMOOTH_LOAD_TILE(k0_)                                                                               \
    do {                                                                                                    \
        gemm_load_operand<UA>(ra, A + (A_KC ? (long)(k0_) : (long)(k0_) * p.lda), offA);                    \
        gemm_load_operand<UB>(rb, B + (B_KC ? (long)(k0_) : (long)(k0_) * p.ldb), offB);                    \
        const int left_ = p.Kd - (k0_);                                                                     \
        if (GEMM == SMOOTH_GEMM_P && bsc) {                                                                 \
            const float sc_ = bsc[(k0_) + knb];                                                             \
            rb[0].x *= sc_; rb[0].y *= sc_; rb[0].z *= sc_; rb[0].w *= sc_;                                 \
        }                                                                                                   \
        _Pragma("unroll") for (int i_ = 0; i_ < UA; ++i_) {                                                 \
            if (A_KC) SMOOTH_MASK4(ra[i_], left_);                                                          \
            else if (!(kna + (NT / (BM / 4)) * i_ < left_)) ra[i_] = make_float4(0.f, 0.f, 0.f, 0.f);       \
        }                                                                                                   \
        if (B_KC) SMOOTH_MASK4(rb[0], left_);                                                               \
        else if (!(knb < left_)) rb[0] = make_float4(0.f, 0.f, 0.f, 0.f);                                   \
    } while (0)
#define SMOOTH_STORE_TILE(buf_)                                                                             \
    do {                                                                                                    \
        float* sbuf_ = smem + (buf_) * SBUF;                                                                \
        gemm_store_operand<BM, NT, UA, A_KC, LDA>(ra, sbuf_, tid);                                          \
        gemm_store_operand<BN, NT, UB, B_KC, LDB>(rb, sbuf_ + SA, tid);                                     \
    } while (0)

    // the k loop of nmf_beta.hip: tile kt from buffer kt & 1, tile kt + 1 on its way into the other one, tile kt + 2 into registers
    const int nkt = (p.Kd + BK - 1) / BK;
    SMOOTH_LOAD_TILE(0);
    SMOOTH_STORE_TILE(0);
    if (nkt > 1) SMOOTH_LOAD_TILE(BK);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nkt) SMOOTH_STORE_TILE(cur ^ 1);
        if (kt + 2 < nkt) SMOOTH_LOAD_TILE((kt + 2) * BK);
        const float* __restrict__ sA = smem + cur * SBUF;
        const float* __restrict__ sB = sA + SA;
        if (wave_active) {
#pragma unroll
            for (int pp = 0; pp < BK / 2; ++pp) {
                const int kk = 2 * pp + hh;      // lane (l31, hh) supplies A[i = l31][k = hh] and B[k = hh][j = l31] of the k-pair
                const float a = A_KC ? sA[arow * LDA + kk] : sA[kk * BM + arow];
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const float b = B_KC ? sB[(bcol + n * 32) * LDB + kk] : sB[kk * BN + bcol + n * 32];
                    acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[n], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
#undef SMOOTH_LOAD_TILE
#undef SMOOTH_STORE_TILE
#undef SMOOTH_MASK4

    // ---- epilogue: MFMA C/D layout col = lane & 31 (+ 32), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) -----------------------------
    if (!wave_active) return;
    const int row_base = row0 + wm * 32 + 4 * hh;
    const int col_a = col0 + l31, col_b = col_a + 32;
    const bool ok_a = col_a < p.N, ok_b = col_b < p.N;
    const int ca = min(col_a, p.N - 1), cb = min(col_b, p.N - 1);
    if (GEMM == SMOOTH_GEMM_P) {
        const float* __restrict__ V = p.V + file * p.sV;
        float* __restrict__ R = p.C + file * p.sC;
        float va[16], vb[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {          // every load up front, from clamped (valid) addresses
            const long ro = (long)min(row_base + (r & 3) + 8 * (r >> 2), p.M - 1) * p.ldc;
            va[r] = V[ro + ca];
            vb[r] = V[ro + cb];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row_base + (r & 3) + 8 * (r >> 2);
            const bool in = row < p.M;
            if (row < p.Mp) {
                const long ro = (long)row * p.ldc;
                if (col_a < p.Np) R[ro + col_a] = (in && ok_a) ? va[r] / acc[0][r] : 0.f;
                if (col_b < p.Np) R[ro + col_b] = (in && ok_b) ? vb[r] / acc[1][r] : 0.f;
            }
        }
    } else if (GEMM == SMOOTH_GEMM_H) {
        float* H = p.C + file * p.sC;           // read-modify-write of this workgroup's own elements: all reads first
        const float* __restrict__ Gm = p.Gm + file * p.sC;
        const float* __restrict__ Gp = p.Gp + file * p.sC;
        const float* __restrict__ hs = p.hscale + (long)file * p.Kp;
        const float* __restrict__ cw = p.colsumW + (long)file * p.Kp;
        float ua[16], ub[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rc = min(row_base + (r & 3) + 8 * (r >> 2), p.M - 1);
            const long ia = (long)rc * p.ldc + ca, ib = (long)rc * p.ldc + cb;
            const float sc = hs[rc], base = __fadd_rn(cw[rc], p.alpha);
            const float na = __fadd_rn(acc[0][r], __fmul_rn(p.weight, Gm[ia])), nb = __fadd_rn(acc[1][r], __fmul_rn(p.weight, Gm[ib]));
            const float da = __fadd_rn(__fadd_rn(base, __fmul_rn(p.weight, Gp[ia])), p.eps);
            const float db = __fadd_rn(__fadd_rn(base, __fmul_rn(p.weight, Gp[ib])), p.eps);
            ua[r] = __fmul_rn(__fmul_rn(H[ia], sc), __fdiv_rn(na, da));
            ub[r] = __fmul_rn(__fmul_rn(H[ib], sc), __fdiv_rn(nb, db));
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row_base + (r & 3) + 8 * (r >> 2);
            if (row < p.M) {                    // (col_b < Np whenever col_a is: Np is a multiple of 64)
                if (col_a < p.Np) H[(long)row * p.ldc + col_a] = ok_a ? ua[r] : 0.f;
                if (col_b < p.Np) H[(long)row * p.ldc + col_b] = ok_b ? ub[r] : 0.f;
            }
        }
    } else {
        float* __restrict__ U = p.C + file * p.sC;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row_base + (r & 3) + 8 * (r >> 2);
            if (row < p.M) {
                if (ok_a) U[(long)row * p.ldc + col_a] = acc[0][r];
                if (ok_b) U[(long)row * p.ldc + col_b] = acc[1][r];
            }
        }
    }
}

static __device__ __forceinline__ double smooth_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// Stage 2, launch A.  grid = ceil(batch * K * segments / 4) workgroups of four waves, a wave per (file, atom, segment) row.  E, D
// [batch][2][Kp] (segment-major inside a file; the second plane is not written when segments = 1), Gm, Gp [batch][Kp][Np].
__global__ __launch_bounds__(256) void nmf_smooth_terms_kernel(const float* __restrict__ H, const float* __restrict__ hscale, float* __restrict__ Gm,
                                                               float* __restrict__ Gp, float* __restrict__ E, float* __restrict__ D, int T,
                                                               int K, int Kp, int Np, int segments, long rows) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                    // (whole waves: no barrier follows)
    const int lane = threadIdx.x & 63;
    const int seg = (int)(row % segments);
    const long fk = row / segments;
    const int k = (int)(fk % K);
    const long file = fk / K;
    const long at = (file * Kp + k) * (long)Np + (long)seg * T;
    const float* __restrict__ h = H + at;
    const double s = (double)hscale[file * Kp + k];
    double e = 0.0, d = 0.0;
    for (int t = lane; t < T; t += 64) {
        const double x = s * (double)h[t];
        e += x * x;
        if (t > 0) {
            const double dx = x - s * (double)h[t - 1];
            d += dx * dx;
        }
    }
    e = smooth_wave_sum(e);
    d = smooth_wave_sum(d);
    if (lane == 0) {
        E[(file * 2 + seg) * Kp + k] = (float)e;
        D[(file * 2 + seg) * Kp + k] = (float)d;
    }
    const double c = e > 0.0 ? 2.0 * (double)T / e : 0.0, doe = e > 0.0 ? d / e : 0.0;
    for (int t = lane; t < T; t += 64) {
        const double x = s * (double)h[t];
        const double left = t > 0 ? s * (double)h[t - 1] : 0.0, right = t + 1 < T ? s * (double)h[t + 1] : 0.0;
        const int nb = (t > 0) + (t + 1 < T);
        Gp[at + t] = (float)(c * ((double)nb * x));
        Gm[at + t] = (float)(c * (left + right) + c * (x * doe));
    }
}

// Stage 4's rowsumH = sum_{n < N} H: a wave per (file, atom) row, float32.
__global__ __launch_bounds__(256) void nmf_smooth_rowsum_kernel(const float* __restrict__ H, float* __restrict__ rowsumH, int N, int K, int Kp,
                                                                int Np, long rows) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int k = (int)(row % K);
    const long file = row / K;
    const float* __restrict__ h = H + (file * Kp + k) * (long)Np;
    float v = 0.f;
    for (int n = lane; n < N; n += 64) v += h[n];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if (lane == 0) rowsumH[file * Kp + k] = v;
}

// The envelope of the temporal-continuity call: that of the IS / Euclidean call, and at most 65535 files (the weight rides in the upper
// halves of K and batch).
bool gccnmf_klnmf_smooth_supported(int F, int K, int batch) { return F >= 2 && F <= 2049 && K >= 1 && K <= 1024 && batch <= 65535; }

// Stages 1-4 of the temporal-continuity iteration.  V, R [batch][Fp][Np], W, U [batch][Fp][Kp], H, Gm, Gp [batch][Kp][Np], colsumW, rowsumH,
// hscale [batch][Kp], E, D [batch][2][Kp]; Np = round_up(N, 64); N = segments * T.
int gccnmf_klnmf_smooth_stage_launch(int stage, const float* V, const float* W, float* H, float* R, float* U, float* rowsumH, const float* colsumW,
                                     const float* hscale, float* Gm, float* Gp, float* E, float* D, int F, int N, int K, int batch, int segments,
                                     float alpha, float eps, float weight, hipStream_t s) {
    if (!gccnmf_klnmf_smooth_supported(F, K, batch) || N < 1 || batch < 1) return GCCNMF_ERR_UNSUPPORTED;
    if ((segments != 1 && segments != 2) || N % segments) return GCCNMF_ERR_ARG;
    const GccNmfPitches pt = gccnmf_make_pitches(F, 1, K);
    const int Fp = pt.Fp, Kp = pt.Kp, Np = gccnmf_round_up(N, 64);
    const long sV = (long)Fp * Np, sW = (long)Fp * Kp, sH = (long)Kp * Np;
    SmoothGemmArgs a = {};
    a.Kp = Kp; a.alpha = alpha; a.eps = eps; a.weight = weight;
    long tiles = 0;
    switch (stage) {
        case 1:
        case 3:
            a.A = W; a.sA = sW; a.lda = Kp; a.a_clamp = F - 1;
            a.B = H; a.sB = sH; a.ldb = Np; a.b_clamp = Np - 4;
            a.M = F; a.N = N; a.Kd = K; a.Mp = Fp; a.Np = Np;
            a.bscale = stage == 1 ? hscale : nullptr;
            a.V = V; a.sV = sV;
            a.C = R; a.sC = sV; a.ldc = Np;
            a.tiles_m = gccnmf_ceil_div(Fp, SMOOTH_BM); a.tiles_n = Np / SMOOTH_BN;
            tiles = (long)a.tiles_m * a.tiles_n * batch;
            if (tiles > 0x7fffffffL) return GCCNMF_ERR_UNSUPPORTED;
            hipLaunchKernelGGL(nmf_smooth_gemm_kernel<SMOOTH_GEMM_P>, dim3((unsigned)tiles), dim3(SMOOTH_NT), 0, s, a);
            break;
        case 2: {
            const long rows = (long)batch * K * segments;
            a.A = W; a.sA = sW; a.lda = Kp; a.a_clamp = Kp - 4;
            a.B = R; a.sB = sV; a.ldb = Np; a.b_clamp = Np - 4;
            a.M = K; a.N = N; a.Kd = F; a.Np = Np;
            a.C = H; a.sC = sH; a.ldc = Np;
            a.hscale = hscale; a.colsumW = colsumW; a.Gm = Gm; a.Gp = Gp;
            a.tiles_m = gccnmf_ceil_div(K, SMOOTH_BM); a.tiles_n = Np / SMOOTH_BN;
            tiles = (long)a.tiles_m * a.tiles_n * batch;
            if (tiles > 0x7fffffffL) return GCCNMF_ERR_UNSUPPORTED;
            hipLaunchKernelGGL(nmf_smooth_terms_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, H, hscale, Gm, Gp, E, D, N / segments, K, Kp,
                               Np, segments, rows);
            GCCNMF_CHECK_LAUNCH();
            hipLaunchKernelGGL(nmf_smooth_gemm_kernel<SMOOTH_GEMM_H>, dim3((unsigned)tiles), dim3(SMOOTH_NT), 0, s, a);
            break;
        }
        case 4: {
            const long rows = (long)batch * K;
            a.A = R; a.sA = sV; a.lda = Np; a.a_clamp = F - 1;
            a.B = H; a.sB = sH; a.ldb = Np; a.b_clamp = K - 1;
            a.M = F; a.N = K; a.Kd = N;
            a.C = U; a.sC = sW; a.ldc = Kp;
            a.tiles_m = gccnmf_ceil_div(F, SMOOTH_BM); a.tiles_n = gccnmf_ceil_div(K, SMOOTH_BN);
            tiles = (long)a.tiles_m * a.tiles_n * batch;
            if (tiles > 0x7fffffffL) return GCCNMF_ERR_UNSUPPORTED;
            hipLaunchKernelGGL(nmf_smooth_gemm_kernel<SMOOTH_GEMM_U>, dim3((unsigned)tiles), dim3(SMOOTH_NT), 0, s, a);
            GCCNMF_CHECK_LAUNCH();
            hipLaunchKernelGGL(nmf_smooth_rowsum_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, H, rowsumH, N, K, Kp, Np, rows);
            break;
        }
        default: return GCCNMF_ERR_ARG;
    }
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}
