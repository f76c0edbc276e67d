// Semi-supervised KL-NMF (gccnmf_klnmf / gccnmf_klnmf_stage with GCCNMF_FLAG_FREE_ATOMS(n)): the W half of the iteration for the n FREE
// atoms that sit beside a pre-trained dictionary -- the last n columns of every file's W.  Stages 0-3, 6 and 7 are the blind call's; this
// file is its stage 4 and stage 5 restricted to those columns (gccNMFFunctions.py:77, :79-81 on W[:, K - n:] and H[K - n:, :]):
//
//   stage 4   U[f][K - n + j] = sum_c R[f][c] * H[K - n + j][c],   rowsumH[K - n + j] = sum_c H[K - n + j][c]          j < n
//   stage 5   Wt = W * (U / rowsumH),  s = sqrt(sum_f Wt^2),  W = Wt / s,  hscale = s,  colsumW = sum_f W            the n free columns
//
// Nothing of the fixed atoms is written: their columns of W and U, their rowsumH, hscale (1) and colsumW (stage 0's) keep their bits.
//
// Stage 4 reads R [F][N] once and does n / K of the blind GEMM's work: it is bound by the bytes of R, not by the matrix cores.
//   * A workgroup owns one band of 32 bins of one file and keeps the whole 32 x n block of U in accumulators (NB = ceil(n / 32) blocks of
//     v_mfma_f32_32x32x2_f32): R is read once however many free atoms there are.
//   * Its four waves split the COLUMNS: wave w takes the 32-column chunks w, w + 4, w + 8, ...  One file alone has only ceil(F / 32)
//     bands, so the parallelism inside a band comes from the reduction; the grid is batch x bands whatever the batch.
//   * Both operands are contiguous along the reduction index.  A chunk of R is 32 rows x 128 bytes, of H_free 32 NB rows x 128 bytes: a
//     wave fetches them as whole 128-byte lines (float4 per lane, 8 rows per instruction) into registers -- the NEXT chunk's, while the
//     matrix cores work on the current one -- and passes them through a wave-private LDS tile (R's 32 rows and one 32-atom block of H_free
//     at a time; row pitch 36 floats: the ds_read_b128 of 16 lanes on 16 different rows hit 16 different bank quads) to reach the MFMA
//     operand layout: lane (i, h) reads the float4s at columns
//     16 h + 4 q of row i, and MFMA (q, e) reduces over the columns 4 q + e (h = 0) and 16 + 4 q + e (h = 1) -- the same permutation of
//     the chunk's columns for both operands.
//   * The four partial blocks meet in LDS and are added in wave order 0, 1, 2, 3.
// The order of every sum is fixed by (F, N, K, n): no atomics, and a file's U_free, W, hscale and colsumW are bit for bit the same alone
// and in any batch.  Rows >= F and atoms >= n of a tile re-read the last valid row (always in bounds) and are never stored: a row of A
// reaches only its own row of the product, a row of H only its own column.  Columns >= N inside the last chunk are the zero padding of R
// and H.
#include "common.h"
#include "../../include/gccnmf_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));        // (a native vector: the staging arrays below stay in registers)

#define SEMI_PITCH 36                      // floats per row of an LDS tile (32 columns + 4: 144 bytes, 16-byte aligned)
#define SEMI_WAVES 4

// row of register r of lane half h inside a 32-row block: the f32 32x32 D layout
__device__ __forceinline__ int semi_d_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

template <int NB>
__global__ __launch_bounds__(64 * SEMI_WAVES) void nmf_semi_rht_kernel(const float* __restrict__ R, const float* __restrict__ H,
                                                                      float* __restrict__ U, float* __restrict__ rowsumH, int F, int N,
                                                                      int Fp, int Kp, int Np, int kf, int nf, int bands) {
    // tile rows of one wave: R's 32, then ONE 32-atom block of H_free at a time (37 KB per workgroup whatever n: four workgroups per CU)
    __shared__ __attribute__((aligned(16))) float tile[SEMI_WAVES][64 * SEMI_PITCH];
    __shared__ float rsum[SEMI_WAVES][32 * NB];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int file = blockIdx.x / bands, band = blockIdx.x - file * bands;
    const int f0 = band * 32;
    const float* Rf = R + (long)file * Fp * Np;
    const float* Hf = H + (long)file * Kp * Np;
    float* my = tile[wave];

    // global -> register staging: instruction p of a 32-row block moves rows 8 p + lane / 8, f32x4 lane % 8 (one 128-byte line per row)
    const int lr = lane >> 3, lc = (lane & 7) * 4;
    int rowR[4], rowH[NB][4];
#pragma unroll
    for (int p = 0; p < 4; ++p) rowR[p] = min(f0 + 8 * p + lr, F - 1);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int p = 0; p < 4; ++p) rowH[b][p] = kf + min(32 * b + 8 * p + lr, nf - 1);

    f32x16 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
    float hs[NB];                                                             // band 0 alone: this lane's share of rowsumH
#pragma unroll
    for (int b = 0; b < NB; ++b) hs[b] = 0.f;

    const int chunks = (N + 31) >> 5;
    // (macros, not lambdas: staging arrays captured by reference would live in scratch memory instead of registers)
    f32x4 gr[4], gh[NB][4];
#define SEMI_FETCH_R(chunk)                                                                     \
    {                                                                                           \
        const int n0_ = (chunk) * 32 + lc;                                                      \
        _Pragma("unroll") for (int p = 0; p < 4; ++p) gr[p] = *(const f32x4*)(Rf + (long)rowR[p] * Np + n0_); \
    }
#define SEMI_FETCH_H(chunk)                                                                     \
    {                                                                                           \
        const int n0_ = (chunk) * 32 + lc;                                                      \
        _Pragma("unroll") for (int b = 0; b < NB; ++b)                                          \
            _Pragma("unroll") for (int p = 0; p < 4; ++p) gh[b][p] = *(const f32x4*)(Hf + (long)rowH[b][p] * Np + n0_); \
    }
    // the tile is this wave's alone and a wave's LDS operations execute in order: no workgroup barrier inside the loop
#define wave_sync()                                             \
    {                                                           \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
        __builtin_amdgcn_wave_barrier();                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
    }
    // Every fetch is unconditional -- behind a wave's last chunk it re-reads that chunk (in bounds, never used): a conditional one would
    // make the staging registers loop-carried copies, and the copies wait for the loads where they are issued.
    SEMI_FETCH_R(min(wave, chunks - 1));
    SEMI_FETCH_H(min(wave, chunks - 1));
    for (int ch = wave; ch < chunks; ch += SEMI_WAVES) {
        const int next = min(ch + SEMI_WAVES, chunks - 1);
#pragma unroll
        for (int p = 0; p < 4; ++p) *(f32x4*)(my + (8 * p + lr) * SEMI_PITCH + lc) = gr[p];
#pragma unroll
        for (int p = 0; p < 4; ++p) *(f32x4*)(my + (32 + 8 * p + lr) * SEMI_PITCH + lc) = gh[0][p];
        wave_sync();
        SEMI_FETCH_R(next);                                                   // the next chunk is in flight while this one feeds the matrix cores
        __builtin_amdgcn_sched_barrier(0);                                    // (issued here, not sunk behind the MFMAs)
        f32x4 a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = *(const f32x4*)(my + c * SEMI_PITCH + 16 * h + 4 * q);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            f32x4 bb[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) bb[q] = *(const f32x4*)(my + (32 + c) * SEMI_PITCH + 16 * h + 4 * q);
            wave_sync();                                                      // every lane has read the block before the next one overwrites it
            if (b + 1 < NB) {
#pragma unroll
                for (int p = 0; p < 4; ++p) *(f32x4*)(my + (32 + 8 * p + lr) * SEMI_PITCH + lc) = gh[b + 1 < NB ? b + 1 : b][p]  /* (the index stays inside the array where the branch is dead) */;
                wave_sync();
            } else {
                SEMI_FETCH_H(next);                                           // (every block of this chunk has left the registers)
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, bb[q].x, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, bb[q].y, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, bb[q].z, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, bb[q].w, acc[b], 0, 0, 0);
            }
            if (band == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) hs[b] += (bb[q].x + bb[q].y) + (bb[q].z + bb[q].w);
            }
        }
    }

    // the waves' partial blocks meet in LDS, one 32-atom block at a time (16 x 64 floats of each wave's tile), added in wave order
    if (band == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float t = hs[b] + __shfl_xor(hs[b], 32);
            if (h == 0) rsum[wave][32 * b + c] = t;
        }
    }
    float* Uf = U + (long)file * Fp * Kp + kf;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int r = 0; r < 16; ++r) my[r * 64 + lane] = acc[b][r];
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int r = 4 * wave + rr;                                      // wave w adds and stores registers 4 w .. 4 w + 3
            const int at = r * 64 + lane;
            const float u = ((tile[0][at] + tile[1][at]) + tile[2][at]) + tile[3][at];
            const int f = f0 + semi_d_row(r, h), j = 32 * b + c;
            if (f < F && j < nf) Uf[(long)f * Kp + j] = u;
        }
        __syncthreads();
    }
    if (band == 0 && (int)threadIdx.x < nf) {                                 // (nf <= 32 NB <= 128 < 256 threads)
        const int j = threadIdx.x;
        rowsumH[(long)file * Kp + kf + j] = ((rsum[0][j] + rsum[1][j]) + rsum[2][j]) + rsum[3][j];
    }
}

// Stage 5 for the free columns: the arithmetic of update_w.h / nmf_update_w_kernel (w * (u / rowsum), an fmaf sum of squares, sqrtf, the
// division by the norm, the column sum of the normalised atom), any F.  grid = batch x ceil(n / 8), 256 threads = 8 atoms x 32 row phases;
// W and U are read twice (L2-resident: 32-byte row segments of a few kilobytes per atom group).  A free atom whose H row sums to 0 takes
// the path the blind stage 5 takes (u / 0).  The groups start at kf, a multiple of 16, so a group never straddles the fixed block.
#define SEMI_AT 8
__global__ __launch_bounds__(256) void nmf_semi_update_w_kernel(float* __restrict__ W, const float* __restrict__ U,
                                                                const float* __restrict__ rowsumH, float* __restrict__ colsumW,
                                                                float* __restrict__ hscale, int F, int Fp, int Kp, int kf, int nf, int chunks) {
    constexpr int PH = 256 / SEMI_AT;
    __shared__ float red[256];
    __shared__ float s_norm[SEMI_AT];
    const int b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;
    const int c = threadIdx.x % SEMI_AT, q = threadIdx.x / SEMI_AT;
    const int j = ch * SEMI_AT + c;
    const bool valid = j < nf;
    const int k = kf + (valid ? j : nf - 1);
    float* Wb = W + (long)b * Fp * Kp;
    const float* Ub = U + (long)b * Fp * Kp;
    const float rs = rowsumH[(long)b * Kp + k];
    float ss = 0.f;
    if (valid)
#pragma unroll 4
        for (int f = q; f < F; f += PH) {
            const long i = (long)f * Kp + k;
            const float wt = Wb[i] * (Ub[i] / rs);
            ss = fmaf(wt, wt, ss);
        }
    red[threadIdx.x] = ss;
    __syncthreads();
    if (q == 0) {
        float t = 0.f;
#pragma unroll
        for (int p = 0; p < PH; ++p) t += red[c + SEMI_AT * p];
        s_norm[c] = sqrtf(t);
    }
    __syncthreads();
    const float norm = s_norm[c];
    float cs = 0.f;
    if (valid)
#pragma unroll 4
        for (int f = q; f < F; f += PH) {
            const long i = (long)f * Kp + k;
            const float wn = (Wb[i] * (Ub[i] / rs)) / norm;
            Wb[i] = wn;
            cs += wn;
        }
    red[threadIdx.x] = cs;
    __syncthreads();
    if (q == 0 && valid) {
        float t = 0.f;
#pragma unroll
        for (int p = 0; p < PH; ++p) t += red[c + SEMI_AT * p];
        colsumW[(long)b * Kp + k] = t;
        hscale[(long)b * Kp + k] = norm;
    }
}

// The envelope of the semi-supervised call (gccnmf_klnmf states the argument rules in front of it): the free block starts on a float4 /
// atom-group boundary, and the shapes are the fixed-dictionary call's.
bool gccnmf_klnmf_semi_supported(int F, int K, int nfree) { return F >= 2 && F <= 2049 && K <= 1024 && nfree >= 1 && nfree <= 128 && nfree < K && ((K - nfree) & 15) == 0; }

// R [batch][Fp][Np] (zero outside F x N), H [batch][Kp][Np] -> U[:, kf : kf + nf], rowsumH[kf : kf + nf] of every file
int gccnmf_klnmf_semi_rht_launch(const float* R, const float* H, float* U, float* rowsumH, int F, int N, int K, int nfree, int batch, hipStream_t s) {
    if (!gccnmf_klnmf_semi_supported(F, K, nfree) || N < 1 || batch < 1) return GCCNMF_ERR_UNSUPPORTED;
    const GccNmfPitches p = gccnmf_make_pitches(F, 1, K);
    const int Np = gccnmf_round_up(N, 64), bands = gccnmf_ceil_div(F, 32), kf = K - nfree;
    const dim3 grid((unsigned)batch * bands), block(64 * SEMI_WAVES);
    switch (gccnmf_ceil_div(nfree, 32)) {
        case 1: hipLaunchKernelGGL(nmf_semi_rht_kernel<1>, grid, block, 0, s, R, H, U, rowsumH, F, N, p.Fp, p.Kp, Np, kf, nfree, bands); break;
        case 2: hipLaunchKernelGGL(nmf_semi_rht_kernel<2>, grid, block, 0, s, R, H, U, rowsumH, F, N, p.Fp, p.Kp, Np, kf, nfree, bands); break;
        case 3: hipLaunchKernelGGL(nmf_semi_rht_kernel<3>, grid, block, 0, s, R, H, U, rowsumH, F, N, p.Fp, p.Kp, Np, kf, nfree, bands); break;
        case 4: hipLaunchKernelGGL(nmf_semi_rht_kernel<4>, grid, block, 0, s, R, H, U, rowsumH, F, N, p.Fp, p.Kp, Np, kf, nfree, bands); break;
        default: return GCCNMF_ERR_UNSUPPORTED;
    }
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

int gccnmf_klnmf_semi_update_w_launch(float* W, const float* U, const float* rowsumH, float* colsumW, float* hscale, int F, int K, int nfree,
                                      int batch, hipStream_t s) {
    if (!gccnmf_klnmf_semi_supported(F, K, nfree) || batch < 1) return GCCNMF_ERR_UNSUPPORTED;
    const GccNmfPitches p = gccnmf_make_pitches(F, 1, K);
    const int chunks = gccnmf_ceil_div(nfree, SEMI_AT);
    hipLaunchKernelGGL(nmf_semi_update_w_kernel, dim3((unsigned)batch * chunks), dim3(256), 0, s, W, U, rowsumH, colsumW, hscale, F, p.Fp, p.Kp,
                       K - nfree, nfree, chunks);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}
