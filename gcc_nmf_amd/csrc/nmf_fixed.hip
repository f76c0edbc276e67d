// KL-NMF coefficients against a FIXED dictionary (gccnmf_klnmf with GCCNMF_FLAG_FIXED_W): every iteration of the call in ONE launch.
//
//   h <- h o (W^T (v / (W h))) / (colsum W + alpha + eps)        per column, W constant (gccNMFFunctions.py:76 without :77-81)
//
// With W fixed every column of H is independent, so a workgroup owns 32 columns of one file and keeps them in registers from the first
// iteration to the last: no hand-over between workgroups of any kind (no counters, no atomics, no grid barrier).
//
// Work of one workgroup (nw waves, 1 <= nw <= 8): the atoms are cut in 32-atom blocks, wave w owns KB consecutive blocks and keeps H and
// the U = W^T R accumulator of those atoms in registers.  Per iteration it walks F in chunks of 32 rows:
//   1. P = W.H   over its own atoms (v_mfma_f32_32x32x2_f32, A = Wt[k][f] from the transposed copy, B = the H registers);
//      the partial P of the waves meet in LDS and every wave adds them in wave order 0, 1, ... (deterministic, identical in every wave)
//   2. R = V / P (the IEEE quotient), 0 outside the file's F x N
//   3. U += W^T.R over the chunk's 32 rows: R is the B operand straight from the accumulator registers.  The 32x32 f32 D layout
//      (col = lane&31, row = (reg&3) + 8(reg>>2) + 4(lane>>5)) is a B layout whose reduction index of MFMA j is that row, so the A
//      fragment W[f][k] is read with the same f permutation -- coalesced from the dictionary itself ([Fp][Kp], k on the lane).
// and then updates H <- H * (U / den).  The H registers use the same permuted k order as the U accumulator, which is also the k order of
// step 1's B operand: H, U and step 1's fragments all pair up register for register.
//
// A file's columns see the same instructions whatever batch they ride in (the shape depends on F and K only): bitwise batch independence.
#include "common.h"
#include "../../include/gccnmf_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define FIXED_MAX_WAVES 8

// den[k] = (colsum W[:, k] + alpha) + eps (numpy's left-to-right order; the column sum in f order); Wt [Kp][Fq] = W^T with Fq = round_up(F, 32),
// zero outside F x K (a chunk of 32 rows never reads past its row).  One workgroup per 32 atoms, 32 x 8 threads.
__global__ __launch_bounds__(256) void nmf_fixed_prepare_kernel(const float* __restrict__ W, float* __restrict__ Wt, float* __restrict__ den,
                                                                int F, int K, int Fq, int Kp, float alpha, float eps) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int k0 = blockIdx.x * 32;
    float sum = 0.f;
    for (int f0 = 0; f0 < Fq; f0 += 32) {
        for (int r = ty; r < 32; r += 8) {
            const int f = f0 + r, k = k0 + tx;
            tile[r][tx] = (f < F && k < K) ? W[(long)f * Kp + k] : 0.f;
        }
        __syncthreads();
        if (ty == 0)
            for (int r = 0; r < 32; ++r) sum += tile[r][tx];      // rows f >= F hold 0: the sum is over f < F in f order
        for (int r = ty; r < 32; r += 8) {
            const int k = k0 + r, f = f0 + tx;
            Wt[(long)k * Fq + f] = tile[tx][r];
        }
        __syncthreads();
    }
    if (ty == 0) den[k0 + tx] = (k0 + tx < K) ? (sum + alpha) + eps : 1.f;
}

// k (or f) of register r of lane half h inside a 32-row block: the f32 32x32 D layout
__device__ __forceinline__ int d_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Operand loads are buffer loads: a wave-uniform descriptor, one per-lane byte offset and the per-register part as a scalar offset -- no
// per-load 64-bit address arithmetic, and nothing for the compiler to hoist out of the iteration loop into live registers.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t fixed_rsrc(const float* base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
// a lane value the compiler may not hoist out of the loops (derived offsets are formed where they are used, not kept live)
__device__ __forceinline__ int opaque(int x) {
    __asm__ volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ float bload(__amdgpu_buffer_rsrc_t r, unsigned v, unsigned s) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, v, s, 0));
}

// Set s of a chunk's operand stream into dst: s < KB -> Wt rows 32 (kb0 + s) + d_row(j, h), columns f0 + c (A of P = W.H; Wt is zero
// outside F x K, so no test); s >= KB -> W rows f0 + d_row(j, h), columns 32 (kb0 + s - KB) + c (A of U = W^T.R).  Rows f >= F of W
// are read as row F - 1 (inside the dictionary): R is 0 there, so they add nothing.  Blocks >= nblk are not read.
template <int KB>
__device__ __forceinline__ void load_set(int s, int f0, float* dst, __amdgpu_buffer_rsrc_t rW, __amdgpu_buffer_rsrc_t rWt, int F, int Fq,
                                         int Kp, int kb0, int nblk, int h, int c) {
    if (s < KB) {
        if (s >= nblk) return;
        const unsigned vo = (unsigned)(4 * h * Fq + c) * 4u;
#pragma unroll
        for (int j = 0; j < 16; ++j) dst[j] = bload(rWt, vo, (unsigned)((32 * (kb0 + s) + d_row(j, 0)) * Fq + f0) * 4u);
    } else {
        if (s - KB >= nblk) return;
        const unsigned col = (unsigned)(32 * (kb0 + s - KB) + c) * 4u;
        const int fh = opaque(f0 + 4 * h);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int f = min(fh + d_row(j, 0), F - 1);
            dst[j] = bload(rW, (unsigned)(f * Kp) * 4u + col, 0u);
        }
    }
}

// V rows f0 + d_row(r, h) of this lane's column (rows f >= F read as row F - 1: R is 0 there)
__device__ __forceinline__ void load_v(float* v, __amdgpu_buffer_rsrc_t rV, int f0, int F, int Np, int n, int h) {
    const int fh = opaque(f0 + 4 * h);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int f = min(fh + d_row(r, 0), F - 1);
        v[r] = bload(rV, (unsigned)(f * Np + n) * 4u, 0u);
    }
}

template <int KB>
__global__ __launch_bounds__(64 * FIXED_MAX_WAVES) void nmf_fixed_kernel(const float* __restrict__ V, const float* __restrict__ W,
                                                                         const float* __restrict__ Wt, const float* __restrict__ den,
                                                                         float* __restrict__ H, int F, int N, int K, int Fp, int Fq, int Kp, int Np,
                                                                         int Kb, int iterations, int ones) {
    __shared__ float part[2][FIXED_MAX_WAVES][16][64];       // partial P of every wave, double buffered (one barrier per chunk)
    const int nw = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int tiles = Np >> 5;
    const int file = blockIdx.x / tiles, n0 = (blockIdx.x - file * tiles) * 32;
    float* Hf = H + (long)file * Kp * Np + n0;
    if (n0 >= N) {                                            // a padding tile: its columns of H are zero
        for (int i = threadIdx.x; i < Kp * 32; i += blockDim.x) Hf[(long)(i >> 5) * Np + (i & 31)] = 0.f;
        return;
    }
    const __amdgpu_buffer_rsrc_t rV = fixed_rsrc(V + (long)file * Fp * Np, (unsigned)(Fp * Np) * 4u);
    const __amdgpu_buffer_rsrc_t rW = fixed_rsrc(W, (unsigned)(Fp * Kp) * 4u);
    const __amdgpu_buffer_rsrc_t rWt = fixed_rsrc(Wt, (unsigned)(Kp * Fq) * 4u);
    const __amdgpu_buffer_rsrc_t rD = fixed_rsrc(den, (unsigned)Kp * 4u);
    const bool nvalid = n0 + c < N;
    const int kb0 = wave * KB;
    const int nblk = min(KB, Kb - kb0);                       // >= 1: nw = ceil(Kb / KB)

    float hr[KB][16];
#pragma unroll
    for (int b = 0; b < KB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = 32 * (kb0 + b) + d_row(r, h);
            const bool ok = b < nblk && k < K && nvalid;
            hr[b][r] = ok ? (ones ? 1.f : Hf[(long)k * Np + c]) : 0.f;
        }

    // The operand stream of one chunk: 2 KB sets of 16 A fragments -- set s < KB is step 1's Wt block s, set KB + b step 3's W block b.
    // Set s + 1 (or the next chunk's set 0) is loaded while set s feeds the matrix cores; the compiler barrier keeps the loads in that
    // order (hoisted all at once they would need more registers than the register file holds).
    // At KB = 4 the registers hold no prefetch (H and U of 128 atoms take half of them): set s and the chunk's V are loaded where they
    // are used, and the other wave of the SIMD covers the latency.
    constexpr bool PF = KB < 4;
    const int chunks = (F + 31) >> 5;
    float frag[2][16], v[16];
    if (PF) {
        load_set<KB>(0, 0, frag[0], rW, rWt, F, Fq, Kp, kb0, nblk, h, c);
        load_v(v, rV, 0, F, Np, n0 + c, h);
    }
    int buf = 0;
    for (int it = 0; it < iterations; ++it) {
        f32x16 u[KB];
#pragma unroll
        for (int b = 0; b < KB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) u[b][r] = 0.f;
        for (int ch = 0; ch < chunks; ++ch) {
            const int f0 = ch * 32;
            const int f1 = ch + 1 < chunks ? f0 + 32 : 0;               // the next chunk: this iteration's or the next one's first
            f32x16 p;
            float rr[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) p[r] = 0.f;
#pragma unroll
            for (int s = 0; s < 2 * KB; ++s) {
                if (PF) load_set<KB>(s + 1 < 2 * KB ? s + 1 : 0, s + 1 < 2 * KB ? f0 : f1, frag[(s + 1) & 1], rW, rWt, F, Fq, Kp, kb0, nblk, h, c);
                else load_set<KB>(s, f0, frag[s & 1], rW, rWt, F, Fq, Kp, kb0, nblk, h, c);
                __asm__ volatile("" ::: "memory");
                const float* a = frag[s & 1];
                if (s < KB) {                                        // 1. partial P = W.H over this wave's atoms
                    if (s < nblk)
#pragma unroll
                        for (int j = 0; j < 16; ++j) p = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], hr[s][j], p, 0, 0, 0);
                    if (s == KB - 1) {
                        // the waves' partials, added in wave order
#pragma unroll
                        for (int r = 0; r < 16; ++r) part[buf][wave][r][lane] = p[r];
                        if (!PF) load_v(v, rV, f0, F, Np, n0 + c, h);
                        __syncthreads();
#pragma unroll
                        for (int r = 0; r < 16; ++r) rr[r] = part[buf][0][r][lane];
                        for (int w = 1; w < nw; ++w)
#pragma unroll
                            for (int r = 0; r < 16; ++r) rr[r] += part[buf][w][r][lane];
                        const int fl = nvalid ? opaque(F - f0 - 4 * h) : 0;          // rows of this lane half left in the file
#pragma unroll
                        for (int r = 0; r < 16; ++r) rr[r] = d_row(r, 0) < fl ? v[r] / rr[r] : 0.f;      // 2. R = V / P
                        buf ^= 1;
                        if (PF) load_v(v, rV, f1, F, Np, n0 + c, h);
                    }
                } else if (s - KB < nblk) {                          // 3. U += W^T.R: MFMA j sums over rows f0 + d_row(j, h)
#pragma unroll
                    for (int j = 0; j < 16; ++j) u[s - KB] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], rr[j], u[s - KB], 0, 0, 0);
                }
            }
        }
        // H <- H * (U / den); padding atoms and columns stay exactly 0
#pragma unroll
        for (int b = 0; b < KB; ++b) {
            const int kl = (b < nblk && nvalid) ? K - 32 * (kb0 + b) - 4 * h : 0;      // atoms of this lane half left in the dictionary
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float d = bload(rD, (unsigned)(4 * h) * 4u, (unsigned)(32 * (kb0 + b) + d_row(r, 0)) * 4u);
                hr[b][r] = d_row(r, 0) < kl ? hr[b][r] * (u[b][r] / d) : 0.f;
            }
            __asm__ volatile("" ::: "memory");                      // one block's den values live at a time
        }
    }
#pragma unroll
    for (int b = 0; b < KB; ++b)
        if (b < nblk)
#pragma unroll
            for (int r = 0; r < 16; ++r) Hf[(long)(32 * (kb0 + b) + d_row(r, h)) * Np + c] = hr[b][r];
    // atom rows beyond the last 32-atom block (up to Kp) are padding
    for (int i = threadIdx.x; i < (Kp - 32 * Kb) * 32; i += blockDim.x) Hf[(long)(32 * Kb + (i >> 5)) * Np + (i & 31)] = 0.f;
}

// Waves per workgroup and 32-atom blocks per wave for K atoms: chosen from K alone (never from the batch).
static void fixed_shape(int K, int* Kb, int* KB, int* nw) {
    *Kb = gccnmf_ceil_div(K, 32);
    *KB = gccnmf_ceil_div(*Kb, FIXED_MAX_WAVES);
    *nw = gccnmf_ceil_div(*Kb, *KB);
}

bool gccnmf_klnmf_fixed_supported(int F, int K) { return F >= 2 && F <= 2049 && K >= 1 && K <= 1024; }

long gccnmf_klnmf_fixed_workspace_floats(int F, int K) { return (long)gccnmf_round_up(K, 64) * (gccnmf_round_up(F, 32) + 1); }

// den [Kp] | Wt [Kp][Fq] at the start of `workspace` (gccnmf_klnmf checks that the blind call's workspace holds them).
int gccnmf_klnmf_fixed_launch(const float* V, const float* W, float* H, float* workspace, int F, int N, int K, int batch, int iterations,
                              float alpha, float eps, bool ones, hipStream_t s) {
    if (!gccnmf_klnmf_fixed_supported(F, K)) return GCCNMF_ERR_UNSUPPORTED;
    const GccNmfPitches p = gccnmf_make_pitches(F, 1, K);
    const int Fp = p.Fp, Kp = p.Kp, Np = gccnmf_round_up(N, 64), Fq = gccnmf_round_up(F, 32);
    float* den = workspace;
    float* Wt = workspace + Kp;
    hipLaunchKernelGGL(nmf_fixed_prepare_kernel, dim3(Kp / 32), dim3(256), 0, s, W, Wt, den, F, K, Fq, Kp, alpha, eps);
    GCCNMF_CHECK_LAUNCH();
    int Kb, KB, nw;
    fixed_shape(K, &Kb, &KB, &nw);
    const dim3 grid((unsigned)batch * (Np / 32)), block(64 * nw);
    const int o = ones ? 1 : 0;
    switch (KB) {
        case 1: hipLaunchKernelGGL(nmf_fixed_kernel<1>, grid, block, 0, s, V, W, Wt, den, H, F, N, K, Fp, Fq, Kp, Np, Kb, iterations, o); break;
        case 2: hipLaunchKernelGGL(nmf_fixed_kernel<2>, grid, block, 0, s, V, W, Wt, den, H, F, N, K, Fp, Fq, Kp, Np, Kb, iterations, o); break;
        case 3: hipLaunchKernelGGL(nmf_fixed_kernel<3>, grid, block, 0, s, V, W, Wt, den, H, F, N, K, Fp, Fq, Kp, Np, Kb, iterations, o); break;
        case 4: hipLaunchKernelGGL(nmf_fixed_kernel<4>, grid, block, 0, s, V, W, Wt, den, H, F, N, K, Fp, Fq, Kp, Np, Kb, iterations, o); break;
        default: return GCCNMF_ERR_UNSUPPORTED;
    }
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}
