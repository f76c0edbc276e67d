// KL-NMF multiplicative updates on gfx950 -- the >98 %-of-FLOPs part of the GCC-NMF path.
// Reference: performKLNMF, gccNMF/gccNMFFunctions.py:69-83.
//
// One iteration (reference lines in brackets) is five launches that cover the whole batch:
//   K1  R  = V / (W . (s*H))                     MFMA GEMM + divide epilogue            [:76 inner]
//   K2  H  = (s*H) * (W^T . R) / (colsum W + alpha + eps)   MFMA GEMM + update epilogue [:76]
//   K3  R  = V / (W . H)                         (new H)                                [:77 inner]
//   K4a U  = R . H^T ,  rowsumH = sum_n H        MFMA GEMM, row sums from the staged B  [:77]
//   K4b W  = normalise(W * U / rowsumH); s = atom norms; colsumW = sum_f W             [:77,:79-80]
// The compensating rescale H *= norms (:81) is NOT a separate pass over H: it is the vector s,
// applied while K1 stages its B operand and inside K2's epilogue (which rewrites H anyway).
// gccnmf_klnmf materialises it once after the last iteration.
#include <mutex>
#include "gemm_ring.h"
#include "direct.h"
#include "update_w.h"
#include "divergence.h"
int gccnmf_klnmf_fixed_launch(const float* V, const float* W, float* H, float* workspace, int F, int N, int K, int batch, int iterations,
                              float alpha, float eps, bool ones, hipStream_t s);      // fixed dictionary, every iteration in one launch (nmf_fixed.hip)
bool gccnmf_klnmf_fixed_supported(int F, int K);
long gccnmf_klnmf_fixed_workspace_floats(int F, int K);
// semi-supervised KL-NMF (GCCNMF_FLAG_FREE_ATOMS): R.H^T and the W update of the free atoms alone (nmf_semi.hip)
bool gccnmf_klnmf_semi_supported(int F, int K, int nfree);
int gccnmf_klnmf_semi_rht_launch(const float* R, const float* H, float* U, float* rowsumH, int F, int N, int K, int nfree, int batch, hipStream_t s);
int gccnmf_klnmf_semi_update_w_launch(float* W, const float* U, const float* rowsumH, float* colsumW, float* hscale, int F, int K, int nfree,
                                      int batch, hipStream_t s);
// Itakura-Saito / Euclidean NMF (GCCNMF_FLAG_DIVERGENCE_IS / _EUCLIDEAN), nmf_beta.hip: stages 1-5 of that iteration
bool gccnmf_klnmf_beta_supported(int F, int K);
int gccnmf_klnmf_beta_stage_launch(int stage, int divergence, const float* V, float* W, float* H, float* R, float* Q, float* Un, float* Ud,
                                   float* colsumW, float* hscale, int F, int N, int K, int batch, float alpha, float eps, hipStream_t s);
// temporal-continuity KL-NMF (GCCNMF_FLAG_CONTINUITY), nmf_smooth.hip: stages 1-4 of that iteration
bool gccnmf_klnmf_smooth_supported(int F, int K, int batch);
int gccnmf_klnmf_smooth_stage_launch(int stage, const float* V, const float* W, float* H, float* R, float* U, float* rowsumH, const float* colsumW,
                                     const float* hscale, float* Gm, float* Gp, float* E, float* D, int F, int N, int K, int batch, int segments,
                                     float alpha, float eps, float weight, hipStream_t s);
#include "../../include/gccnmf_hip.h"

#include <atomic>
#include <cmath>
#include <cstring>
#include <algorithm>
#include <vector>
#define GCCNMF_SHARED_STREAMS 4
#define GCCNMF_CHAIN_MAX_ITERATIONS gccnmf_tune_chain_chunk   // iterations per chained launch (tuning key 24, default 2048: the grid stays far below 2^30 workgroups)
#define GCCNMF_RAGGED_MAX_BATCH 248   // files of a ragged batch: 8 lists of at most GEMM_RAGGED_LMAX
#define GCCNMF_SPLITS 4           // the one-file workspace layouts keep a RESERVED block of this many partial products (the room of a removed split-K path: nothing
                                  // reads or writes it; the sizes are part of what callers see, so the block stays where it is)
#define GCCNMF_DIRECT_MAX_BATCH 8    // workspaces of at most this many files carry the transposed copies of the direct path (key 12 selects up to here; from 8 files on
                                     // the ring / throughput kernels win anyway: 8 files 41.5 against 41.3 ms, 12 files 61.9 against 59.3)
// The tuning table (common.h documents the keys): default, lowest and highest value, experiment-only.  An unused slot has an EMPTY range (lo > hi: no
// value is accepted); it is kept so that the numbers of the other keys stay what tests, scripts and callers use.
struct GccNmfKnob {
    int def, lo, hi, experiment;
};
static const GccNmfKnob gccnmf_knobs[GCCNMF_TUNE_KEYS] = {
    {0, 1, 0, 0},                       //  0 (unused)
    {0, 1, 0, 0},                       //  1 (unused)
    {0, 0, 2, 0},                       //  2 tile_policy
    {1, 0, 1, 0},                       //  3 dma
    {0, 1, 0, 0},                       //  4 (unused)
    {0, 1, 0, 0},                       //  5 (unused)
    {0, 1, 0, 0},                       //  6 (unused)
    {1, 0, 1, 0},                       //  7 exact_div: the IEEE quotient since round 5 (measured cost on K1 / K3: 0.0 %, profiles/r05b_kbench_exact_div.txt)
    {3, 1, GCCNMF_SHARED_STREAMS, 0},   //  8 shared_groups
    {1, 0, 3, 0},                       //  9 tail_split (3 = half-height tiles everywhere: tests / measurements)
    {1, 0, 1, 0},                       // 10 direct
    {0, 1, 0, 0},                       // 11 (unused)
    {4, 1, GCCNMF_DIRECT_MAX_BATCH, 0}, // 12 direct_batch (measured, K = 1024: 4 files 21.8 ms against 25.8 on the ring kernel, 8 files 41.5 / 41.3)
    {0, 1, 0, 0},                       // 13 (unused)
    {0, 1, 0, 0},                       // 14 (unused)
    {0, 1, 0, 0},                       // 15 (unused)
    {1, 0, 2, 0},                       // 16 fused_k12
    {1, 0, 2, 0},                       // 17 fused_k34
    {0, 1, 0, 0},                       // 18 (unused)
    {0, 1, 0, 0},                       // 19 (unused)
    {0, 1, 0, 0},                       // 20 (unused)
    {1, 0, 8, 0},                       // 21 chain: 1 = the whole call as one chained launch where the rule in plan_klnmf says so; 0 off; forced forms (tests, A/B):
                                        //    2 = K1 | K2, 4 = K1 | K2 | K3 | K4 per iteration, 8 = every iteration of the call
    {0, 0, 1, 1},                       // 22 chain_solo: chained launches with one workgroup per CU (the freedom-from-deadlock test)
    {1, 0, 3, 0},                       // 23 chain_lists: 1 by rule (whole files per XCD where they balance, else spread) | 0 the plain launch's lists (batch a multiple of 8) |
                                        //    2 always spread: file-major equal eighths, agent-scope hand-over | 3 always whole files
    {2048, 1, 65536, 0},                // 24 chain_chunk: iterations per chained launch (a call of more iterations is several launches; tests use small values)
    {0, 0, 1, 1},                       // 25 chain_fault: fault injection -- consumers of chained launches give up waiting at once (the failure path's test)
};
static std::atomic<int> gccnmf_knob_value[GCCNMF_TUNE_KEYS];
static std::atomic<int> gccnmf_knobs_ready{0};
static void gccnmf_knobs_init() {
    static std::mutex mu;
    if (gccnmf_knobs_ready.load(std::memory_order_acquire)) return;
    std::lock_guard<std::mutex> lock(mu);
    if (gccnmf_knobs_ready.load(std::memory_order_relaxed)) return;
    for (int k = 0; k < GCCNMF_TUNE_KEYS; ++k) gccnmf_knob_value[k].store(gccnmf_knobs[k].def, std::memory_order_relaxed);
    gccnmf_knobs_ready.store(1, std::memory_order_release);
}
static GccNmfTune gccnmf_tune_load() {
    gccnmf_knobs_init();
    GccNmfTune t;
    for (int k = 0; k < GCCNMF_TUNE_KEYS; ++k) t.v[k] = gccnmf_knob_value[k].load(std::memory_order_relaxed);
    return t;
}
thread_local GccNmfTune gccnmf_tune = gccnmf_tune_load();
static thread_local int gccnmf_call_depth = 0;
GccNmfCall::GccNmfCall() {
    if (gccnmf_call_depth++ == 0) gccnmf_tune = gccnmf_tune_load();      // one snapshot per outermost library call
}
GccNmfCall::~GccNmfCall() { --gccnmf_call_depth; }
long long* gccnmf_trace_buf = nullptr;
int gccnmf_trace_blocks = 0;

extern "C" {
int gccnmf_version(void) { return 106; }   // round 5: work lists with narrow items in the throughput tile (gccnmf_debug_gemm_plan), IEEE division by default,
                                           // tuning keys as atomics snapshotted per call, product / experiment build flavours (42 product entry points)

int gccnmf_set_tuning(int key, int value) {
    GCCNMF_ENTER();
    gccnmf_knobs_init();
    if (key < 1 || key >= GCCNMF_TUNE_KEYS) return GCCNMF_ERR_ARG;
    const GccNmfKnob& k = gccnmf_knobs[key];
#ifndef GCCNMF_EXPERIMENTS
    if (k.experiment) return GCCNMF_ERR_ARG;                 // the test hooks of experiment builds
#endif
    if (value < k.lo || value > k.hi || (key == 21 && value != 0 && value != 1 && value != 2 && value != 4 && value != 8)) return GCCNMF_ERR_ARG;
    gccnmf_knob_value[key].store(value, std::memory_order_relaxed);      // takes effect at the next library call (GccNmfCall)
    return GCCNMF_OK;
}

}  // extern "C"

extern "C" {
#ifdef GCCNMF_EXPERIMENTS
int gccnmf_debug_set_trace(long long* buf, int blocks) {
    GCCNMF_ENTER();
    gccnmf_trace_buf = buf;
    gccnmf_trace_blocks = buf ? blocks : 0;
    return GCCNMF_OK;
}

#endif

int gccnmf_pitches(int F, int T, int K, int* Fp, int* Kp, int* Np, int* Tp) {
    GCCNMF_ENTER();
    if (F < 2 || T < 1 || K < 1 || !Fp || !Kp || !Np || !Tp) return GCCNMF_ERR_ARG;
    GccNmfPitches p = gccnmf_make_pitches(F, T, K);
    *Fp = p.Fp;
    *Kp = p.Kp;
    *Np = p.Np;
    *Tp = p.Tp;
    return GCCNMF_OK;
}
}

#ifdef GCCNMF_EXPERIMENTS
// MFMA-only probe: what the f32 matrix pipe sustains on this box (clock included), nothing but 8 independent
// accumulator chains per wave, two waves per SIMD.  grid = 512 blocks of 256 threads.
__global__ __launch_bounds__(256, 2) void mfma_peak_kernel(float* out, int iters) {
    f32x16 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    float a = 1.0f + threadIdx.x * 1e-3f, b = 0.5f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i], 0, 0, 0);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) s += acc[i][r];
    if (s == 123.456f) out[0] = s;
}
#endif

// ------------------------------------------------------------------------------------------
// small K-vector kernels
// ------------------------------------------------------------------------------------------
// colsumW[k] = sum_f W[f][k]; hscale[k] = 1.   grid = batch * Kp/16, 256 threads = 16 atoms x 16 row phases (one file: 64 workgroups
// of 33-row chains instead of 16 of 129: 40 -> ~8 us).
__global__ __launch_bounds__(256) void nmf_prepare_kernel(const float* __restrict__ W, float* __restrict__ colsumW,
                                                          float* __restrict__ hscale, int F, int Fp, int Kp) {
    __shared__ float red[4][16];
    const int chunks = Kp / 16;
    const int b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;
    const int c = threadIdx.x & 15, q = threadIdx.x >> 4, wave = threadIdx.x >> 6;
    const int k = ch * 16 + c;
    const float* Wb = W + (long)b * Fp * Kp;
    float s = 0.f;
#pragma unroll 4
    for (int f = q; f < F; f += 16) s += Wb[(long)f * Kp + k];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if ((threadIdx.x & 63) < 16) red[wave][c] = s;
    __syncthreads();
    if (threadIdx.x < 16) {
        colsumW[(long)b * Kp + k] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
        hscale[(long)b * Kp + k] = 1.f;
    }
}

// W update + unit-L2 atom normalisation (gccNMFFunctions.py:77,79-80):
//   Wt = W * (U / rowsumH[k]);  norm[k] = sqrt(sum_f Wt^2);  W = Wt / norm;  hscale = norm;  colsumW = sum_f W
// grid = batch * Kp/AT, 256 threads = AT atoms x 256/AT row phases; W and U are read twice (L2-resident) instead of
// keeping F*AT/256 values per thread in registers.  AT = 64 for big batches (256-byte row segments); AT = 16 when the
// launch would otherwise be a handful of workgroups (single file: 16 -> 64 workgroups, 4x shorter row loops).
template <int AT>
__global__ __launch_bounds__(256) void nmf_update_w_kernel(float* __restrict__ W, const float* __restrict__ U,
                                                           const float* __restrict__ rowsumH, float* __restrict__ colsumW,
                                                           float* __restrict__ hscale, int F, int Fp, int K, int Kp,
                                                           long sW, long sU, long sVec, long sRowsum) {
    constexpr int PH = 256 / AT;
    __shared__ float red[256];
    __shared__ float s_norm[AT];
    const int chunks = Kp / AT;
    const int b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;
    const int c = threadIdx.x % AT, q = threadIdx.x / AT;
    const int k = ch * AT + c;
    const bool valid = k < K;          // padded atoms stay exactly zero
    float* Wb = W + b * sW;
    const float* Ub = U + b * sU;
    const float rs = valid ? rowsumH[b * sRowsum + k] : 1.f;
    float ss = 0.f;
    if (valid)
        for (int f = q; f < F; f += PH) {
            const float wt = Wb[(long)f * Kp + k] * (Ub[(long)f * Kp + k] / rs);
            ss = fmaf(wt, wt, ss);
        }
    red[threadIdx.x] = ss;
    __syncthreads();
    if (q == 0) {
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < PH; ++j) t += red[c + AT * j];
        s_norm[c] = sqrtf(t);
    }
    __syncthreads();
    const float norm = s_norm[c];
    float cs = 0.f;
    if (valid)
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
        for (int j = 0; j < PH; ++j) t += red[c + AT * j];
        colsumW[b * sVec + k] = t;
        hscale[b * sVec + k] = norm;
    }
}

// The same update in ONE pass for launches of a few files (the two-pass kernel above re-reads W and U, 64 dependent
// round trips per thread: 50 us for one file at K = 1024): 16 atoms per workgroup as float4 columns x 64 row phases, the
// R <= 17 rows of a thread stay in registers between the norm and the store, all loads of a thread are independent.
// Column reductions: xor-shuffles over the 16 row phases of a wave, then 4 waves through LDS (fixed order: deterministic).
template <int AT>
__global__ __launch_bounds__(256) void nmf_update_w_onepass_kernel(float* __restrict__ W, const float* __restrict__ U,
                                                                   const float* __restrict__ rowsumH, float* __restrict__ colsumW,
                                                                   float* __restrict__ hscale, int F, int K, int Kp, long sW, long sU,
                                                                   long sVec, long sRowsum, float* __restrict__ Wt, long sWt, int ldwt) {
    __shared__ __attribute__((aligned(16))) float smem[5 * AT];
    const int chunks = Kp / AT;
    const int b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;
    nmf_update_w_onepass_item<AT>(W, U, rowsumH, colsumW, hscale, F, K, Kp, sW, sU, sVec, sRowsum, Wt, sWt, ldwt, b, ch, smem, (int)threadIdx.x);
}

// `a`: the factors and their strides (direct.h; update_w_args below fills it); what it does not hold: the files of this launch, the file groups that
// run it side by side and the transposed copy of W the direct path keeps (Wt, or nullptr)
static int launch_update_w(const UpdateWArgs& a, int batch, int groups, hipStream_t s, float* Wt, long sWt, int ldwt) {
    const int Kp = a.Kp;
    const long sized = (long)batch * groups;           // files of every group that runs this launch side by side: the kernel is chosen for all of them
    if (sized * (Kp / 64) < 256 && a.F <= 64 * 9) {
        // 16 atoms per workgroup (64-byte row segments); 8 (twice the workgroups, 32-byte segments) measured slower: 13.0 vs 11.4 us for one
        // file at K = 1024
#define GCCNMF_ONEPASS(AT_) hipLaunchKernelGGL((nmf_update_w_onepass_kernel<AT_>), dim3(batch * (Kp / AT_)), dim3(256), 0, s, a.W, a.U, a.rowsumH, \
                                               a.colsumW, a.hscale, a.F, a.K, Kp, a.sW, a.sU, a.sVec, a.sRowsum, Wt, sWt, ldwt)
        // short dictionaries at batch scale (64 files, K = 128: the launch between the two fused GEMM launches): 32 atoms per workgroup =
        // whole 128-byte lines per row and workgroup -- with 16 atoms every line of W and U is fetched by two workgroups (17 us for 51 MB).
        // Only for K <= 128, where the launch forms follow the batch size anyway (a file's bits are batch-independent for K > 128).
        if (!Wt && a.K <= 128 && sized * (Kp / 32) >= 256) GCCNMF_ONEPASS(32);
        else GCCNMF_ONEPASS(16);
#undef GCCNMF_ONEPASS
        GCCNMF_CHECK_LAUNCH();
        return GCCNMF_OK;
    }
    const int Fp = gccnmf_round_up(a.F, 16);
    if (sized * (Kp / 64) >= 256) {
        hipLaunchKernelGGL(nmf_update_w_kernel<64>, dim3(batch * (Kp / 64)), dim3(256), 0, s, a.W, a.U, a.rowsumH, a.colsumW, a.hscale, a.F, Fp, a.K,
                           Kp, a.sW, a.sU, a.sVec, a.sRowsum);
    } else {
        hipLaunchKernelGGL(nmf_update_w_kernel<16>, dim3(batch * (Kp / 16)), dim3(256), 0, s, a.W, a.U, a.rowsumH, a.colsumW, a.hscale, a.F, Fp, a.K,
                           Kp, a.sW, a.sU, a.sVec, a.sRowsum);
    }
    GCCNMF_CHECK_LAUNCH();
    if (Wt) return gccnmf_transpose_launch(a.W, a.sW, Kp, Wt, sWt, ldwt, a.F, Kp, batch, s);      // (the one-pass kernel writes it itself)
    return GCCNMF_OK;
}

// H[k][:] *= hscale[k].  grid = batch * K rows, 256 threads.  (sScale = 0: one shared scale vector; file b starts sH floats after
// file b-1, rows are ld floats apart, Np of them are touched)
__global__ __launch_bounds__(256) void nmf_scale_h_kernel(float* __restrict__ H, const float* __restrict__ hscale, long sScale,
                                                          int K, long sH, int ld, int Np) {
    const int b = blockIdx.x / K, k = blockIdx.x - b * K;
    const float s = hscale[b * sScale + k];
    float4* row = (float4*)(H + b * sH + (long)k * ld);
    for (int i = threadIdx.x; i < Np / 4; i += 256) {
        float4 v = row[i];
        v.x *= s;
        v.y *= s;
        v.z *= s;
        v.w *= s;
        row[i] = v;
    }
}

__global__ __launch_bounds__(256) void nmf_fill_kernel(float* __restrict__ p, float v, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// out[i] = sum_b in[b*stride + i], files added in ascending order (deterministic); accumulate: out[i] += that sum (a rank's
// second, third ... shard: the shards' sums are added in shard order).
__global__ __launch_bounds__(256) void nmf_reduce_files_kernel(const float* __restrict__ in, long stride, int batch, long n,
                                                               float* __restrict__ out, int accumulate) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int b = 0; b < batch; ++b) s += in[b * stride + i];
    out[i] = accumulate ? out[i] + s : s;
}

// ------------------------------------------------------------------------------------------
// GEMM dispatch: tall <4,1> tile for >128 output rows, wide <1,4> otherwise
// ------------------------------------------------------------------------------------------
// Tile choice.  Throughput tile: <4,1> x TM=4 = 512 x 64 per workgroup (128 x 64 per wave).  When the whole launch has
// fewer tall tiles than the chip has CUs (a single file: 16-40 of them), a workgroup's duration IS the launch duration,
// so the same 4 waves take a 128 x 64 tile instead (TM = 1: 32 x 64 per wave, 4x shorter, 4x more workgroups).
// <1,4> serves outputs of <= 128 rows at any batch.
static bool small_batch_tile(const GemmArgs& a) {
    if (a.M <= 128 || gccnmf_tune_tile_policy == 1) return false;
    if (gccnmf_tune_tile_policy == 2) return true;
    // (file groups that run side by side -- a.concurrent of them -- are sized together: a file's tile does not depend on how the batch was split)
    const long tall_tiles = (long)a.batch * (a.concurrent > 1 ? a.concurrent : 1) * gccnmf_ceil_div(a.M, 512) * gccnmf_ceil_div(a.N, 64);
    return tall_tiles < 256;
}

enum GemmFamily { GEMM_RING, GEMM_SMALL_BATCH, GEMM_DMA, GEMM_TALL, GEMM_WIDE };
template <bool A_KC, bool B_KC, int EPI, bool TAIL>
static int launch_gemm_family(GemmFamily family, const GemmArgs& a, hipStream_t s) {
    switch (family) {
        case GEMM_RING: return gccnmf_launch_gemm_ring<A_KC, B_KC, EPI, TAIL>(a, s);
        case GEMM_SMALL_BATCH: return gccnmf_launch_gemm<4, 1, A_KC, B_KC, EPI, TAIL, 1>(a, s);
        case GEMM_DMA: return gccnmf_launch_gemm_dma<A_KC, B_KC, EPI, TAIL>(a, s);
        case GEMM_TALL: return gccnmf_launch_gemm<4, 1, A_KC, B_KC, EPI, TAIL>(a, s);
        default: return gccnmf_launch_gemm<1, 4, A_KC, B_KC, EPI, TAIL>(a, s);
    }
}

template <bool A_KC, bool B_KC, int EPI>
static int dispatch_gemm(const GemmArgs& a, bool tail, hipStream_t s) {
    const bool tall = a.M > 128;
    // The H update of a SMALL dictionary (K <= 128 atoms = output rows: the reference driver's default, runGCCNMF.py:41) used to ride the
    // register-staged wide tile (128 x 256 per workgroup, one k-tile prefetched): 154 us per launch for 64 files at K = 128 = 0.43 of the
    // matrix peak.  The LDS-DMA ring kernel's 128 x 64 tiles (six stages in flight, image-layout epilogue) take it instead.
    const bool short_updh = !tall && EPI == EPI_UPDH && gccnmf_tune_tile_policy != 1 && a.N >= 256;
    const bool ring = (small_batch_tile(a) || short_updh) && gccnmf_ring_supports(a.Kd);   // (longer reductions: the register-staged tile)
    const GemmFamily family = ring ? GEMM_RING : small_batch_tile(a) ? GEMM_SMALL_BATCH : !tall ? GEMM_WIDE : gccnmf_tune_dma ? GEMM_DMA : GEMM_TALL;
    if (tail && !A_KC) return GCCNMF_ERR_ARG;      // the VALU tail row needs a reduction-contiguous A
    return tail ? launch_gemm_family<A_KC, B_KC, EPI, A_KC>(family, a, s) : launch_gemm_family<A_KC, B_KC, EPI, false>(family, a, s);
}

struct NmfGeom {
    int F, N, K, Fp, Kp, Np;
    int ld;         // row pitch (floats) of V, R and H: Np for back-to-back files, the big matrix's pitch for column blocks
    int Fm;         // rows computed on the matrix cores
    bool tail;      // F % 128 == 1: the last bin rides on the VALU
    long sV, sW, sH, sU;
};

static NmfGeom make_geom(int F, int N, int K) {
    NmfGeom g;
    GccNmfPitches p = gccnmf_make_pitches(F, 1, K);
    g.F = F; g.N = N; g.K = K;
    g.Fp = p.Fp; g.Kp = p.Kp; g.Np = gccnmf_round_up(N, 64);
    g.ld = g.Np;
    g.tail = (F % 128) == 1 && F > 1;
    g.Fm = g.tail ? F - 1 : F;
    g.sV = (long)g.Fp * g.Np;
    g.sW = (long)g.Fp * g.Kp;
    g.sH = (long)g.Kp * g.Np;
    g.sU = (long)g.Fp * g.Kp;
    return g;
}

// What the `flags` word of gccnmf_klnmf / _stage / _plan / _ragged asks for, decoded ONCE at the entry point; everything below reads these fields.
struct KlnmfMode {
    bool xcd_affine;            // not GCCNMF_FLAG_NO_XCD_AFFINITY
    bool unfused_w_update;      // GCCNMF_FLAG_UNFUSED_W_UPDATE
    int groups;                 // GCCNMF_FLAG_GROUPS: file groups that run this call side by side on separate streams, launch forms sized for all (1 = alone)
    bool fixed_w, h_ones;       // GCCNMF_FLAG_FIXED_W, GCCNMF_FLAG_H_ONES
    int free_atoms;             // GCCNMF_FLAG_FREE_ATOMS(n): the last n atoms of every file's W are learned beside a dictionary (0 = not semi-supervised)
    int divergence;             // bits 26-27: 0 = KL, 1 = GCCNMF_FLAG_DIVERGENCE_IS, 2 = GCCNMF_FLAG_DIVERGENCE_EUCLIDEAN
    int segments;               // GCCNMF_FLAG_CONTINUITY: the column segments the temporal-continuity term runs inside (1 | 2 with _STEREO), 0 = no such term
    float continuity;           // ... and its weight (unpack_continuity took it out of K and batch)
};
// GCCNMF_FLAG_CONTINUITY: the weight's float32 bits ride in the upper halves of K and batch (GCCNMF_CONTINUITY_K / _BATCH); the entry points
// call this FIRST, so that everything behind it sees the plain K and batch.  Without the bit the words are left alone.  GCCNMF_ERR_ARG:
// the stereo bit without the continuity bit, a weight that is negative, NaN or Inf, two segments with N odd.
static int unpack_continuity(int flags, int N, int& K, int& batch, KlnmfMode& m) {
    m.segments = 0;
    m.continuity = 0.f;
    if (!(flags & GCCNMF_FLAG_CONTINUITY)) return (flags & GCCNMF_FLAG_CONTINUITY_STEREO) ? GCCNMF_ERR_ARG : GCCNMF_OK;
    const unsigned bits = ((unsigned)K & 0xffff0000u) | ((unsigned)batch >> 16);
    K &= 0xffff;
    batch &= 0xffff;
    std::memcpy(&m.continuity, &bits, sizeof(float));
    m.segments = (flags & GCCNMF_FLAG_CONTINUITY_STEREO) ? 2 : 1;
    if (!(m.continuity >= 0.f) || std::isinf(m.continuity)) return GCCNMF_ERR_ARG;
    return m.segments == 2 && (N & 1) ? GCCNMF_ERR_ARG : GCCNMF_OK;
}
// ... with the argument rules of the flag combinations, decided before anything is launched: GCCNMF_OK = a valid word.
//   fixed dictionary: GCCNMF_FLAG_FIXED_W alone or with GCCNMF_FLAG_H_ONES, nothing else (H_ONES without FIXED_W: GCCNMF_ERR_ARG)
//   free atoms: not with the concurrent-groups or the unfused-W-update bit, n <= 128, n < K (GCCNMF_ERR_ARG); (K - n) % 16 == 0, K <= 1024,
//   F <= 2049 (GCCNMF_ERR_UNSUPPORTED)
//   IS / Euclid: one of the two bits, not with a fixed dictionary, the all-ones start, free atoms, concurrent groups or the unfused W update
//   (GCCNMF_ERR_ARG); F <= 2049, K <= 1024 (GCCNMF_ERR_UNSUPPORTED)
//   temporal continuity (m.segments, set by unpack_continuity): with none of those, nor IS / Euclid (GCCNMF_ERR_ARG); F <= 2049, K <= 1024
//   (GCCNMF_ERR_UNSUPPORTED)
static int decode_mode(int flags, int F, int K, KlnmfMode& m) {
    const int n = (flags & (GCCNMF_FLAG_GROUPS(255) & ~GCCNMF_FLAG_CONCURRENT_GROUPS)) / (GCCNMF_FLAG_GROUPS(1) & ~GCCNMF_FLAG_CONCURRENT_GROUPS);
    m.xcd_affine = !(flags & GCCNMF_FLAG_NO_XCD_AFFINITY);
    m.unfused_w_update = (flags & GCCNMF_FLAG_UNFUSED_W_UPDATE) != 0;
    m.groups = (flags & GCCNMF_FLAG_CONCURRENT_GROUPS) ? (n >= 2 ? n : 2) : 1;
    m.fixed_w = (flags & GCCNMF_FLAG_FIXED_W) != 0;
    m.h_ones = (flags & GCCNMF_FLAG_H_ONES) != 0;
    m.free_atoms = (flags & GCCNMF_FLAG_FREE_ATOMS(255)) / GCCNMF_FLAG_FREE_ATOMS(1);
    m.divergence = (flags >> 26) & 3;
    if (m.segments) {
        if (m.divergence || m.fixed_w || m.h_ones || m.free_atoms || (flags & GCCNMF_FLAG_CONCURRENT_GROUPS) || m.unfused_w_update) return GCCNMF_ERR_ARG;
        return gccnmf_klnmf_smooth_supported(F, K, 1) ? GCCNMF_OK : GCCNMF_ERR_UNSUPPORTED;
    }
    if (m.divergence) {
        if (m.divergence == 3 || m.fixed_w || m.h_ones || m.free_atoms || (flags & GCCNMF_FLAG_CONCURRENT_GROUPS) || m.unfused_w_update) return GCCNMF_ERR_ARG;
        return gccnmf_klnmf_beta_supported(F, K) ? GCCNMF_OK : GCCNMF_ERR_UNSUPPORTED;
    }
    if (m.fixed_w || m.h_ones) return m.fixed_w && !(flags & ~(GCCNMF_FLAG_FIXED_W | GCCNMF_FLAG_H_ONES)) ? GCCNMF_OK : GCCNMF_ERR_ARG;
    if (!m.free_atoms) return GCCNMF_OK;
    if (m.groups > 1 || m.unfused_w_update || m.free_atoms > 128 || m.free_atoms >= K) return GCCNMF_ERR_ARG;
    return gccnmf_klnmf_semi_supported(F, K, m.free_atoms) ? GCCNMF_OK : GCCNMF_ERR_UNSUPPORTED;
}

// The operands of the iteration's GEMMs, stated ONCE: the plain launches below and the chained launch (launch_klnmf_chain) both build them here, which
// is what makes a chained call bit for bit the plain one.  sW, sScale, sVec: per-file strides of W and of the K-vectors (0 = one dictionary shared
// by every file: the shared-dictionary callers).  xcd_affine / concurrent: GemmArgs' fields of those names (gemm_dma.h).
// K1, K3: R = V / (W . (hscale*H))   (hscale = nullptr: K3, H carries its scale already)
static GemmArgs wh_div_args(const NmfGeom& g, const float* V, const float* W, long sW, const float* H, const float* hscale, long sScale, float* R,
                            int batch, int xcd_affine, int concurrent) {
    GemmArgs a = {};
    a.A = W; a.sA = sW; a.lda = g.Kp; a.a_clamp = g.Fp - 1;
    a.B = H; a.sB = g.sH; a.ldb = g.ld; a.b_clamp = g.Np - 4;
    a.M = g.Fm; a.N = g.N; a.Kd = g.K;
    a.batch = batch; a.xcd_affine = xcd_affine; a.concurrent = concurrent;
    a.bscale = hscale; a.s_bscale = sScale;
    a.tail_row = g.F - 1;
    a.C = R; a.sC = g.sV; a.ldc = g.ld;
    a.E0 = V; a.sE0 = g.sV;
    return a;
}

// K2: H = (hscale*H) * (W^T . R) / (colsumW + alpha + eps)
static GemmArgs update_h_args(const NmfGeom& g, const float* W, long sW, const float* R, float* H, const float* hscale, long sScale,
                              const float* colsumW, long sVec, float alpha, float eps, int batch, int xcd_affine, int concurrent) {
    GemmArgs a = {};
    a.A = W; a.sA = sW; a.lda = g.Kp; a.a_clamp = g.Kp - 4;
    a.B = R; a.sB = g.sV; a.ldb = g.ld; a.b_clamp = g.Np - 4;
    a.M = g.K; a.N = g.N; a.Kd = g.F;
    if ((g.F % 16) == 1) {   // F = 16*n + 1: bin F-1 leaves the matrix cores and becomes a rank-1 term of the epilogue
        a.Kd = g.F - 1;      // (always so in a chained launch: chain_capable admits no other F)
        a.ktailA = W + (long)(g.F - 1) * g.Kp; a.s_ktailA = sW;
        a.ktailB = R + (long)(g.F - 1) * g.ld; a.s_ktailB = g.sV;
    }
    a.batch = batch; a.xcd_affine = xcd_affine; a.concurrent = concurrent;
    a.C = H; a.sC = g.sH; a.ldc = g.ld;
    a.E1 = hscale; a.sE1 = sScale;
    a.E2 = colsumW; a.sE2 = sVec;
    a.alpha = alpha; a.eps = eps;
    return a;
}

// the product both forms of K4 share: R . H^T
static GemmArgs rht_operands(const NmfGeom& g, const float* R, const float* H, int batch, int xcd_affine, int concurrent) {
    GemmArgs a = {};
    a.A = R; a.sA = g.sV; a.lda = g.ld; a.a_clamp = g.Fp - 1;
    a.B = H; a.sB = g.sH; a.ldb = g.ld; a.b_clamp = g.Kp - 1;
    a.M = g.Fm; a.N = g.K; a.Kd = g.N;
    a.batch = batch; a.xcd_affine = xcd_affine; a.concurrent = concurrent;
    a.tail_row = g.F - 1;
    return a;
}

// K4a: U = R . H^T, rowsumH = sum_n H
static GemmArgs rht_args(const NmfGeom& g, const float* R, const float* H, float* U, float* rowsumH, int batch, int xcd_affine, int concurrent) {
    GemmArgs a = rht_operands(g, R, H, batch, xcd_affine, concurrent);
    a.rowsumB = rowsumH; a.s_rowsumB = g.Kp;
    a.C = U; a.sC = g.sU; a.ldc = g.Kp;
    return a;
}

// K4a and K4b in one: W = normalise(W * (R.H^T) / rowsumH), colsumW, hscale
static GemmArgs rht_update_w_args(const NmfGeom& g, const float* R, const float* H, float* W, float* colsumW, float* hscale, int batch,
                                  int xcd_affine, int concurrent) {
    GemmArgs a = rht_operands(g, R, H, batch, xcd_affine, concurrent);
    a.C = W; a.sC = g.sW; a.ldc = g.Kp;
    a.out_colsum = colsumW; a.out_norm = hscale; a.s_out = g.Kp;
    return a;
}

static int launch_wh_div(const NmfGeom& g, const GemmArgs& a, hipStream_t s) { return dispatch_gemm<true, false, EPI_DIV>(a, g.tail, s); }
static int launch_update_h(const GemmArgs& a, hipStream_t s) { return dispatch_gemm<false, false, EPI_UPDH>(a, false, s); }
static int launch_rht(const NmfGeom& g, const GemmArgs& a, hipStream_t s) { return dispatch_gemm<true, true, EPI_STORE>(a, g.tail, s); }

// W = normalise(W * (R.H^T) / rowsumH), colsumW, hscale -- K4a and K4b in one launch (tall tile, all F rows in one workgroup)
static int launch_rht_update_w(const NmfGeom& g, const GemmArgs& a, hipStream_t s) {
    // the LDS-DMA kernel carries only the full-tile form of this epilogue (every wave entirely inside or outside M, no
    // ragged atom tile); anything else takes the register-staged kernel with the generic one
    if (gccnmf_tune_dma && (a.M & 127) == 0 && (a.N & 63) == 0)
        return g.tail ? gccnmf_launch_gemm_dma<true, true, EPI_UPDW, true>(a, s) : gccnmf_launch_gemm_dma<true, true, EPI_UPDW, false>(a, s);
    return g.tail ? gccnmf_launch_gemm<4, 1, true, true, EPI_UPDW, true>(a, s) : gccnmf_launch_gemm<4, 1, true, true, EPI_UPDW, false>(a, s);
}

// ------------------------------------------------------------------------------------------
// The direct path (csrc/direct.hip): launches that cannot fill the chip -- one mixture alone, the shape behind the reference's
// own function names (runGCCNMF.py:41 -> performKLNMF(V, dictionarySize, 100, 0))
// ------------------------------------------------------------------------------------------
// All four GEMMs of an iteration as "both operands reduction-major" products, one round of one workgroup per CU each, the
// reduction split inside the workgroup (no partial products through HBM, no combine launches):
//   K1  R  = V / (Wt^T . (s*H))           A = Wt [k][f]   B = H  [k][n]      -> R [f][n]
//   K2  H  = (s*H) * (W^T . R) / (...)    A = W  [f][k]   B = R  [f][n]      -> H [k][n] and Ht [n][k]
//   K3  Rt = (V / (Wt^T . H))^T           A = Wt [k][f]   B = H  [k][n]      -> Rt [n][f] (+ the Nyquist row into R)
//   K4  U  = Rt^T . Ht, rowsumH           A = Rt [n][f]   B = Ht [n][k]      -> U [f][k]
//   K4b W update (one pass)                                                   -> W [f][k] and Wt [k][f]
// The transposed copies (Wt, Ht, Rt) live behind the other scratch in the workspace.  F = 16 n + 1 (513): bin F-1 is the VALU tail
// row of K1 / K3 / K4 and the rank-1 epilogue term of K2.
struct DirectBufs {
    float *Wt, *Ht, *Rt;
    long sWt, sHt, sRt;
    int ldwt, ldht, ldrt;
};
static long direct_floats(const NmfGeom& g, int batch) { return batch <= GCCNMF_DIRECT_MAX_BATCH ? (long)batch * (g.sU + g.sH + g.sV) : 0; }
static bool direct_path(const NmfGeom& g, int batch, int groups) {
    return gccnmf_tune_direct && gccnmf_tune_tile_policy == 0 && (long)batch * groups <= gccnmf_tune_direct_batch && batch <= GCCNMF_DIRECT_MAX_BATCH;
}
static DirectBufs direct_bufs(const NmfGeom& g, float* base, int batch) {
    DirectBufs d;
    d.sWt = (long)g.Kp * g.Fp; d.sHt = (long)g.Np * g.Kp; d.sRt = (long)g.Np * g.Fp;
    d.ldwt = g.Fp; d.ldht = g.Kp; d.ldrt = g.Fp;
    d.Wt = base;
    d.Ht = d.Wt + batch * d.sWt;
    d.Rt = d.Ht + batch * d.sHt;
    return d;
}
static bool direct_tail(const NmfGeom& g) { return g.F > 16 && (g.F % 16) == 1; }

// K1 (hscale != nullptr) and K3 (transposed output)
static int direct_wh_div(const NmfGeom& g, const DirectBufs& d, const float* V, const float* W, const float* H, const float* hscale, float* R,
                         bool transposed, int batch, hipStream_t s) {
    DirectArgs a = {};
    a.A = d.Wt; a.sA = d.sWt; a.lda = d.ldwt;
    a.B = H; a.sB = g.sH; a.ldb = g.ld;
    a.M = direct_tail(g) ? g.F - 1 : g.F; a.N = g.N; a.Kd = g.K; a.batch = batch;
    a.bscale = hscale; a.s_bscale = g.Kp;
    if (direct_tail(g)) {
        a.tailA = W + (long)(g.F - 1) * g.Kp; a.s_tailA = g.sW; a.tail_row = g.F - 1;
    }
    a.C = R; a.sC = g.sV; a.ldc = g.ld;
    a.E0 = V; a.sE0 = g.sV; a.lde0 = g.ld;
    if (transposed) {
        a.Ct = d.Rt; a.sCt = d.sRt; a.ldct = d.ldrt;
    }
    return gccnmf_direct_launch(a, transposed ? DEPI_DIVT : DEPI_DIV, 0, s);
}

static int direct_update_h(const NmfGeom& g, const DirectBufs& d, const float* W, const float* R, float* H, const float* hscale,
                           const float* colsumW, float alpha, float eps, int batch, hipStream_t s) {
    DirectArgs a = {};
    a.A = W; a.sA = g.sW; a.lda = g.Kp;
    a.B = R; a.sB = g.sV; a.ldb = g.ld;
    a.M = g.K; a.N = g.N; a.Kd = g.F; a.batch = batch;
    if (direct_tail(g)) {
        a.Kd = g.F - 1;
        a.ktailA = W + (long)(g.F - 1) * g.Kp; a.s_ktailA = g.sW;
        a.ktailB = R + (long)(g.F - 1) * g.ld; a.s_ktailB = g.sV;
    }
    a.C = H; a.sC = g.sH; a.ldc = g.ld;
    a.Ct = d.Ht; a.sCt = d.sHt; a.ldct = d.ldht;
    a.E1 = hscale; a.sE1 = g.Kp;
    a.E2 = colsumW; a.sE2 = g.Kp;
    a.alpha = alpha; a.eps = eps;
    return gccnmf_direct_launch(a, DEPI_UPDH, 0, s);
}

static int direct_rht(const NmfGeom& g, const DirectBufs& d, const float* R, float* U, float* rowsumH, int batch, hipStream_t s) {
    DirectArgs a = {};
    a.A = d.Rt; a.sA = d.sRt; a.lda = d.ldrt;
    a.B = d.Ht; a.sB = d.sHt; a.ldb = d.ldht;
    a.M = direct_tail(g) ? g.F - 1 : g.F; a.N = g.K; a.Kd = g.N; a.batch = batch;
    if (direct_tail(g)) {
        a.tailA = R + (long)(g.F - 1) * g.ld; a.s_tailA = g.sV; a.tail_row = g.F - 1;
    }
    a.rowsumB = rowsumH; a.s_rowsumB = g.Kp;
    a.C = U; a.sC = g.sU; a.ldc = g.Kp;
    return gccnmf_direct_launch(a, DEPI_STORE, 0, s);
}

// The operands of the short-dictionary launches (plan_klnmf says where they run).  K1 + K2 in one launch:
static WhUpdhArgs wh_updh_args(const NmfGeom& g, const float* V, const float* W, float* H, const float* hscale, const float* colsumW, float alpha,
                               float eps, int batch) {
    WhUpdhArgs a = {};
    a.W = W; a.sW = g.sW; a.lda = g.Kp;
    a.H = H; a.sH = g.sH; a.ldb = g.ld;
    a.V = V; a.sV = g.sV; a.ldv = g.ld;
    a.scale = hscale; a.colsum = colsumW; a.sVec = g.Kp;
    a.M = g.Fm; a.N = g.N; a.Kd = g.K; a.batch = batch;
    a.alpha = alpha; a.eps = eps;
    return a;
}

// K3 + K4a in one launch:
static WhdivRhtArgs whdiv_rht_args(const NmfGeom& g, const float* V, const float* W, const float* H, float* U, float* rowsumH, int batch) {
    WhdivRhtArgs a = {};
    a.W = W; a.sW = g.sW; a.lda = g.Kp;
    a.H = H; a.sH = g.sH; a.ldb = g.ld;
    a.V = V; a.sV = g.sV; a.ldv = g.ld;
    a.U = U; a.sU = g.sU; a.ldu = g.Kp;
    a.rowsumH = rowsumH; a.sVec = g.Kp;
    a.M = g.Fm; a.N = g.N; a.Kd = g.K; a.batch = batch;
    return a;
}
// the one-pass / two-pass W update (launch_update_w; the last stage of the short-dictionary chain).  sW, sU, sVec: per-file strides, 0 = shared
static UpdateWArgs update_w_args(const NmfGeom& g, float* W, long sW, const float* U, long sU, const float* rowsumH, float* colsumW, float* hscale,
                                 long sVec) {
    UpdateWArgs a = {};
    a.W = W; a.U = U; a.rowsumH = rowsumH; a.colsumW = colsumW; a.hscale = hscale;
    a.F = g.F; a.K = g.K; a.Kp = g.Kp; a.sW = sW; a.sU = sU; a.sVec = sVec; a.sRowsum = sVec;
    return a;
}

// ---- the workspace of gccnmf_klnmf / gccnmf_klnmf_ragged, carved in ONE place ---------------------------------------------------------
// R [batch][Fp][Np] | U [batch][Fp][Kp] | colsumW, rowsumH, hscale [batch][Kp] each | (batch == 1) a reserved block, unused: GCCNMF_SPLITS x
// max(Fp*Np, Fp*Kp) + GCCNMF_SPLITS x Kp floats | (batch <= GCCNMF_DIRECT_MAX_BATCH)
// the transposed copies of the direct path: Wt [batch][Kp][Fp], Ht [batch][Np][Kp], Rt [batch][Np][Fp] | the ready counters of the chained
// launches (tuning key 21; gemm_dma.h: GemmSync, gccnmf_gemm_chain_kernel) | the status words | (a ragged batch) its tables.
// Counters of one file group: c12 [batch][tiles_n] (K1 -> K2, in 32-column blocks), c23 [batch][tiles_n] (K2 -> K3), c34 [batch] (K3 -> K4, items),
// c41 [batch] (K4 -> the next iteration's K1, items).  Zeroed once per gccnmf_klnmf call; iteration `it` waits for (it + 1) x the per-iteration count,
// so nothing is reset between launches.  (The short-dictionary chain keeps its [3][batch] counters at the same place.)
// The ready counters are rounded up to a 128-byte line (32 words), the GCCNMF_STATUS_WORDS status words follow: error [1], 15 unused, XCCs
// seen per list [8] (from GCCNMF_STATUS_XCC_SEEN on), 8 unused.  Every block in front of the counters is a multiple of 64 floats, the counter and status
// block one of 32, so the workspace is a multiple of 32 (a ragged batch's, with its tables: of 4) -- workspaces carved back to back out of ONE allocation (the engine's file groups) all start
// 16-byte aligned when the first does, which the float4 / LDS-DMA accesses to R, U, Wt, Ht, Rt rely on (the entry points reject a workspace that is
// not 16-byte aligned).  Everything that locates a block -- the size functions included: `floats` of a carve of no memory -- takes it from here.
#define GCCNMF_STATUS_WORDS 32
#define GCCNMF_STATUS_XCC_SEEN 16
struct KlnmfWorkspace {
    float *R, *U, *colsumW, *rowsumH, *hscale;
    float* direct_base;                     // Wt | Ht | Rt (direct_bufs)
    unsigned *c12, *c23, *c34, *c41;        // ready counters
    unsigned *status, *xcc_seen;
    int* ragged_tables;                     // the files' column counts [batch] | 8 lists of GEMM_RAGGED_LMAX + 1 words
    long scratch_floats;                    // everything in front of the counters
    long counter_words;                     // ready counters, their padding and the status words: what zero_chain_counters clears
    long floats;                            // the whole workspace
};
static long ragged_table_ints(int batch) { return (long)gccnmf_round_up(batch + 8 * (GEMM_RAGGED_LMAX + 1), 4); }
static KlnmfWorkspace carve(float* workspace, const NmfGeom& g, int batch, bool ragged) {
    KlnmfWorkspace ws;
    long end = 0;
    auto take = [&](long n) { float* p = workspace ? workspace + end : nullptr; end += n; return p; };      // (nullptr: the size functions)
    ws.R = take(batch * g.sV);
    ws.U = take(batch * g.sU);
    ws.colsumW = take((long)batch * g.Kp);
    ws.rowsumH = take((long)batch * g.Kp);
    ws.hscale = take((long)batch * g.Kp);
    if (batch == 1) take(GCCNMF_SPLITS * ((g.sV > g.sU ? g.sV : g.sU) + (long)g.Kp));      // the reserved block
    ws.direct_base = take(direct_floats(g, batch));
    ws.scratch_floats = end;
    const long tn = gccnmf_ceil_div(g.N, 64);
    ws.c12 = (unsigned*)take(batch * tn);
    ws.c23 = (unsigned*)take(batch * tn);
    ws.c34 = (unsigned*)take(batch);
    ws.c41 = (unsigned*)take(batch);
    end = ws.scratch_floats + (end - ws.scratch_floats + 31) / 32 * 32;
    ws.status = (unsigned*)take(GCCNMF_STATUS_WORDS);
    ws.xcc_seen = workspace ? ws.status + GCCNMF_STATUS_XCC_SEEN : nullptr;
    ws.counter_words = end - ws.scratch_floats;
    ws.ragged_tables = (int*)take(ragged ? ragged_table_ints(batch) : 0);
    ws.floats = end;
    return ws;
}
// An IS / Euclidean call's workspace is the KL carve above followed by GCCNMF_KLNMF_DIVERGENCE_WORKSPACE_FLOATS more floats: Q [batch][Fp][Np] |
// Ud [batch][Fp][Kp] (the KL carve is a multiple of 32 floats: both blocks start 16-byte aligned).  R, U (= Un), colsumW, hscale, the status words
// and stage 7's float64 partials and results sit where the KL call keeps them.
struct BetaWorkspace {
    float *Q, *Ud;
};
static BetaWorkspace carve_beta(float* workspace, const KlnmfWorkspace& ws, const NmfGeom& g, int batch) {
    BetaWorkspace b;
    b.Q = workspace + ws.floats;
    b.Ud = b.Q + batch * g.sV;
    return b;
}
// A temporal-continuity call's workspace is the KL carve followed by GCCNMF_KLNMF_CONTINUITY_WORKSPACE_FLOATS more floats: Gm | Gp
// [batch][Kp][Np] each | E | D [batch][2][Kp] each (segment-major inside a file).
struct SmoothWorkspace {
    float *Gm, *Gp, *E, *D;
};
static SmoothWorkspace carve_smooth(float* workspace, const KlnmfWorkspace& ws, const NmfGeom& g, int batch) {
    SmoothWorkspace w;
    w.Gm = workspace + ws.floats;
    w.Gp = w.Gm + batch * g.sH;
    w.E = w.Gp + batch * g.sH;
    w.D = w.E + (long)batch * 2 * g.Kp;
    return w;
}
static bool workspace_aligned(const void* workspace) { return ((uintptr_t)workspace & 15) == 0; }

// The lists of a chained launch (tuning key 23): 1 = whole files per XCD (hand-over through that XCD's L2), 2 = the file-major tile list cut into equal
// eighths (a file may straddle XCDs: agent-scope hand-over, the producer writes its L2 back before it signals), 0 = the plain launch's lists.
// By rule (key 23 = 1): whole files where they balance -- the longest list at most 2.7 % above the mean, i.e. multiples of 8 and e.g. 102 files -- else the
// spread lists.  Same box (profiles/r06y_files_sweep_*.txt, iteration as a fraction of peak, whole | spread): 64 files 0.845 | 0.830 (the write-back costs
// 1.7 %), 24: 0.774 | 0.761, 32: 0.840 | 0.826, 40: 0.849 | 0.832; 26: plain 0.698 | spread 0.786, 51: plain 0.781 | 0.826, 52: whole 0.795 | 0.826,
// 77: 0.826 | 0.829, 25: plain 0.763 | 0.774, 20: plain 0.642 | 0.685; 16 files: plain 0.747, chained 0.584 -- the four stages of two files per XCD
// cannot fill 64 slots, spread or not.
static int chain_list_mode(int batch) {
    const int key = gccnmf_tune_chain_rag;
    if (key == 0 || key == 2) return key;
    if (key == 3) return 1;
    const int longest = (batch + 7) / 8;
    return 1000L * 8 * longest <= 1027L * batch ? 1 : 2;
}
// Which iterations can be chained -- the shape and tuning conditions of any chained launch: the four GEMMs all on full-height LDS-DMA throughput
// tiles (K2 half-height up to 256 atoms) with one XCD-affine list per XCD, enough column tiles (64 columns, all files) to fill the chip, not `latency`
// (direct_path).  (gccnmf_klnmf asks more -- plan_klnmf; a ragged batch has no plain form to agree with and asks this alone.)
static bool chain_capable(const NmfGeom& g, int batch, const KlnmfMode& m, bool latency, long column_tiles) {
    if (!gccnmf_tune_chain || !gccnmf_tune_dma || gccnmf_tune_tile_policy == 2 || gccnmf_tune_tail_split > 1) return false;
    if (latency || !m.xcd_affine || m.unfused_w_update || batch < 8) return false;
    // (K a multiple of 128: a K2 tile whose last wave is partly beyond M takes the generic epilogue h * (acc / den) for that wave, a plain
    // launch on half-height tiles the lean one (h * acc) * (s / den) for the same rows: a few ulp apart, so the forms would not be bitwise equal)
    if (g.K <= 128 || g.Fm <= 128 || g.Fm > 512 || (g.Fm & 127) || (g.K & 127) || (g.F % 16) != 1 || !g.tail) return false;
    return gccnmf_tune_tile_policy == 1 || column_tiles >= 256;      // (fewer: the small-batch tile's territory)
}
static bool chain_rule(int batch, const KlnmfMode& m) {
    // The rule (profiles/r06h_files_sweep_*.txt, one-stream iteration as a fraction of the f32 peak, plain launches -> whole-call chain):
    //   24 files 0.74 -> 0.78, 32: 0.81 -> 0.85, 40: 0.73 -> 0.86, 64: 0.83 -> 0.86, 72: 0.79 -> 0.86, 104: 0.80 -> 0.86 -- but 16 files (two per XCD:
    //   the four stages of so few files cannot fill 64 slots): 0.75 -> 0.59, and with whole-file lists the longest list sets the pace: 25
    //   files (4 on one XCD, 3 on the others) 0.77 -> 0.68, 51: a tie, 52 (7 | 6): 0.75 -> 0.80.  So: at least three files per XCD and a longest
    //   list at most 8 % above the mean.  Not beside another file group's launches (GCCNMF_FLAG_CONCURRENT_GROUPS): two chained launches that
    //   share the chip are slower than two plain ones (155 k against 158 k frames/s end to end).
    if (m.groups > 1) return false;
    const int longest = (batch + 7) / 8;
    return batch >= 24 && 100L * 8 * longest <= 108L * batch;
}
// ---- which launches a per-file-dictionary call is made of, decided ONCE at the entry point (gccnmf_klnmf / _stage / _plan / _ragged) ---------
// plan_klnmf is the only code that reads the form-selecting tuning keys and shape rules; klnmf_stage and the call loops test these fields and no rule.
enum KlnmfKind { KLNMF_BLIND, KLNMF_FIXED_W, KLNMF_FREE_ATOMS, KLNMF_BETA, KLNMF_SMOOTH };      // W learned | one given W (GCCNMF_FLAG_FIXED_W) | free atoms beside a dictionary | IS / Euclid | temporal continuity
struct KlnmfPlan {
    KlnmfKind kind;
    bool direct;            // every stage on the direct latency kernels (direct.hip)
    bool fused12;           // K1 + K2 in one launch: stage 1 runs it, stage 2 has nothing to do
    int head34;             // files (from the front of the batch) on the K3 + K4a slab launch of stage 3; the rest on the two launches behind it
    bool w_in_rht;          // the W update rides in stage 4's epilogue: stage 5 has nothing to do
    int chain;              // 0 | 2: K1 | K2 in one chained launch | 4: the whole iteration | 8: the whole call
    int short_group;        // K <= 128: the three launches of every iteration as one chained launch -- atoms per W-update group (16 | 32), 0 = no chain
};
static KlnmfPlan plan_klnmf(const NmfGeom& g, int batch, const KlnmfMode& m) {
    KlnmfPlan p = {};
    p.kind = m.fixed_w ? KLNMF_FIXED_W : m.free_atoms ? KLNMF_FREE_ATOMS : KLNMF_BLIND;
    if (p.kind == KLNMF_FIXED_W) return p;      // one launch runs every iteration (nmf_fixed.hip); of the stages only 7 exists, in one form
    if (m.divergence) {                         // IS / Euclid: five plain launches per iteration in ONE form (nmf_beta.hip), no tuning key is read
        p.kind = KLNMF_BETA;
        return p;
    }
    if (m.segments) {                           // temporal continuity: plain launches in ONE form (nmf_smooth.hip), R materialised, no tuning key is read
        p.kind = KLNMF_SMOOTH;
        return p;
    }
    // Free atoms (semi-supervised): stage 4 reads a materialised R [batch][Fp][Np] with zero padding, so stages 1-3 take the forms that leave
    // one in the workspace whatever the tuning keys say -- never the direct kernels (they keep Rt), never the K3 + K4a slab launch.  K1 + K2
    // fused stays: stage 3 rewrites R.  Stages 4 and 5 are nmf_semi.hip's, on the free columns alone.  Nothing chains.
    const bool semi = p.kind == KLNMF_FREE_ATOMS;
    const int groups = m.groups;      // launch forms that follow the launch size are chosen for all groups together (GCCNMF_FLAG_GROUPS)
    const bool latency = direct_path(g, batch, groups);
    const int want = gccnmf_tune_chain;
    p.direct = latency && !semi;
    // the shapes of the short-dictionary kernels (direct.hip), and of them those whose W rows fit the registers of the K3 + K4a slab workgroups
    const bool short_shape = gccnmf_tune_tile_policy == 0 && !latency && batch >= 2 && g.tail && g.Fm >= 64 && g.Fm <= 512 && (g.Fm % 64) == 0 && g.K <= 128;
    const bool slab_shape = short_shape && (g.Fm / 64) * 16 >= 32 * gccnmf_ceil_div(g.K, 32);
    // Short dictionaries (K <= 128 -- the reference driver's K = 128): K1 and K2 as ONE launch (gccnmf_wh_updh_kernel: a workgroup per
    // 64-frame column tile with its scaled H resident in registers, W in 64-bin chunks through LDS), R never written.
    // Measured at K = 128, N = 1244 (profiles/r04w_fused_k12_sweep.txt; files: fused / two launches, us): 20: 82 / 92, 25: 86 / 109, 26: 127 / 123,
    // 40: 153 / 186, 50: 160 / 189, 64: 208 / 240, 96: 312 / 333, 128: 379 / 431; K = 64, 64 files: 116 / 195.  A full round of 512 workgroups
    // (two per CU) takes 78 us, a last round of at most 256 (one per CU) 45, a larger one 76; the two launches 25 + 0.17 us per column tile.
    // Both scale alike with K, so the choice is made in those units.  (GCCNMF_FLAG_GROUPS: the file groups that run side by side are priced together.)
    if (short_shape && gccnmf_tune_fused_k12) {
        const long wgs = (long)batch * gccnmf_ceil_div(g.N, 64) * groups, rem = wgs % 512;
        const long fused = 780 * (wgs / 512) + (rem == 0 ? 0 : rem <= 256 ? 450 : 760), two = 250 + 17 * wgs / 10;      // tenths of a microsecond
        p.fused12 = fused < two || gccnmf_tune_fused_k12 == 2;
    }
    // K3 and K4a as ONE launch (gccnmf_whdiv_rht_kernel: 64-bin slabs with their W rows in registers), K <= 128.
    // Every slab workgroup walks ALL column tiles of its file, so the launch costs one "round" (two workgroups per CU, 512 at a time) however
    // few workgroups it holds: measured at K = 128, N = 1244 a round takes 184 us against 3.72 us per file for the two launches it replaces
    // (64 files: 184 against 238 us; 40 files: 184 against 149).  Both scale alike with K and N, so the choice is a ratio.  head34 is the number of
    // files (from the front of the batch) that take the slab launch: all of them, none, or whole rounds' worth with the REST of the files on
    // the two launches behind it (72 files: 64 + 8 -> 184 + 40 us against 268 for the two launches over all of them, 368 for two slab rounds).
    // (GCCNMF_FLAG_GROUPS: the file groups that run side by side share the rounds; they are not split.)
    if (slab_shape && !semi && gccnmf_tune_fused_k34) {
        const long slabs = g.Fm / 64, wgs = (long)batch * slabs * groups, rounds = (wgs + 511) / 512;
        const long per_round = 512 / slabs;                          // files per round
        // in hundredths of a microsecond: 3.72 us x slabs / 8 per file on the two launches, 184 us per round, 10 us for the extra launch pair
        const long two = 372 * slabs / 8;
        long best = two * batch * groups, head = 0;                  // all files on the two launches
        if (18400 * rounds < best) {
            best = 18400 * rounds;
            head = batch;
        }
        if (groups == 1) {
            const long r = batch / per_round;                        // whole rounds of files, the rest behind them on the two launches
            // (+ 10 %: the two launches are dearer per file on a small rest than the straight line says -- 104 files: 64 + 40 measured 717 us
            // per iteration against 699 for two slab rounds)
            if (r >= 1 && r * per_round < batch && 11 * (18400 * r + two * (batch - r * per_round) + 1000) < 10 * best) head = r * per_round;
        }
        p.head34 = gccnmf_tune_fused_k34 == 2 ? batch : (int)head;
    }
    // K4a + K4b in one launch (launch_rht_update_w): the fused epilogue needs the tall tile; tiny launches prefer the small-batch tile and two launches
    const bool tall_tile = gccnmf_tune_tile_policy == 1 || (gccnmf_tune_tile_policy == 0 && (long)batch * groups * gccnmf_ceil_div(g.K, 64) >= 256);
    p.w_in_rht = g.Fm > 128 && g.Fm <= 512 && tall_tile && !m.unfused_w_update && !p.head34 && !semi && !p.direct;

    // The chained launches: bit for bit the plain call, which is why they are derived from the fields above.  K > 128: a plain launch of a few files
    // takes the two-launch W update -- other kernels, other summation order -- so the call chains only where the plain one has the W update in K4's
    // epilogue.  Every file's tiles on ONE XCD in every stage (batch a multiple of 8: list x holds the files x, x + 8, ...) unless the lists say otherwise.
    if (p.w_in_rht && chain_capable(g, batch, m, latency, (long)batch * gccnmf_ceil_div(g.N, 64)) && !((batch & 7) && chain_list_mode(batch) == 0)) {
        // a forced form, or by rule: not beside another file group's launches (two chained launches that share the chip are slower than two plain ones:
        // 155 k against 158 k frames/s end to end); whole-file lists from three files per XCD on, spread lists from 20 files on
        p.chain = want != 1 ? want : groups == 1 && batch >= (chain_list_mode(batch) == 1 ? 24 : 20) ? 8 : 0;
    }
    // Short dictionaries (K <= 128): the three launches of an iteration -- K1 + K2 on column tiles, K3 + K4a on bin slabs, the one-pass W update --
    // chained the same way (direct.hip: gccnmf_short_chain_kernel).  Shapes both fused kernels and the one-pass W update take; the same batch
    // rule as the throughput chain.  short_group: the atoms per W-update group (16 / 32: what the plain launch would use at this batch).
    if (!p.chain && !semi && (want == 1 || want == 8) && slab_shape && gccnmf_tune_fused_k12 && gccnmf_tune_fused_k34 && m.xcd_affine &&
        !m.unfused_w_update && batch >= 8 && g.F <= 64 * 9 && (long)batch * (g.Kp / 64) < 256) {
        // by rule: only where the plain call runs the SAME three item programs for every file (both fused launches, no files left to the two-launch
        // form) -- the chained call is then bit for bit the plain one, and a file's bits keep following the batch size exactly as before
        if (want == 8 || (chain_rule(batch, m) && p.fused12 && p.head34 == batch))
            p.short_group = (long)batch * (g.Kp / 32) >= 256 ? 32 : 16;
    }
    return p;
}

// A ragged batch (gccnmf_klnmf_ragged): files of different lengths in ONE chained launch.  g is the geometry of the LONGEST file (every file's V, H,
// R live in blocks of that pitch); n[f] = the file's own column count.  The host deals the files out to the eight XCD lists (longest first, each to
// the list with the least work so far); the device tables sit behind the status words in the workspace.
struct RaggedPlan {
    const int* n;                                   // host [batch]
    int lists[8][GEMM_RAGGED_LMAX + 1];             // host: count, files
    const int* d_n;                                 // device copies
    const int* d_lists;
};

// stages: 2 = K1 | K2, 4 = the four GEMMs; iterations [it0, it0 + iterations) in one launch; rg: the lists of a ragged batch, else nullptr
static int launch_klnmf_chain(int stages, const NmfGeom& g, const float* V, float* W, float* H, const KlnmfWorkspace& ws, float alpha, float eps,
                              int batch, const KlnmfMode& m, int it0, int iterations, hipStream_t s, const RaggedPlan* rg) {
    const int concurrent = m.groups > 1 ? 1 : 0;      // (intended today: a chained launch says THAT other groups run beside it, not how many)
    // the operands of the plain launches, from the same builders (K1 with the pending row scale of H on the B fragments, K3 without)
    GemmArgs a[4] = {wh_div_args(g, V, W, g.sW, H, ws.hscale, g.Kp, ws.R, batch, 1, concurrent),
                     update_h_args(g, W, g.sW, ws.R, H, ws.hscale, g.Kp, ws.colsumW, g.Kp, alpha, eps, batch, 1, concurrent),
                     wh_div_args(g, V, W, g.sW, H, nullptr, 0, ws.R, batch, 1, concurrent),
                     rht_update_w_args(g, ws.R, H, W, ws.colsumW, ws.hscale, batch, 1, concurrent)};
    for (GemmArgs& x : a) x.exact_div = gccnmf_tune_exact_div;
    const int tm1 = g.K <= 256 ? 2 : 4;            // K2's outputs are the K atoms: at most 256 rows -> half-height tiles, as in a plain launch
    GemmChain ch = {};
    for (int i = 0; i < 4; ++i) {
        int len = 0;
        if (i < stages) {
            // whole-file lists (key 23, default): any batch size, K4 never waits for a ragged K3 item at the end of a list
            const int tm = (i == 1 && tm1 == 2) ? 2 : 4;
            int grid = gemm_dma_plan(a[i], i != 3 && tm == 4, tm, rg ? 1 : chain_list_mode(batch));      // 0: the plain launch's lists | 1: whole files | 2: file-major equal eighths
            if (grid < 8 || a[i].lists != 8 || a[i].split) return GCCNMF_ERR_ARG;
            if (rg) {
                // per list: the sum over its files of tiles_m x the file's own column tiles (K4: the uniform atom tiles, the file's own reduction length)
                a[i].ragged_n = rg->d_n; a[i].ragged_lists = rg->d_lists; a[i].ragged_kd = i == 3 ? 1 : 0;
                long longest = 0;
                for (int l = 0; l < 8; ++l) {
                    long items = 0;
                    for (int k = 0; k < rg->lists[l][0]; ++k)
                        items += (long)a[i].tiles_m * (i == 3 ? a[i].tiles_n : gccnmf_ceil_div(rg->n[rg->lists[l][1 + k]], 64));
                    if (items > longest) longest = items;
                }
                if (longest < 1 || longest > (1L << 24)) return GCCNMF_ERR_ARG;
                a[i].cw = (int)longest;
                grid = 8 * a[i].cw;
            }
            len = grid / 8;
        }
        ch.first[i + 1] = ch.first[i] + len;
    }
    const int tn = gccnmf_ceil_div(g.N, 64);
    unsigned *c12 = ws.c12, *c23 = ws.c23, *c34 = ws.c34, *c41 = ws.c41;
    const bool wide = !rg && chain_list_mode(batch) == 2;          // a file's tiles spread over the XCDs: agent-scope hand-over, no XCC check
    for (int i = 0; i < 4; ++i) {
        ch.sync[i].error = ws.status;
        ch.sync[i].timeout = gccnmf_tune_chain_fault ? 0 : GEMM_SYNC_TIMEOUT;      // (lab build, key 25: every consumer that has to wait gives up at once)
        ch.sync[i].xcc_seen = wide ? nullptr : ws.xcc_seen;
        ch.sync[i].wide = wide ? 1 : 0;
    }
    // does a producer run a file's ragged last column tile as ONE narrow item?  (a uniform batch: decided for the launch; a ragged one: per file)
    auto narrow_items = [&](int i) { return rg ? a[i].narrow_ok : (a[i].rag ? 1 : 0); };
    // K1 -> K2: column tile j of a file is ready when its 32-column blocks (2; the ragged last tile as ONE narrow item: 1) are stored
    ch.sync[0].sig_cnt = c12; ch.sync[0].sig_stride = tn; ch.sync[0].sig_per_tile = 1;
    ch.sync[1].wait_cnt = c12; ch.sync[1].wait_stride = tn; ch.sync[1].wait_per_tile = 1;
    ch.sync[1].wait_need = 2u; ch.sync[1].prod_narrow = narrow_items(0);
    if (stages == 4) {
        // K2 -> K3: both atom tiles (tiles_m of K2) of column tile j;  K3 -> K4: every item of the file
        ch.sync[1].sig_cnt = c23; ch.sync[1].sig_stride = tn; ch.sync[1].sig_per_tile = 1;
        ch.sync[2].wait_cnt = c23; ch.sync[2].wait_stride = tn; ch.sync[2].wait_per_tile = 1;
        ch.sync[2].wait_need = 2u * a[1].tiles_m; ch.sync[2].prod_narrow = narrow_items(1);
        ch.sync[2].sig_cnt = c34; ch.sync[2].sig_stride = 1; ch.sync[2].sig_per_tile = 0;
        ch.sync[3].wait_cnt = c34; ch.sync[3].wait_stride = 1; ch.sync[3].wait_per_tile = 0;
        ch.sync[3].wait_need = (unsigned)(a[2].tiles_m * (rg ? 1 : a[2].tiles_n));
        ch.sync[3].wait_scale_tiles = rg ? 1 : 0;
        {
            // K4 -> the next iteration's K1 (also across launches: a call of very many iterations is a few chained launches, and forced per-iteration
            // launches keep counting -- the kernel boundary makes the wait trivially true there): every atom tile of the file (W, its column sums and the pending row scale are complete; R is free)
            ch.sync[3].sig_cnt = c41; ch.sync[3].sig_stride = 1; ch.sync[3].sig_per_tile = 0;
            ch.sync[0].wait_cnt = c41; ch.sync[0].wait_stride = 1; ch.sync[0].wait_per_tile = 0; ch.sync[0].wait_lag = 1;
            ch.sync[0].wait_need = (unsigned)(a[3].tiles_m * a[3].tiles_n);
        }
    }
    if (iterations > 1 && stages != 4) return GCCNMF_ERR_ARG;
    if (it0 == 0 && iterations == 1) ch.sync[0].wait_cnt = nullptr;      // (nothing to wait for: the counters were just zeroed)
    ch.it0 = it0; ch.iterations = iterations;
    ch.trace_it = it0 + (iterations > 4 ? iterations - 3 : iterations - 1);      // timeline builds: an iteration in the steady state of a whole-call launch, not its last
    if ((long)8 * ch.first[4] * iterations > (1L << 30)) return GCCNMF_ERR_ARG;
    for (int i = 0; i < stages; ++i) {           // timeline builds (gccnmf_debug_set_trace): stage i's item t of list x -> row 8 * (first[i] + t) + x
        a[i].trace = gccnmf_trace_buf ? gccnmf_trace_buf + 8L * 8 * ch.first[i] : nullptr;
        a[i].trace_rows = gccnmf_trace_buf ? gccnmf_trace_blocks - 8 * ch.first[i] : 0;
        if (a[i].trace_rows <= 0) a[i].trace = nullptr;
    }
    const int grid = 8 * ch.first[4] * iterations;
    const unsigned pad = gccnmf_tune_chain_solo ? 16384u : 0u;         // static 78 KB + 16 KB: one workgroup per CU
    if (!g.tail) return GCCNMF_ERR_ARG;
    if (stages == 2 && tm1 == 4) hipLaunchKernelGGL((gccnmf_gemm_chain_kernel<true, 2, 4>), dim3(grid), dim3(256), pad, s, a[0], a[1], a[2], a[3], ch);
    else if (stages == 2) hipLaunchKernelGGL((gccnmf_gemm_chain_kernel<true, 2, 2>), dim3(grid), dim3(256), pad, s, a[0], a[1], a[2], a[3], ch);
    else if (tm1 == 4) hipLaunchKernelGGL((gccnmf_gemm_chain_kernel<true, 4, 4>), dim3(grid), dim3(256), pad, s, a[0], a[1], a[2], a[3], ch);
    else hipLaunchKernelGGL((gccnmf_gemm_chain_kernel<true, 4, 2>), dim3(grid), dim3(256), pad, s, a[0], a[1], a[2], a[3], ch);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

// the short-dictionary chain (plan_klnmf: short_group = `group`), iterations [it0, it0 + iterations) in one launch
static int launch_short_chain(const NmfGeom& g, const float* V, float* W, float* H, const KlnmfWorkspace& ws, float alpha, float eps, int batch,
                              int group, int it0, int iterations, hipStream_t s) {
    ShortChainArgs c = {};
    // the arguments of the three plain launches, from the same builders
    c.a12 = wh_updh_args(g, V, W, H, ws.hscale, ws.colsumW, alpha, eps, batch);
    c.a34 = whdiv_rht_args(g, V, W, H, ws.U, ws.rowsumH, batch);
    c.aw = update_w_args(g, W, g.sW, ws.U, g.sU, ws.rowsumH, ws.colsumW, ws.hscale, g.Kp);
    c.it0 = it0; c.iterations = iterations; c.atoms_per_group = group; c.solo = gccnmf_tune_chain_solo;
    c.counters = ws.c12;
    c.error = ws.status;
    c.xcc_seen = ws.xcc_seen;
    c.timeout = gccnmf_tune_chain_fault ? 0 : GEMM_SYNC_TIMEOUT;
    return gccnmf_short_chain_launch(c, s);
}

// a consumer gave up waiting (GEMM_SYNC_TIMEOUT), or the workgroups of a list were NOT all on one XCD (the data hand-over through that XCD's
// L2 is then not guaranteed): the factors cannot be trusted -- make them NaN so that nothing downstream looks plausible
__global__ void nmf_chain_poison_kernel(const unsigned* __restrict__ err, float* __restrict__ W, float* __restrict__ H, long nW, long nH) {
    bool bad = err[0] != 0u;
    for (int l = 0; l < 8; ++l) bad = bad || __popc(err[GCCNMF_STATUS_XCC_SEEN + l]) > 1;
    if (!bad) return;
    const float nan = __int_as_float(0x7fc00000);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < nW; i += 256L * gridDim.x) W[i] = nan;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < nH; i += 256L * gridDim.x) H[i] = nan;
}

extern "C" {

// the end of the carve (KlnmfWorkspace states the layout)
long gccnmf_klnmf_workspace_floats(int F, int N, int K, int batch) {
    GCCNMF_ENTER();
    if (F < 2 || N < 1 || K < 1 || batch < 1) return -1;
    return carve(nullptr, make_geom(F, N, K), batch, false).floats;
}

// One launch group of the iteration, addressable on its own so that tests and the benchmark can time / check each kernel in isolation; which form
// it takes, and whether another stage has done its work, the plan says.  stage: 0 prepare | 1 K1 | 2 K2 | 3 K3 | 4 K4a | 5 K4b | 6 final H rescale | 7 KL divergence of the current factors
static int klnmf_stage(int stage, const float* V, float* W, float* H, const KlnmfWorkspace& ws, const NmfGeom& g, int batch, float alpha, float eps,
                       const KlnmfMode& m, const KlnmfPlan& p, hipStream_t s) {
    float *R = ws.R, *U = ws.U, *colsumW = ws.colsumW, *rowsumH = ws.rowsumH, *hscale = ws.hscale;
    if (stage == 7) {
        // D(V || W.H) of the current (materialised) factors, divergence.hip: tile partials (float64) in each file's R block, the batch
        // results (float64) at the start of the U region; one launch form whatever the batch or the tuning.  V, W, H are read only.
        // (float64 partials and results: the workspace is 16-byte aligned -- the entry point checked -- and both offsets are multiples of 4096 bytes)
        return gccnmf_kl_divergence_launch(V, W, p.kind == KLNMF_FIXED_W ? 0 : g.sW, H, g.F, g.N, g.K, g.Fp, g.Kp, g.Np, batch, (double*)R, g.sV / 2, (double*)U, s,
                                           m.divergence);
    }
    if (p.kind == KLNMF_BETA && stage != 6) {      // (stage 6 is the same launch on every path: below)
        const BetaWorkspace bw = carve_beta(R, ws, g, batch);      // (R is the start of the workspace)
        if (stage == 0) {
            // R and Q are zero outside f < F, n < N from here on (stages 1 and 3 rewrite the whole padded blocks); colsumW, hscale = 1 as for KL
            if (hipMemsetAsync(R, 0, sizeof(float) * batch * g.sV, s) != hipSuccess) return GCCNMF_ERR_LAUNCH;
            if (hipMemsetAsync(bw.Q, 0, sizeof(float) * batch * g.sV, s) != hipSuccess) return GCCNMF_ERR_LAUNCH;
            hipLaunchKernelGGL(nmf_prepare_kernel, dim3(batch * (g.Kp / 16)), dim3(256), 0, s, W, colsumW, hscale, g.F, g.Fp, g.Kp);
            GCCNMF_CHECK_LAUNCH();
            return GCCNMF_OK;
        }
        return gccnmf_klnmf_beta_stage_launch(stage, m.divergence, V, W, H, R, bw.Q, U, bw.Ud, colsumW, hscale, g.F, g.N, g.K, batch, alpha, eps, s);
    }
    if (p.kind == KLNMF_SMOOTH && stage >= 1 && stage <= 5) {      // (stages 0 and 6 are the KL launches below)
        if (stage == 5) {      // the two-pass W update on 16 atoms per workgroup, whatever the batch: a file's bits do not follow the launch size
            hipLaunchKernelGGL(nmf_update_w_kernel<16>, dim3(batch * (g.Kp / 16)), dim3(256), 0, s, W, U, rowsumH, colsumW, hscale, g.F, g.Fp, g.K, g.Kp,
                               g.sW, g.sU, (long)g.Kp, (long)g.Kp);
            GCCNMF_CHECK_LAUNCH();
            return GCCNMF_OK;
        }
        const SmoothWorkspace sw = carve_smooth(R, ws, g, batch);      // (R is the start of the workspace)
        return gccnmf_klnmf_smooth_stage_launch(stage, V, W, H, R, U, rowsumH, colsumW, hscale, sw.Gm, sw.Gp, sw.E, sw.D, g.F, g.N, g.K, batch, m.segments,
                                                alpha, eps, m.continuity, s);
    }
    const int nfree = m.free_atoms, groups = m.groups;      // (GCCNMF_FLAG_GROUPS: the W update kernel is sized for all groups together)
    const bool semi = p.kind == KLNMF_FREE_ATOMS;
    const int head34 = p.head34, rest34 = batch - head34;      // files on the slab launch | behind it on the two launches
    if (p.direct && stage != 6) {      // (stage 6 is the same launch on every path: below)
        const DirectBufs d = direct_bufs(g, ws.direct_base, batch);
        switch (stage) {
            case 0: {
                // zero: R's padding (reduction operand of K2), Rt / Ht rows n >= N (reduction operands of K4), Wt columns f >= F
                if (hipMemsetAsync(R, 0, sizeof(float) * batch * g.sV, s) != hipSuccess) return GCCNMF_ERR_LAUNCH;
                if (hipMemsetAsync(d.Wt, 0, sizeof(float) * direct_floats(g, batch), s) != hipSuccess) return GCCNMF_ERR_LAUNCH;
                hipLaunchKernelGGL(nmf_prepare_kernel, dim3(batch * (g.Kp / 16)), dim3(256), 0, s, W, colsumW, hscale, g.F, g.Fp, g.Kp);
                GCCNMF_CHECK_LAUNCH();
                return gccnmf_transpose_launch(W, g.sW, g.Kp, d.Wt, d.sWt, d.ldwt, g.F, g.Kp, batch, s);
            }
            case 1: return direct_wh_div(g, d, V, W, H, hscale, R, false, batch, s);
            case 2: return direct_update_h(g, d, W, R, H, hscale, colsumW, alpha, eps, batch, s);
            case 3: return direct_wh_div(g, d, V, W, H, nullptr, R, true, batch, s);
            case 4: return direct_rht(g, d, R, U, rowsumH, batch, s);
            case 5: return launch_update_w(update_w_args(g, W, g.sW, U, g.sU, rowsumH, colsumW, hscale, g.Kp), batch, groups, s, d.Wt, d.sWt, d.ldwt);
            default: return GCCNMF_ERR_ARG;
        }
    }
    const int xa = m.xcd_affine, conc = m.groups > 1 ? m.groups : 0;      // GemmArgs.concurrent: the file groups whose launches run side by side (0: this one alone)
    const int vec_grid = batch * (g.Kp / 16);
    switch (stage) {
        case 0:
            // R's padding (rows >= F, columns >= N) must be zero: it is a reduction operand of K2 and K4a.
            if (hipMemsetAsync(R, 0, sizeof(float) * batch * g.sV, s) != hipSuccess) return GCCNMF_ERR_LAUNCH;
            hipLaunchKernelGGL(nmf_prepare_kernel, dim3(vec_grid), dim3(256), 0, s, W, colsumW, hscale, g.F, g.Fp, g.Kp);
            break;
        case 1:
            if (p.fused12) return gccnmf_wh_updh_launch(wh_updh_args(g, V, W, H, hscale, colsumW, alpha, eps, batch), s);    // K1 + K2
            return launch_wh_div(g, wh_div_args(g, V, W, g.sW, H, hscale, g.Kp, R, batch, xa, conc), s);
        case 2:
            if (p.fused12) return GCCNMF_OK;                                                                             // done by stage 1
            return launch_update_h(update_h_args(g, W, g.sW, R, H, hscale, g.Kp, colsumW, g.Kp, alpha, eps, batch, xa, conc), s);
        case 3:
            if (head34) {                                                                                              // K3 + K4a
                const int rc = gccnmf_whdiv_rht_launch(whdiv_rht_args(g, V, W, H, U, rowsumH, head34), s);
                if (rc || !rest34) return rc;
                return launch_wh_div(g, wh_div_args(g, V + head34 * g.sV, W + head34 * g.sW, g.sW, H + head34 * g.sH, nullptr, 0, R + head34 * g.sV, rest34, xa, conc), s);
            }
            return launch_wh_div(g, wh_div_args(g, V, W, g.sW, H, nullptr, 0, R, batch, xa, conc), s);
        case 4:
            if (semi) return gccnmf_klnmf_semi_rht_launch(R, H, U, rowsumH, g.F, g.N, g.K, nfree, batch, s);           // U[:, K - n:], rowsumH[K - n:]
            if (head34)                                                                                                // done by stage 3 ...
                return rest34 ? launch_rht(g, rht_args(g, R + head34 * g.sV, H + head34 * g.sH, U + head34 * g.sU, rowsumH + (long)head34 * g.Kp, rest34, xa, conc), s)
                              : GCCNMF_OK;                                                                             // ... but for the rest
            if (p.w_in_rht)                                                                                            // K4a + K4b
                return launch_rht_update_w(g, rht_update_w_args(g, R, H, W, colsumW, hscale, batch, xa, conc), s);
            return launch_rht(g, rht_args(g, R, H, U, rowsumH, batch, xa, conc), s);
        case 5:
            if (semi) return gccnmf_klnmf_semi_update_w_launch(W, U, rowsumH, colsumW, hscale, g.F, g.K, nfree, batch, s);
            if (p.w_in_rht) return GCCNMF_OK;                                                                          // done by stage 4's epilogue
            return launch_update_w(update_w_args(g, W, g.sW, U, g.sU, rowsumH, colsumW, hscale, g.Kp), batch, groups, s, nullptr, 0, 0);
        case 6:
            hipLaunchKernelGGL(nmf_scale_h_kernel, dim3(batch * g.K), dim3(256), 0, s, H, hscale, (long)g.Kp, g.K, g.sH, g.ld, g.Np);
            break;
        default: return GCCNMF_ERR_ARG;
    }
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

// ---- the prologue and the epilogue of a call --------------------------------------------------------------------------------------
// The status words describe THIS call (gccnmf_klnmf_chain_status): a call that does not chain clears what an earlier, chained one may have left.
static int clear_chain_status(const KlnmfWorkspace& ws, hipStream_t s) {
    return hipMemsetAsync(ws.status, 0, GCCNMF_STATUS_WORDS * sizeof(unsigned), s) == hipSuccess ? GCCNMF_OK : GCCNMF_ERR_LAUNCH;
}
// A call that chains starts its ready counters at zero, once (and with them the status words behind them).
static int zero_chain_counters(const KlnmfWorkspace& ws, hipStream_t s) {
    return hipMemsetAsync(ws.c12, 0, sizeof(unsigned) * ws.counter_words, s) == hipSuccess ? GCCNMF_OK : GCCNMF_ERR_LAUNCH;
}
// The end of every iterating call: W and H become NaN if a chained launch of this call failed to hand over (the call is never silent about it),
// then stage 6 materialises the pending row scale of H.
static int finish_call(bool chained, const float* V, float* W, float* H, const KlnmfWorkspace& ws, const NmfGeom& g, int batch, float alpha, float eps,
                       const KlnmfMode& m, const KlnmfPlan& p, hipStream_t s) {
    if (chained) {
        hipLaunchKernelGGL(nmf_chain_poison_kernel, dim3(64), dim3(256), 0, s, ws.status, W, H, (long)batch * g.sW, (long)batch * g.sH);
        GCCNMF_CHECK_LAUNCH();
    }
    return klnmf_stage(6, V, W, H, ws, g, batch, alpha, eps, m, p, s);
}

// Which launches gccnmf_klnmf would use for this problem under the current tuning: bit 0 the direct latency kernels, bit 1 the fused
// K1 + K2 launch, bit 2 the fused K3 + K4a slab launch, bit 3 chained launches of the iteration (benchmarks and tests name the kernel they
// time by this; the engine keeps ONE file group when the library chains), bit 4 the fused fixed-dictionary launch (GCCNMF_FLAG_FIXED_W),
// bit 5 the semi-supervised iteration (GCCNMF_FLAG_FREE_ATOMS), bit 6 the IS / Euclidean iteration (GCCNMF_FLAG_DIVERGENCE_*), bit 7 the
// temporal-continuity iteration (GCCNMF_FLAG_CONTINUITY; bits 4, 5, 6 and 7: then no other bit).
int gccnmf_klnmf_plan(int F, int N, int K, int batch, int flags) {
    GCCNMF_ENTER();
    KlnmfMode m;
    if (unpack_continuity(flags, N, K, batch, m)) return -1;
    if (F < 2 || N < 1 || K < 1 || batch < 1) return -1;
    if (decode_mode(flags, F, K, m)) return -1;
    const KlnmfPlan p = plan_klnmf(make_geom(F, N, K), batch, m);
    if (p.kind == KLNMF_FIXED_W) return gccnmf_klnmf_fixed_supported(F, K) ? 16 : -1;
    if (p.kind == KLNMF_FREE_ATOMS) return 32;
    if (p.kind == KLNMF_BETA) return 64;
    if (p.kind == KLNMF_SMOOTH) return 128;
    return (p.direct ? 1 : 0) | (p.fused12 ? 2 : 0) | (p.head34 > 0 ? 4 : 0) | ((p.chain || p.short_group) ? 8 : 0);
}

int gccnmf_klnmf_stage(const float* V, float* W, float* H, float* workspace, int F, int N, int K, int batch,
                       float sparsity_alpha, float epsilon, int flags, int stage, void* stream) {
    GCCNMF_ENTER();
    KlnmfMode m;
    if (const int rc = unpack_continuity(flags, N, K, batch, m)) return rc;
    if (!V || !W || !H || !workspace || F < 2 || N < 1 || K < 1 || batch < 1) return GCCNMF_ERR_ARG;
    if (!workspace_aligned(workspace)) return GCCNMF_ERR_ARG;          // float4 / LDS-DMA accesses to its blocks; stage 7's float64 partials and results
    if (const int rc = decode_mode(flags, F, K, m)) return rc;
    // (a fixed dictionary -- one W for every file -- exists for stage 7 alone: the divergence against it; the iteration stages have no such form)
    if (m.fixed_w && (stage != 7 || m.h_ones)) return GCCNMF_ERR_ARG;
    const NmfGeom g = make_geom(F, N, K);
    return klnmf_stage(stage, V, W, H, carve(workspace, g, batch, false), g, batch, sparsity_alpha, epsilon, m, plan_klnmf(g, batch, m), (hipStream_t)stream);
}

int gccnmf_klnmf(const float* V, float* W, float* H, float* workspace, int F, int N, int K, int batch, int iterations,
                 float sparsity_alpha, float epsilon, int flags, void* stream) {
    GCCNMF_ENTER();
    KlnmfMode m;
    int rc;
    if ((rc = unpack_continuity(flags, N, K, batch, m))) return rc;
    if (!V || !W || !H || !workspace || F < 2 || N < 1 || K < 1 || batch < 1 || iterations < 0) return GCCNMF_ERR_ARG;
    if (!workspace_aligned(workspace)) return GCCNMF_ERR_ARG;          // R, U, Wt, Ht, Rt are read with float4 loads and LDS-DMA: 16 bytes
    hipStream_t s = (hipStream_t)stream;
    if ((rc = decode_mode(flags, F, K, m))) return rc;
    const NmfGeom g = make_geom(F, N, K);
    const KlnmfPlan p = plan_klnmf(g, batch, m);
    const KlnmfWorkspace ws = carve(workspace, g, batch, false);
    const float alpha = sparsity_alpha, eps = epsilon;
    if (p.kind == KLNMF_FREE_ATOMS || p.kind == KLNMF_BETA || p.kind == KLNMF_SMOOTH) {
        // IS / Euclid: five plain launches per iteration (nmf_beta.hip); nothing chains.
        // temporal continuity: seven plain launches per iteration (nmf_smooth.hip and the two-pass W update); nothing chains.
        // semi-supervised: the dictionary in W[:, :K - n] of every file stays as it is, the n free atoms behind it and all of H are learned.
        // Plain launches (klnmf_stage keeps R materialised); nothing chains.
        if ((rc = clear_chain_status(ws, s))) return rc;
        if ((rc = klnmf_stage(0, V, W, H, ws, g, batch, alpha, eps, m, p, s))) return rc;
        for (int it = 0; it < iterations; ++it)
            for (int stage = 1; stage <= 5; ++stage)
                if ((rc = klnmf_stage(stage, V, W, H, ws, g, batch, alpha, eps, m, p, s))) return rc;
        return finish_call(false, V, W, H, ws, g, batch, alpha, eps, m, p, s);
    }
    if (p.kind == KLNMF_FIXED_W) {
        // fixed dictionary: W is read only, H holds the initial coefficients (or, with H_ONES, is output only); one launch runs every
        // iteration (and leaves H materialised).  Nothing chains.
        if (!gccnmf_klnmf_fixed_supported(F, K) || gccnmf_klnmf_fixed_workspace_floats(F, K) > ws.scratch_floats) return GCCNMF_ERR_UNSUPPORTED;
        if ((rc = clear_chain_status(ws, s))) return rc;
        return gccnmf_klnmf_fixed_launch(V, W, H, workspace, F, N, K, batch, iterations, alpha, eps, m.h_ones, s);
    }
    if ((rc = klnmf_stage(0, V, W, H, ws, g, batch, alpha, eps, m, p, s))) return rc;
    const int chained = p.chain, short_group = p.short_group;      // (at most one of the two)
    const bool chains = (chained || short_group) && iterations > 0;
    if (!chained && !short_group && (rc = clear_chain_status(ws, s))) return rc;
    if (chains && (rc = zero_chain_counters(ws, s))) return rc;
    if (short_group) {                                      // the short chain: every iteration of the call
        for (int it0 = 0; it0 < iterations; it0 += GCCNMF_CHAIN_MAX_ITERATIONS)
            if ((rc = launch_short_chain(g, V, W, H, ws, alpha, eps, batch, short_group, it0, std::min(GCCNMF_CHAIN_MAX_ITERATIONS, iterations - it0), s))) return rc;
    } else if (chained == 8) {                              // chained, the whole call
        for (int it0 = 0; it0 < iterations; it0 += GCCNMF_CHAIN_MAX_ITERATIONS)      // (one launch; a call of thousands of iterations: a few, the grid stays below 2^30 workgroups)
            if ((rc = launch_klnmf_chain(4, g, V, W, H, ws, alpha, eps, batch, m, it0, std::min(GCCNMF_CHAIN_MAX_ITERATIONS, iterations - it0), s, nullptr))) return rc;
    } else {                                                // chained per iteration (the first 2 or 4 stages), or plain
        for (int it = 0; it < iterations; ++it) {
            if (chained && (rc = launch_klnmf_chain(chained, g, V, W, H, ws, alpha, eps, batch, m, it, 1, s, nullptr))) return rc;
            for (int stage = chained + 1; stage <= 5; ++stage)
                if ((rc = klnmf_stage(stage, V, W, H, ws, g, batch, alpha, eps, m, p, s))) return rc;
        }
    }
    return finish_call(chains, V, W, H, ws, g, batch, alpha, eps, m, p, s);
}

// Did the chained launches of the LAST gccnmf_klnmf / gccnmf_klnmf_ragged call on this workspace hand over cleanly?  (The call itself is
// asynchronous and poisons W, H with NaN if they did not; this is the explicit check: a blocking read of the status words.)  status: 0 = clean (or
// the call did not chain), bit 0 = a consumer gave up waiting for its producer (GEMM_SYNC_TIMEOUT), bit 1 = the workgroups of some list ran on more
// than one XCC (the hand-over through one XCD's L2 is then not guaranteed).  N: the column count the workspace was sized with (Nmax for a ragged batch).
int gccnmf_klnmf_chain_status(const float* workspace, int F, int N, int K, int batch, int* status) {
    GCCNMF_ENTER();
    if (!workspace || !status || F < 2 || N < 1 || K < 1 || batch < 1) return GCCNMF_ERR_ARG;
    const KlnmfWorkspace ws = carve(const_cast<float*>(workspace), make_geom(F, N, K), batch, false);
    unsigned host[GCCNMF_STATUS_WORDS];
    if (hipMemcpy(host, ws.status, sizeof(host), hipMemcpyDeviceToHost) != hipSuccess) return GCCNMF_ERR_LAUNCH;
    int st = host[0] ? 1 : 0;
    for (int l = 0; l < 8; ++l)
        if (__builtin_popcount(host[GCCNMF_STATUS_XCC_SEEN + l]) > 1) st |= 2;
    *status = st;
    return GCCNMF_OK;
}

// ---- ragged batches: mixtures of different lengths in one call (gccNMF/runGCCNMF.py:30-36 separates a file of ANY length) -------------
struct RaggedTables {
    int v[GCCNMF_RAGGED_MAX_BATCH + 8 * (GEMM_RAGGED_LMAX + 1)];
};
__global__ void nmf_store_ragged_tables_kernel(RaggedTables t, int* dst, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = t.v[i];
}

long gccnmf_klnmf_ragged_workspace_floats(int F, int Nmax, int K, int batch) {
    GCCNMF_ENTER();
    if (F < 2 || Nmax < 1 || K < 1 || batch < 1 || batch > GCCNMF_RAGGED_MAX_BATCH) return -1;
    return carve(nullptr, make_geom(F, Nmax, K), batch, true).floats;
}

int gccnmf_klnmf_ragged(const float* V, float* W, float* H, float* workspace, int F, const int* N, int Nmax, int K, int batch, int iterations,
                        float sparsity_alpha, float epsilon, int flags, void* stream) {
    GCCNMF_ENTER();
    if (!V || !W || !H || !workspace || !N || F < 2 || Nmax < 1 || K < 1 || batch < 1 || iterations < 0) return GCCNMF_ERR_ARG;
    if (flags & (GCCNMF_FLAG_CONTINUITY | GCCNMF_FLAG_CONTINUITY_STEREO)) return GCCNMF_ERR_ARG;      // (a ragged batch has no temporal-continuity form)
    KlnmfMode m;
    m.segments = 0;
    if (decode_mode(flags, F, K, m) || m.fixed_w || m.free_atoms || m.divergence) return GCCNMF_ERR_ARG;
    m.groups = 1;      // (intended today: the concurrent-groups bit is masked off -- a ragged batch exists in ONE form, whatever runs beside it)
    if (!workspace_aligned(workspace)) return GCCNMF_ERR_ARG;
    if (batch > GCCNMF_RAGGED_MAX_BATCH) return GCCNMF_ERR_UNSUPPORTED;
    long tiles = 0;
    for (int f = 0; f < batch; ++f) {
        if (N[f] < 1 || N[f] > Nmax) return GCCNMF_ERR_ARG;
        tiles += gccnmf_ceil_div(N[f], 64);
    }
    hipStream_t s = (hipStream_t)stream;
    const NmfGeom g = make_geom(F, Nmax, K);
    // a ragged batch exists only as a chained launch (the plain launches take one N for the whole batch): where that form is not available
    // -- short dictionaries, a handful of files -- the caller runs the files of each length as a batch of their own
    const KlnmfPlan p = plan_klnmf(g, batch, m);      // (of a uniform batch of the longest file: stages 0 and 6 are all that is run by it)
    if (!chain_capable(g, batch, m, p.direct, tiles)) return GCCNMF_ERR_UNSUPPORTED;
    // deal the files out to the eight lists: longest first, each to the list with the fewest column tiles so far (ties: the lower list)
    RaggedPlan rg = {};
    rg.n = N;
    std::vector<int> order(batch);
    for (int f = 0; f < batch; ++f) order[f] = f;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return N[x] > N[y]; });
    long load[8] = {};
    for (int f : order) {
        int best = 0;
        for (int l = 1; l < 8; ++l)
            if (load[l] < load[best]) best = l;
        int& cnt = rg.lists[best][0];
        if (cnt >= GEMM_RAGGED_LMAX) return GCCNMF_ERR_UNSUPPORTED;
        rg.lists[best][1 + cnt++] = f;
        load[best] += gccnmf_ceil_div(N[f], 64);
    }
    for (int l = 0; l < 8; ++l) std::sort(rg.lists[l] + 1, rg.lists[l] + 1 + rg.lists[l][0]);      // a list serves its files in ascending order
    const KlnmfWorkspace ws = carve(workspace, g, batch, true);
    RaggedTables t = {};
    for (int f = 0; f < batch; ++f) t.v[f] = N[f];
    for (int l = 0; l < 8; ++l)
        for (int k = 0; k <= GEMM_RAGGED_LMAX; ++k) t.v[batch + l * (GEMM_RAGGED_LMAX + 1) + k] = rg.lists[l][k];
    hipLaunchKernelGGL(nmf_store_ragged_tables_kernel, dim3(1), dim3(256), 0, s, t, ws.ragged_tables, batch + 8 * (GEMM_RAGGED_LMAX + 1));
    GCCNMF_CHECK_LAUNCH();
    rg.d_n = ws.ragged_tables;
    rg.d_lists = ws.ragged_tables + batch;
    int rc;
    if ((rc = klnmf_stage(0, V, W, H, ws, g, batch, sparsity_alpha, epsilon, m, p, s))) return rc;
    if (iterations > 0) {
        if ((rc = zero_chain_counters(ws, s))) return rc;
        for (int it0 = 0; it0 < iterations; it0 += GCCNMF_CHAIN_MAX_ITERATIONS)
            if ((rc = launch_klnmf_chain(4, g, V, W, H, ws, sparsity_alpha, epsilon, batch, m, it0, std::min(GCCNMF_CHAIN_MAX_ITERATIONS, iterations - it0), s, &rg)))
                return rc;
    }
    return finish_call(iterations > 0, V, W, H, ws, g, batch, sparsity_alpha, epsilon, m, p, s);
}

// ---- shared dictionary (one W for every file / rank) ------------------------------------------
// A rank's columns come as SHARDS: `batch` files of N columns each, either whole padded matrices back to back
// ([batch][Fp][Np] / [batch][Kp][Np], ld = 0) or -- ld > 0 -- column blocks of ONE matrix with row pitch ld (file b = columns
// [b*N, b*N+N) of V [Fp][ld], H [Kp][ld]; N a multiple of 64 unless batch == 1): the frame windows of one long mixture need no
// gather / scatter that way.  Per shard scratch: R (same layout as V) | Upart [batch][Fp][Kp] | rowsum_part [batch][Kp] | (one file in the
// plain layout) a reserved block, unused: GCCNMF_SPLITS x (max(Fp*Np, Fp*Kp) + Kp) floats | the direct path's Wt, Ht, Rt.
// Shared by all shards of a rank: W, vec = colsumW [Kp] | hscale [Kp], partial = num [Fp][Kp] | den [Kp].
struct SharedShard {
    const float* V;
    float *H, *R, *Upart, *rowsum_part;
    bool single_file;                 // one file in the plain layout: its scratch carries the direct path's buffers
    bool direct;                      // ... and the current tuning sends it down that path: the direct-to-register kernels (direct.hip)
    DirectBufs d;                     // transposed copies (Wt, Ht, Rt) of such a shard, behind the reserved block
    NmfGeom g;
    int batch;
    long r_floats;
};

static long shared_r_floats(const NmfGeom& g, int batch, int ld) { return ld > 0 ? (long)g.Fp * ld : (long)batch * g.sV; }

static bool shared_shard_ok(int F, int N, int K, int batch, int ld) {
    if (F < 2 || N < 1 || K < 1 || batch < 1 || ld < 0) return false;
    if (ld > 0 && ((ld & 3) || (long)batch * N > ld || (batch > 1 && (N & 63)))) return false;
    return true;
}

// A shard that is ONE file in the plain layout (a rank's whole, short column range: at eight ranks a 160 s mixture leaves 20 s each)
// is latency-bound exactly like one mixture alone: it takes that path's direct kernels instead of 64-80 workgroup launches with 64-78-step chains.
static bool shared_single_file_layout(const NmfGeom& g, int batch, int ld) { return batch == 1 && (ld == 0 || ld == g.Np); }   // sizes the scratch
static long shared_reserved_floats(const NmfGeom& g) { return GCCNMF_SPLITS * ((g.sV > g.sU ? g.sV : g.sU) + (long)g.Kp); }
static long shared_single_file_floats(const NmfGeom& g) { return shared_reserved_floats(g) + direct_floats(g, 1); }

static SharedShard make_shard(const float* V, float* H, float* ws, int F, int N, int K, int batch, int ld) {
    SharedShard sh;
    sh.g = make_geom(F, N, K);
    sh.single_file = shared_single_file_layout(sh.g, batch, ld);
    sh.direct = sh.single_file && direct_path(sh.g, 1, 1);
    if (ld > 0) {
        sh.g.ld = ld;
        sh.g.sV = sh.g.sH = N;              // the next file is the next column block
    }
    sh.V = V; sh.H = H; sh.batch = batch;
    sh.r_floats = shared_r_floats(sh.g, batch, ld);
    sh.R = ws;
    sh.Upart = sh.R + sh.r_floats;
    sh.rowsum_part = sh.Upart + (long)batch * sh.g.sU;
    if (sh.single_file) {
        sh.g = make_geom(F, N, K);              // (ld == Np: the plain single-file geometry; strides are irrelevant for one file)
        sh.d = direct_bufs(sh.g, sh.rowsum_part + (long)batch * sh.g.Kp + shared_reserved_floats(sh.g), 1);
    }
    return sh;
}

static int shared_begin(const SharedShard* sh, int n, const float* W, float* colsumW, float* hscale, int F, int K, hipStream_t s) {
    NmfGeom g = make_geom(F, 1, K);
    for (int i = 0; i < n; ++i) {    // R's padding (rows >= F, columns >= N) is a reduction operand of K2 and K4a: zero
        if (hipMemsetAsync(sh[i].R, 0, sizeof(float) * sh[i].r_floats, s) != hipSuccess) return GCCNMF_ERR_LAUNCH;
        // ... and so are the rows n >= N of Ht / Rt and the columns f >= F of Wt on the direct path
        if (sh[i].single_file && hipMemsetAsync(sh[i].d.Wt, 0, sizeof(float) * direct_floats(sh[i].g, 1), s) != hipSuccess) return GCCNMF_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(nmf_prepare_kernel, dim3(g.Kp / 16), dim3(256), 0, s, W, colsumW, hscale, g.F, g.Fp, g.Kp);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

// Side streams of the shared-dictionary iteration.  K1 .. K4a of different files (column blocks) are independent until the W update,
// so a rank's files run as up to GCCNMF_SHARED_STREAMS groups on separate streams (tuning key 8, default 3): the tail of one group's
// launch -- when its last workgroups no longer fill both slots of every CU -- overlaps the head of another group's, exactly as the
// per-file-dictionary engine does with its file groups.  Same kernels on the same data: bitwise the one-stream result.
struct SidePool {
    hipStream_t side[GCCNMF_SHARED_STREAMS - 1];
    hipEvent_t fork, join[GCCNMF_SHARED_STREAMS - 1];
    bool ok = false;
};
static SidePool* side_pool() {
    static SidePool pools[GCCNMF_MAX_DEVICES];
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= GCCNMF_MAX_DEVICES) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    SidePool& p = pools[dev];
    if (!p.ok) {
        if (hipEventCreateWithFlags(&p.fork, hipEventDisableTiming) != hipSuccess) return nullptr;
        for (int i = 0; i < GCCNMF_SHARED_STREAMS - 1; ++i) {
            if (hipStreamCreateWithFlags(&p.side[i], hipStreamNonBlocking) != hipSuccess) return nullptr;
            if (hipEventCreateWithFlags(&p.join[i], hipEventDisableTiming) != hipSuccess) return nullptr;
        }
        p.ok = true;
    }
    return &p;
}

// files [b0, b1) of a shard as a shard of their own (same matrices, offset bases)
static SharedShard sub_shard(const SharedShard& sh, int b0, int b1) {
    SharedShard u = sh;
    u.V = sh.V + b0 * sh.g.sV;
    u.H = sh.H + b0 * sh.g.sH;
    u.R = sh.R + b0 * sh.g.sV;
    u.Upart = sh.Upart + b0 * sh.g.sU;
    u.rowsum_part = sh.rowsum_part + (long)b0 * sh.g.Kp;
    u.batch = b1 - b0;
    return u;
}

// H update with the current W, then the per-file (V/WH).H^T and row sums of H (K1, K2, K3, K4a on stream s)
static int shared_gemms(const SharedShard& sh, const float* W, const float* colsumW, const float* hscale, float alpha, float eps,
                        bool beside_others, hipStream_t s) {
    const NmfGeom& g = sh.g;
    int rc;
    // another unit's launches run beside these on a side stream: the tile-layout cost model of gemm_dma.h prices a launch that has the chip
    // to itself, so such units keep full tiles (their partial rounds overlap the neighbours' kernels)
    const int xa = 1, conc = beside_others ? 1 : 0;      // (intended today: 1, not the number of units)
    if (sh.direct) {                            // one file alone: the direct-to-register kernels (csrc/direct.hip), W transposed per iteration
        if ((rc = gccnmf_transpose_launch(W, 0, g.Kp, sh.d.Wt, sh.d.sWt, sh.d.ldwt, g.F, g.Kp, 1, s))) return rc;
        if ((rc = direct_wh_div(g, sh.d, sh.V, W, sh.H, hscale, sh.R, false, 1, s))) return rc;
        if ((rc = direct_update_h(g, sh.d, W, sh.R, sh.H, hscale, colsumW, alpha, eps, 1, s))) return rc;
        if ((rc = direct_wh_div(g, sh.d, sh.V, W, sh.H, nullptr, sh.R, true, 1, s))) return rc;
        return direct_rht(g, sh.d, sh.R, sh.Upart, sh.rowsum_part, 1, s);
    }
    // files are independent inside K1-K3 and per file inside K4a: keep every tile of a file on one XCD (its H / R panels are shared
    // through that XCD's L2), exactly as the per-file-dictionary path does
    if ((rc = launch_wh_div(g, wh_div_args(g, sh.V, W, 0, sh.H, hscale, 0, sh.R, sh.batch, xa, conc), s))) return rc;
    if ((rc = launch_update_h(update_h_args(g, W, 0, sh.R, sh.H, hscale, 0, colsumW, 0, alpha, eps, sh.batch, xa, conc), s))) return rc;
    // (H now carries the previous normalisation; K3 below takes no scale, and step B rewrites hscale before anyone reads it again)
    if ((rc = launch_wh_div(g, wh_div_args(g, sh.V, W, 0, sh.H, nullptr, 0, sh.R, sh.batch, xa, conc), s))) return rc;
    return launch_rht(g, rht_args(g, sh.R, sh.H, sh.Upart, sh.rowsum_part, sh.batch, xa, conc), s);
}

// partial (+)= [sum_files Upart || sum_files rowsum_part], files in ascending order (deterministic)
static int shared_reduce(const SharedShard& sh, float* partial, int accumulate, hipStream_t s) {
    const NmfGeom& g = sh.g;
    hipLaunchKernelGGL(nmf_reduce_files_kernel, dim3((unsigned)((g.sU + 255) / 256)), dim3(256), 0, s, sh.Upart, g.sU, sh.batch, g.sU, partial, accumulate);
    GCCNMF_CHECK_LAUNCH();
    hipLaunchKernelGGL(nmf_reduce_files_kernel, dim3(gccnmf_ceil_div(g.Kp, 256)), dim3(256), 0, s, sh.rowsum_part, (long)g.Kp, sh.batch, (long)g.Kp,
                       partial + g.sU, accumulate);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

// Step A of every shard of a rank: the GEMMs of the shards' file groups dealt out over the main stream and the side streams, joined,
// then the file-order reductions on the main stream.
static int shared_step_a_all(const SharedShard* sh, int n, const float* W, const float* colsumW, const float* hscale, float* partial,
                             float alpha, float eps, hipStream_t s) {
    int rc;
    SharedShard units[GCCNMF_MAX_SHARDS * GCCNMF_SHARED_STREAMS];
    int nu = 0;
    const int want = gccnmf_tune_shared_groups;
    for (int i = 0; i < n; ++i) {
        // Groups pay only when ONE launch over the whole shard cannot fill the chip (fewer than 512 throughput tiles = two per CU:
        // a 160 s mixture has 313): then the groups' launches, each a fraction of a round, run side by side and the short kernels of
        // different stages overlap.  A shard that fills the chip by itself loses with groups in lock-step (64 files: 151 k frames/s
        // as one group, 144 k as two, 130 k as three -- profiles/r03b): one group.
        const long tiles = (long)sh[i].batch * gccnmf_ceil_div(sh[i].g.N, 64);
        int groups = tiles >= 512 ? 1 : (int)(tiles / 64);
        if (groups > sh[i].batch) groups = sh[i].batch;
        groups = groups < 1 ? 1 : (groups > want ? want : groups);
        for (int q = 0; q < groups; ++q) units[nu++] = sub_shard(sh[i], (int)((long)sh[i].batch * q / groups), (int)((long)sh[i].batch * (q + 1) / groups));
    }
    SidePool* pool = (nu > 1 && want > 1) ? side_pool() : nullptr;
    const int lanes = pool ? (want < nu ? want : nu) : 1;
    if (lanes > 1) {
        if (hipEventRecord(pool->fork, s) != hipSuccess) return GCCNMF_ERR_LAUNCH;
        for (int l = 1; l < lanes; ++l)
            if (hipStreamWaitEvent(pool->side[l - 1], pool->fork, 0) != hipSuccess) return GCCNMF_ERR_LAUNCH;
    }
    for (int u = 0; u < nu; ++u) {
        const int l = u % lanes;
        if ((rc = shared_gemms(units[u], W, colsumW, hscale, alpha, eps, lanes > 1, l ? pool->side[l - 1] : s))) return rc;
    }
    for (int l = 1; l < lanes; ++l) {
        if (hipEventRecord(pool->join[l - 1], pool->side[l - 1]) != hipSuccess) return GCCNMF_ERR_LAUNCH;
        if (hipStreamWaitEvent(s, pool->join[l - 1], 0) != hipSuccess) return GCCNMF_ERR_LAUNCH;
    }
    for (int i = 0; i < n; ++i)
        if ((rc = shared_reduce(sh[i], partial, i > 0, s))) return rc;
    return GCCNMF_OK;
}

static int shared_step_b(float* W, const float* partial, float* colsumW, float* hscale, int F, int K, hipStream_t s) {
    NmfGeom g = make_geom(F, 1, K);
    return launch_update_w(update_w_args(g, W, 0, partial, 0, partial + g.sU, colsumW, hscale, 0), 1, 1, s, nullptr, 0, 0);
}

static int shared_finish(const SharedShard* sh, int n, float* hscale, int K, hipStream_t s) {
    for (int i = 0; i < n; ++i) {
        const NmfGeom& g = sh[i].g;
        hipLaunchKernelGGL(nmf_scale_h_kernel, dim3(sh[i].batch * g.K), dim3(256), 0, s, sh[i].H, hscale, 0L, g.K, g.sH, g.ld, g.Np);
        GCCNMF_CHECK_LAUNCH();
    }
    const int Kp = gccnmf_round_up(K, 64);
    hipLaunchKernelGGL(nmf_fill_kernel, dim3(gccnmf_ceil_div(Kp, 256)), dim3(256), 0, s, hscale, 1.f, (long)Kp);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

// the four-call protocol's workspace: one default-layout shard's scratch | colsumW [Kp] | hscale [Kp]
static float* legacy_vec(const SharedShard& sh) {
    return sh.single_file ? sh.d.Wt + direct_floats(sh.g, 1) : sh.rowsum_part + (long)sh.batch * sh.g.Kp;
}

long gccnmf_klnmf_shared_workspace_floats(int F, int N, int K, int batch) {
    GCCNMF_ENTER();
    if (!shared_shard_ok(F, N, K, batch, 0)) return -1;
    NmfGeom g = make_geom(F, N, K);
    return (long)batch * (g.sV + g.sU + g.Kp) + (shared_single_file_layout(g, batch, 0) ? shared_single_file_floats(g) : 0) + 2L * g.Kp;
}

long gccnmf_klnmf_shared_shard_workspace_floats(int F, int N, int K, int batch, int ld) {
    GCCNMF_ENTER();
    if (!shared_shard_ok(F, N, K, batch, ld)) return -1;
    NmfGeom g = make_geom(F, N, K);
    return shared_r_floats(g, batch, ld) + (long)batch * (g.sU + g.Kp) + (shared_single_file_layout(g, batch, ld) ? shared_single_file_floats(g) : 0);
}

long gccnmf_klnmf_shared_partial_floats(int F, int K) {
    GCCNMF_ENTER();
    if (F < 2 || K < 1) return -1;
    NmfGeom g = make_geom(F, 1, K);
    return g.sU + g.Kp;
}

int gccnmf_klnmf_shared_begin(const float* W, float* workspace, int F, int N, int K, int batch, void* stream) {
    GCCNMF_ENTER();
    if (!W || !workspace || !shared_shard_ok(F, N, K, batch, 0)) return GCCNMF_ERR_ARG;
    SharedShard sh = make_shard(nullptr, nullptr, workspace, F, N, K, batch, 0);
    float* vec = legacy_vec(sh);
    return shared_begin(&sh, 1, W, vec, vec + sh.g.Kp, F, K, (hipStream_t)stream);
}

int gccnmf_klnmf_shared_step_a(const float* V, const float* W, float* H, float* workspace, float* partial, int F, int N,
                               int K, int batch, float sparsity_alpha, float epsilon, void* stream) {
    GCCNMF_ENTER();
    if (!V || !W || !H || !workspace || !partial || !shared_shard_ok(F, N, K, batch, 0)) return GCCNMF_ERR_ARG;
    SharedShard sh = make_shard(V, H, workspace, F, N, K, batch, 0);
    float* vec = legacy_vec(sh);
    return shared_step_a_all(&sh, 1, W, vec, vec + sh.g.Kp, partial, sparsity_alpha, epsilon, (hipStream_t)stream);
}

int gccnmf_klnmf_shared_step_b(float* W, float* workspace, const float* partial, int F, int N, int K, int batch, void* stream) {
    GCCNMF_ENTER();
    if (!W || !workspace || !partial || !shared_shard_ok(F, N, K, batch, 0)) return GCCNMF_ERR_ARG;
    SharedShard sh = make_shard(nullptr, nullptr, workspace, F, N, K, batch, 0);
    float* vec = legacy_vec(sh);
    return shared_step_b(W, partial, vec, vec + sh.g.Kp, F, K, (hipStream_t)stream);
}

int gccnmf_klnmf_shared_finish(float* H, float* workspace, int F, int N, int K, int batch, void* stream) {
    GCCNMF_ENTER();
    if (!H || !workspace || !shared_shard_ok(F, N, K, batch, 0)) return GCCNMF_ERR_ARG;
    SharedShard sh = make_shard(nullptr, H, workspace, F, N, K, batch, 0);
    float* vec = legacy_vec(sh);
    return shared_finish(&sh, 1, vec + sh.g.Kp, K, (hipStream_t)stream);
}

// The whole shared-dictionary training of one rank in ONE call: begin, `iterations` x (step A of every shard -> all-reduce of
// `partial` -> step B), finish -- every launch and the collective enqueued on `stream` from C, no host round trip per iteration.
// One training at a time per device: the side streams and events of shared_step_a_all are per-device library state.  A second call that
// arrives while one is still enqueueing is REJECTED (GCCNMF_ERR_UNSUPPORTED) instead of racing on them.
namespace {
std::atomic<int> shared_run_busy[GCCNMF_MAX_DEVICES];
struct SharedRunGuard {
    int dev = -1;
    bool held = false;
    SharedRunGuard() {
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= GCCNMF_MAX_DEVICES) { dev = -1; held = true; return; }
        int expected = 0;
        held = shared_run_busy[dev].compare_exchange_strong(expected, 1);
    }
    ~SharedRunGuard() {
        if (held && dev >= 0) shared_run_busy[dev].store(0);
    }
};
}  // namespace

int gccnmf_klnmf_shared_run(const gccnmf_shared_shard* shards, int nshards, float* W, float* partial, float* vec, int F, int K,
                            int iterations, float sparsity_alpha, float epsilon, gccnmf_allreduce_fn allreduce, void* allreduce_ctx,
                            void* stream) {
    GCCNMF_ENTER();
    if (nshards < 0 || nshards > GCCNMF_MAX_SHARDS || (nshards && !shards) || !W || !partial || !vec || F < 2 || K < 1 || iterations < 0)
        return GCCNMF_ERR_ARG;
    SharedRunGuard guard;
    if (!guard.held) return GCCNMF_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    SharedShard sh[GCCNMF_MAX_SHARDS];
    for (int i = 0; i < nshards; ++i) {
        const gccnmf_shared_shard& d = shards[i];
        if (!d.V || !d.H || !d.workspace || !shared_shard_ok(F, d.N, K, d.batch, d.ld)) return GCCNMF_ERR_ARG;
        sh[i] = make_shard(d.V, d.H, d.workspace, F, d.N, K, d.batch, d.ld);
    }
    const NmfGeom g = make_geom(F, 1, K);
    float *colsumW = vec, *hscale = vec + g.Kp;
    const long np = g.sU + g.Kp;
    int rc;
    if ((rc = shared_begin(sh, nshards, W, colsumW, hscale, F, K, s))) return rc;
    for (int it = 0; it < iterations; ++it) {
        // a rank without columns (fewer files than ranks) contributes a zero partial and still follows every W update
        if (nshards == 0 && hipMemsetAsync(partial, 0, sizeof(float) * np, s) != hipSuccess) return GCCNMF_ERR_LAUNCH;
        if (nshards && (rc = shared_step_a_all(sh, nshards, W, colsumW, hscale, partial, sparsity_alpha, epsilon, s))) return rc;
        if (allreduce && allreduce(allreduce_ctx, partial, np, stream) != 0) return GCCNMF_ERR_COLLECTIVE;
        if ((rc = shared_step_b(W, partial, colsumW, hscale, F, K, s))) return rc;
    }
    return shared_finish(sh, nshards, hscale, K, s);
}

#ifdef GCCNMF_EXPERIMENTS
int gccnmf_debug_mfma_peak(float* scratch, int blocks, int iters, void* stream) {
    GCCNMF_ENTER();
    if (!scratch || blocks < 1 || iters < 1) return GCCNMF_ERR_ARG;
    hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, scratch, iters);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}
#endif

int gccnmf_debug_gemm_plan(int M, int N, int batch, int xcd_affine, int concurrent, int narrow_capable, int* plan, int* items, int max_items) {
    GCCNMF_ENTER();
    if (M < 1 || N < 1 || batch < 1 || !plan || (max_items > 0 && !items)) return -1;
    GemmArgs a = {};
    a.M = M; a.N = N; a.batch = batch; a.xcd_affine = xcd_affine; a.concurrent = concurrent;
    const int grid = gemm_dma_plan(a, (narrow_capable & 1) != 0, 4, (narrow_capable & 2) != 0);      // bit 1: the whole-file lists of chained launches
    if (grid < 1) return -1;
    const int fields[8] = {a.lists, a.cw, a.cr, a.split, a.rag, a.tiles_m, a.tiles_n, grid};
    for (int i = 0; i < 8; ++i) plan[i] = fields[i];
    int n = 0;
    for (int list = 0; list < a.lists; ++list)
        for (int t = 0;; ++t) {
            int file, tm, col0, nw;
            if (!gemm_dma_item(a, list, t, file, tm, col0, nw)) break;      // the same decode the kernel runs
            if (n < max_items) {
                int* it = items + 6 * n;
                it[0] = list; it[1] = t; it[2] = file; it[3] = tm; it[4] = col0; it[5] = nw;
            }
            ++n;
        }
    return n;
}

int gccnmf_debug_gemm(const float* A, const float* B, float* C, int M, int N, int Kd, int lda, int ldb, int ldc,
                      int a_clamp, int b_clamp, int layout, int batch, long sA, long sB, long sC, const float* bscale,
                      float* rowsumB, void* stream) {
    GCCNMF_ENTER();
    GemmArgs a = {};
    a.A = A; a.sA = sA; a.lda = lda; a.a_clamp = a_clamp;
    a.B = B; a.sB = sB; a.ldb = ldb; a.b_clamp = b_clamp;
    const bool tail = layout & 4;
    a.M = tail ? M - 1 : M; a.N = N; a.Kd = Kd;
    if (layout & 16) {   // rank-1 reduction tail (non-KC operands only)
        if (layout & 3) return GCCNMF_ERR_ARG;
        a.Kd = Kd - 1;
        a.ktailA = A + (long)(Kd - 1) * lda; a.s_ktailA = sA;
        a.ktailB = B + (long)(Kd - 1) * ldb; a.s_ktailB = sB;
    }
    a.tail_row = M - 1;
    a.batch = batch; a.xcd_affine = 1;
    a.bscale = bscale; a.s_bscale = 0;
    a.rowsumB = rowsumB; a.s_rowsumB = N;
    a.C = C; a.sC = sC; a.ldc = ldc;
    hipStream_t s = (hipStream_t)stream;
    if (layout & 32) return GCCNMF_ERR_UNSUPPORTED;      // (once a kernel that is gone)
    const bool wide = layout & 8;
    if (!wide && gccnmf_tune_dma) {       // the throughput tile's default staging path (tuning key 3)
        switch (layout & 3) {
            case 0: return tail ? GCCNMF_ERR_ARG : gccnmf_launch_gemm_dma<false, false, EPI_STORE, false>(a, s);
            case 1: return tail ? gccnmf_launch_gemm_dma<true, false, EPI_STORE, true>(a, s) : gccnmf_launch_gemm_dma<true, false, EPI_STORE, false>(a, s);
            case 3: return tail ? gccnmf_launch_gemm_dma<true, true, EPI_STORE, true>(a, s) : gccnmf_launch_gemm_dma<true, true, EPI_STORE, false>(a, s);
            default: return GCCNMF_ERR_UNSUPPORTED;
        }
    }
    switch (layout & 3) {
        case 0:
            if (tail) return GCCNMF_ERR_ARG;
            return wide ? gccnmf_launch_gemm<1, 4, false, false, EPI_STORE, false>(a, s)
                        : gccnmf_launch_gemm<4, 1, false, false, EPI_STORE, false>(a, s);
        case 1:
            if (wide) return tail ? gccnmf_launch_gemm<1, 4, true, false, EPI_STORE, true>(a, s)
                                  : gccnmf_launch_gemm<1, 4, true, false, EPI_STORE, false>(a, s);
            return tail ? gccnmf_launch_gemm<4, 1, true, false, EPI_STORE, true>(a, s)
                        : gccnmf_launch_gemm<4, 1, true, false, EPI_STORE, false>(a, s);
        case 3:
            if (wide) return tail ? gccnmf_launch_gemm<1, 4, true, true, EPI_STORE, true>(a, s)
                                  : gccnmf_launch_gemm<1, 4, true, true, EPI_STORE, false>(a, s);
            return tail ? gccnmf_launch_gemm<4, 1, true, true, EPI_STORE, true>(a, s)
                        : gccnmf_launch_gemm<4, 1, true, true, EPI_STORE, false>(a, s);
        default:
            return GCCNMF_ERR_UNSUPPORTED;   // (A non-KC, B KC) is not used by the path
    }
}

}  // extern "C"
