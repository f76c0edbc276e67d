// GCC-PHAT localisation, GCC-NMF target scores / coefficient masks and masked reconstruction.
// Reference: gccNMF/gccNMFFunctions.py:85-151 and gccNMF/runGCCNMF.py:46.
//
// Every contraction here is a real GEMM on the f32 matrix cores (gemm_mfma.h):
//   angular spectrogram   A[tau,t]  = [cos;sin]^T (D x 2Fp) . [Re C; Im C] (2Fp x T)        (:88-92)
//   GCC-NMF scores        G_i[k,t]  = W^T (K x F) . P_i (F x T),  P_i = Re(C * exp(-j w tau_i))  (:127-133)
//   reconstruction        S[i,c]    = W (F x K) . (H_c * M_i) (K x T)  * X_c/|X_c|           (:147-151)
// The three targets / six (target, channel) pairs are concatenated along the GEMM's column axis,
// so each stage is ONE launch for the whole batch.
#include "gemm_ring.h"
#include "ratio.h"
#include "phat.h"
#include "spatial.h"
#include "angular_nl.h"
#include "atom_tdoa.h"
#include "source_count.h"
#include "../../include/gccnmf_hip.h"


// One-shot GEMMs of a launch that cannot fill the chip with 512 x 64 tiles (one mixture alone: 60 of them) take the small-tile ring
// kernel (128 x 64, gemm_ring.h): 240 workgroups instead of 60 -- reconstruction 191 -> ~40 us, scores 83 -> ~25 us, angular
// spectrogram (three 128 x 256 workgroups before) 148 -> ~40 us for one file.
static bool gcc_small_launch(int batch, int M, int N, int Kd) {
    if (!gccnmf_ring_supports(Kd) || gccnmf_tune_tile_policy == 1) return false;
    if (gccnmf_tune_tile_policy == 2) return true;
    return (long)batch * gccnmf_ceil_div(M, 512) * gccnmf_ceil_div(N, 64) < 256;
}

// mean over time of the angular spectrogram, accumulated in double (runGCCNMF.py:46 works on float64).
// grid = batch * D, 256 threads.
__global__ __launch_bounds__(256) void ang_mean_kernel(const float* __restrict__ ang, int T, int D, int Dp, int Tp,
                                                       double* __restrict__ mean_ang) {
    __shared__ double red[256];
    const int b = blockIdx.x / D, d = blockIdx.x - b * D;
    const float* row = ang + ((long)b * Dp + d) * Tp;
    double s = 0.0;
    for (int t = threadIdx.x; t < T; t += 256) s += (double)row[t];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) mean_ang[(long)b * Dp + d] = red[0] / (double)T;
}

// Strict local maxima (scipy.signal.argrelmax, order 1: edges never qualify, NaN never compares greater),
// keep the S largest, ascending index order.  Among peaks of equal height the LARGER index is kept: the reference keeps
// peakIndexes[argsort(values)[-S:]], and a stable ascending sort puts the larger of two equal values last.
// THE peak rule, on one row v[0..D) that the calling 64-thread block has put into LDS (D <= 4096): the whole-file estimate runs it on
// the time mean, the time-varying tracks on every frame's windowed mean.  out[n * out_stride], n < S, receives the chosen indexes
// (-1 beyond the peaks found); returns whether S peaks were found (valid in thread 0).
__device__ __forceinline__ bool pick_peaks_row(const double* v, unsigned char* is_peak, int* s_found, int D, int S, int* out,
                                               long out_stride) {
    __syncthreads();
    for (int i = threadIdx.x; i < D; i += 64) is_peak[i] = (i > 0 && i < D - 1 && v[i] > v[i - 1] && v[i] > v[i + 1]) ? 1 : 0;
    __syncthreads();
    // top-S peaks: S rounds of a 64-lane arg-max over the peaks still standing (largest value, largest index on ties; a serial scan
    // cost 33 us of a single-mixture run)
    if (threadIdx.x == 0) *s_found = 0;
    __syncthreads();
    for (int s = 0; s < S; ++s) {
        double bv = 0.0;
        int bi = -1;
        for (int i = 1 + threadIdx.x; i < D - 1; i += 64)
            if (is_peak[i] == 1 && (bi < 0 || v[i] >= bv)) {
                bv = v[i];
                bi = i;
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi > bi))) {
                bv = ov;
                bi = oi;
            }
        }
        if (bi < 0) break;                     // wave-uniform after the butterfly
        if (threadIdx.x == 0) {
            is_peak[bi] = 2;
            ++*s_found;
        }
        __syncthreads();
    }
    __syncthreads();
    if (threadIdx.x != 0) return false;
    int n = 0;
    for (int i = 1; i < D - 1 && n < S; ++i)
        if (is_peak[i] == 2) out[(n++) * out_stride] = i;
    for (; n < S; ++n) out[n * out_stride] = -1;
    return *s_found == S;
}

// One 64-thread block per file; D <= 4096.
__global__ __launch_bounds__(64) void pick_peaks_kernel(const double* __restrict__ mean_ang, int D, int Dp, int S,
                                                        int* __restrict__ tdoa_idx, int* __restrict__ status) {
    __shared__ double v[4096];
    __shared__ unsigned char is_peak[4096];
    __shared__ int s_found;
    const int b = blockIdx.x;
    const double* m = mean_ang + (long)b * Dp;
    for (int i = threadIdx.x; i < D; i += 64) v[i] = m[i];
    const bool all = pick_peaks_row(v, is_peak, &s_found, D, S, tdoa_idx + (long)b * S, 1);
    if (threadIdx.x == 0) status[b] = all ? 0 : 1;
}

// Time-varying TDOA tracks, stage 1 of 2: for frame t of file b the mean of ang over the centred window
// [lo, hi) = [max(0, t - L/2), min(T, t - L/2 + L)) -- a float64 sum in ascending frame order over its own length, so a value depends on
// (t, L, T) and the file alone, never on the batch -- and the peak rule above on that column.  One 64-thread block per (frame, file):
// a lane owns the TDOAs d = lane, lane + 64, ... and walks its rows in aligned 16-byte groups (the groups that straddle lo or hi are
// masked: Tp is a multiple of 64, so they stay inside the row).  Dynamic LDS: 8 D + 16 + round_up(D, 16) bytes.  tracks [batch][S][Tp], status [batch][Tp]: 0 = S peaks, 1 = fewer
// (stage 2 replaces the set).  Frames t >= T are not written.  grid = (T, batch)
__global__ __launch_bounds__(64) void track_peaks_kernel(const float* __restrict__ ang, int T, int Tp, int D, int Dp, int S, int L,
                                                         int* __restrict__ tracks, int* __restrict__ status) {
    extern __shared__ double track_lds[];                        // v [D] | s_found (16 bytes) | is_peak [D]: sized by D, not by the
    double* v = track_lds;                                       // 4096-TDOA limit (36 KB a block would leave one wave per SIMD)
    int* s_found = (int*)(track_lds + D);
    unsigned char* is_peak = (unsigned char*)(track_lds + D + 2);
    const int t = blockIdx.x, b = blockIdx.y;
    const int first = t - L / 2;
    const int lo = first < 0 ? 0 : first, hi = first + L < T ? first + L : T;       // lo <= t < hi
    const double len = (double)(hi - lo);
    for (int d = threadIdx.x; d < D; d += 64) {
        const float* row = ang + ((long)b * Dp + d) * Tp;
        double s = 0.0;
        for (int g = lo & ~3; g < hi; g += 4) {
            const float4 a = *(const float4*)(row + g);
            if (g >= lo) s += (double)a.x;
            if (g + 1 >= lo && g + 1 < hi) s += (double)a.y;
            if (g + 2 >= lo && g + 2 < hi) s += (double)a.z;
            if (g + 3 >= lo && g + 3 < hi) s += (double)a.w;
        }
        v[d] = s / len;
    }
    const bool all = pick_peaks_row(v, is_peak, s_found, D, S, tracks + (long)b * S * Tp + t, Tp);
    if (threadIdx.x == 0) status[(long)b * Tp + t] = all ? 0 : 1;
}

// Stage 2: a frame with fewer than S peaks takes the set of the last complete frame before it, the frames in front of the first
// complete one take that one's; status 1 marks both, 3 (= 1 | 2) every frame of a file without any complete frame (tracks -1).
// Pass 1 leaves in status[t] the last complete frame <= t (-1: none yet) -- a running maximum, 256 frames per step -- and pass 2
// copies: a complete frame is never written, and a thread reads back only the words it wrote itself.  One 256-thread block per file.
__global__ __launch_bounds__(256) void track_carry_kernel(int T, int Tp, int S, int* __restrict__ tracks, int* __restrict__ status) {
    __shared__ int scan[256];
    __shared__ int s_carry, s_first;
    const int tid = threadIdx.x;
    int* st = status + (long)blockIdx.x * Tp;
    int* tr = tracks + (long)blockIdx.x * S * Tp;
    if (tid == 0) {
        s_carry = -1;
        s_first = T;
    }
    __syncthreads();
    for (int c = 0; c < T; c += 256) {
        const int t = c + tid;
        const bool complete = t < T && st[t] == 0;
        if (complete) atomicMin(&s_first, t);
        scan[tid] = complete ? t : -1;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int left = tid >= o ? scan[tid - o] : -1;
            __syncthreads();
            if (left > scan[tid]) scan[tid] = left;
            __syncthreads();
        }
        const int src = scan[tid] > s_carry ? scan[tid] : s_carry;
        if (t < T) st[t] = src;
        __syncthreads();
        if (tid == 255) s_carry = src;
        __syncthreads();
    }
    const int first = s_first;
    for (int t = tid; t < T; t += 256) {
        int src = st[t];
        if (src == t) {
            st[t] = 0;
            continue;
        }
        if (src < 0) src = first;
        for (int i = 0; i < S; ++i) tr[(long)i * Tp + t] = first < T ? tr[(long)i * Tp + src] : -1;
        st[t] = first < T ? 1 : 3;
    }
}

// The steering product Re(C e^{-j w tau}) = Cr cos + Ci sin of a thread's four frames, with its roundings written out and the SAME for
// every frame: fma(Cr, cos, Ci * sin), contraction off, so that neither the fixed-index nor the per-frame form depends on what a compiler
// would have paired.  A frame's product must not know where the frame sits in its buffer: the frame-sharded separation
// (distributed.py, mode 3) hands a rank the frames [t0, t1) of a mixture as its frames [0, t1 - t0), and its scores have to be the
// unsplit run's in every bit.  (Until tests/test_gpu_time_shards.py compared them, frame 1 of every four added two rounded products --
// what the compiler's packed-math pairing had once made of `cr * c + ci * sn` -- and a shard whose t0 is no multiple of 4 differed from
// the unsplit run in the last bit of a quarter of its scores.)
__device__ __forceinline__ float4 gcc_steer4(float4 cr, float4 ci, float4 c, float4 sn) {
#pragma clang fp contract(off)
    float4 out;
    out.x = fmaf(cr.x, c.x, ci.x * sn.x);
    out.y = fmaf(cr.y, c.y, ci.y * sn.y);
    out.z = fmaf(cr.z, c.z, ci.z * sn.z);
    out.w = fmaf(cr.w, c.w, ci.w * sn.w);
    return out;
}

// P[f][i*Tp + t] = Re(C[f,t] * exp(-j 2 pi f tau_i)) = Cr*cos + Ci*sin, zero in every padded position.
// One thread = four consecutive frames (16-byte loads of Cr / Ci, one 16-byte store).  grid = (ceil(S*Tp/1024), Fp, batch)
// TRACKS: tdoa_idx is [batch][S][Tp], one index per (target, frame) -- the four frames' indexes are one 16-byte load, their table
// entries four lookups in row f of the steering table (512 bytes at D = 128: they hit the vector cache); the same products in the
// same order (gcc_steer4), so constant tracks give the bits of the fixed-index form.
// COUNTED (fixed indexes only; numSources='auto'): a negative index is a target the file does not have -- its
// column is quiet NaN where a present target's holds a product, so the GEMM behind it gives NaN scores and the arg-max, which
// ignores NaN, never hands it an atom; a non-negative index takes the path it always took.
template <bool TRACKS, bool COUNTED>
__global__ __launch_bounds__(256) void gcc_steer_kernel(const float* __restrict__ CC, const float* __restrict__ trig,
                                                        const int* __restrict__ tdoa_idx, int F, int Fp, int T, int Tp, int D,
                                                        int Dp, int S, float* __restrict__ P) {
    const int col = 4 * (blockIdx.x * 256 + threadIdx.x);
    const int f = blockIdx.y, b = blockIdx.z;
    if (col >= S * Tp) return;
    const int i = col / Tp, t = col - i * Tp;                   // Tp is a multiple of 64: the four frames share the target
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f < F && t < T) {
        const long plane = (long)Fp * Tp;
        const float4 cr = *(const float4*)(CC + (long)b * 2 * plane + (long)f * Tp + t);
        const float4 ci = *(const float4*)(CC + (long)b * 2 * plane + plane + (long)f * Tp + t);
        const float* cos_row = trig + (long)f * Dp;
        const float* sin_row = trig + ((long)Fp + f) * Dp;
        int4 tau;
        if (TRACKS) tau = *(const int4*)(tdoa_idx + ((long)b * S + i) * Tp + t);
        else tau.x = tau.y = tau.z = tau.w = tdoa_idx[(long)b * S + i];
        const bool absent = COUNTED && tau.x < 0;
        tau.x = tau.x < 0 ? 0 : (tau.x >= D ? D - 1 : tau.x);
        tau.y = tau.y < 0 ? 0 : (tau.y >= D ? D - 1 : tau.y);
        tau.z = tau.z < 0 ? 0 : (tau.z >= D ? D - 1 : tau.z);
        tau.w = tau.w < 0 ? 0 : (tau.w >= D ? D - 1 : tau.w);
        out = gcc_steer4(cr, ci, make_float4(cos_row[tau.x], cos_row[tau.y], cos_row[tau.z], cos_row[tau.w]),
                         make_float4(sin_row[tau.x], sin_row[tau.y], sin_row[tau.z], sin_row[tau.w]));
        if (absent) out.x = out.y = out.z = out.w = __builtin_nanf("");
        if (t + 1 >= T) out.y = 0.f;
        if (t + 2 >= T) out.z = 0.f;
        if (t + 3 >= T) out.w = 0.f;
    }
    *(float4*)(P + ((long)b * Fp + f) * ((long)S * Tp) + col) = out;
}

// argmax over targets, first index wins ties, NaN ignored (numpy.nanargmax, gccNMFFunctions.py:138).
// One thread = four consecutive frames (S 16-byte loads, one 4-byte store).  grid = (ceil(Tp/1024), Kp, batch)
__global__ __launch_bounds__(256) void gcc_argmax_kernel(const float* __restrict__ scores, int K, int Kp, int T, int Tp, int S,
                                                         unsigned char* __restrict__ argmax) {
    const int t = 4 * (blockIdx.x * 256 + threadIdx.x);
    const int k = blockIdx.y, b = blockIdx.z;
    if (t >= Tp) return;
    unsigned char best[4] = {0, 0, 0, 0};
    if (k < K && t < T) {
        const float* row = scores + ((long)b * Kp + k) * ((long)S * Tp) + t;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        bool have[4] = {false, false, false, false};
        for (int i = 0; i < S; ++i) {
            const float4 v4 = *(const float4*)(row + (long)i * Tp);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (v[j] != v[j]) continue;
                if (!have[j] || v[j] > bv[j]) {
                    bv[j] = v[j];
                    best[j] = (unsigned char)i;
                    have[j] = true;
                }
            }
        }
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if (t + j >= T) best[j] = 0;                          // padded frames stay 0
    }
    *(uchar4*)(argmax + ((long)b * Kp + k) * Tp + t) = make_uchar4(best[0], best[1], best[2], best[3]);
}

// PHAT coherence X0*conj(X1)/|X0|/|X1| from an existing spectrogram (runGCCNMF.py:44); the pipeline gets
// it for free from the STFT epilogue, this standalone form serves the host-array API.
// grid = (ceil(T/256), F, batch)
__global__ __launch_bounds__(256) void gcc_coherence_kernel(const float2* __restrict__ X, int Fp, int T, int Tp,
                                                            float* __restrict__ CC) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int f = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    const long plane = (long)Fp * Tp;
    const float2 xl = X[(long)b * 2 * plane + (long)f * Tp + t];
    const float2 xr = X[(long)b * 2 * plane + plane + (long)f * Tp + t];
    float re, im;
    phat_coherence(xl, xr, re, im);
    float* Cb = CC + (long)b * 2 * plane + (long)f * Tp + t;
    Cb[0] = re;
    Cb[plane] = im;
}

// V = concatenate(abs(X), axis=-1) (runGCCNMF.py:40) from an existing spectrogram: V[f][c*T + t] = |X[c][f][t]|, the same hypotf as the
// STFT epilogue (fft.hip), which is where the pipeline gets V from; this standalone form serves the host-array API
// (getTargetSpectrogramEstimates called with a spectrogram that did not come from this process's STFT).
// grid = (ceil(T/256), F, batch * 2)
__global__ __launch_bounds__(256) void gcc_magnitude_kernel(const float2* __restrict__ X, int Fp, int T, int Tp, int Np,
                                                            float* __restrict__ V) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int f = blockIdx.y, b = blockIdx.z >> 1, c = blockIdx.z & 1;
    if (t >= T) return;
    const float2 x = X[((long)b * 2 + c) * Fp * Tp + (long)f * Tp + t];
    V[(long)b * Fp * Np + (long)f * Np + c * T + t] = hypotf(x.x, x.y);
}

// Hm[k][(i*2+c)*Tp + t] = H[k][c*T + t] if argmax[k][t] == i else 0 (H_c * M_i, gccNMFFunctions.py:150).
// One thread = four consecutive frames of one (target, channel) block: one 16-byte store (the write is 4/5 of this kernel's traffic:
// 1 GB per 64-file step), the arg-max as one 4-byte load; H_c starts at column c*T, which is only 4-byte aligned: scalar loads (L2).
// grid = (ceil(2*S*Tp/1024), Kp, batch)
__global__ __launch_bounds__(256) void gcc_masked_h_kernel(const float* __restrict__ H, const unsigned char* __restrict__ argmax,
                                                           const float* __restrict__ masks, int K, int Kp, int T, int Tp, int Np,
                                                           int S, float* __restrict__ Hm) {
    const int col = 4 * (blockIdx.x * 256 + threadIdx.x);
    const int k = blockIdx.y, b = blockIdx.z;
    const int ncol = 2 * S * Tp;
    if (col >= ncol) return;
    const int ic = col / Tp, t = col - ic * Tp;                 // Tp is a multiple of 64: the four frames share (target, channel)
    const int i = ic >> 1, c = ic & 1;
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < K && t < T) {
        const float* h = H + ((long)b * Kp + k) * Np + c * T + t;
        float4 m;
        if (masks) {   // arbitrary (soft) masks [batch][S][Kp][Tp]: coefficients * targetCoefficientMask
            m = *(const float4*)(masks + (((long)b * S + i) * Kp + k) * Tp + t);
        } else {
            const uchar4 a = *(const uchar4*)(argmax + ((long)b * Kp + k) * Tp + t);
            m = make_float4(a.x == i ? 1.f : 0.f, a.y == i ? 1.f : 0.f, a.z == i ? 1.f : 0.f, a.w == i ? 1.f : 0.f);
        }
        // (h * 1.0f and h * 0.0f are h and +-0: the product form IS the select for finite h, and NaN / Inf coefficients propagate as in
        // the reference's H * mask)
        out.x = h[0] * m.x;
        if (t + 1 < T) out.y = h[1] * m.y;
        if (t + 2 < T) out.z = h[2] * m.z;
        if (t + 3 < T) out.w = h[3] * m.w;
    }
    *(float4*)(Hm + ((long)b * Kp + k) * (long)ncol + col) = out;
}

// C [batch][M][ldc] = A . B with both operands stored [reduction][.] (A(i,kk) = A[kk*lda + i], B(kk,j) = B[kk*ldb + j]), plain store:
// the DFT-as-GEMM path of fft.hip (any n_fft).  Rows of A / B between Kd and the next multiple of 16 must exist and be zero;
// lda, ldb multiples of 4 and >= the tile overreach (operands padded to multiples of 64 columns).
int gccnmf_gemm_nn_store(const float* A, const float* B, float* C, int M, int N, int Kd, int lda, int ldb, int ldc, int batch, long sA,
                         long sB, long sC, hipStream_t s) {
    GemmArgs a = {};
    a.A = A; a.sA = sA; a.lda = lda; a.a_clamp = lda - 4;
    a.B = B; a.sB = sB; a.ldb = ldb; a.b_clamp = ldb - 4;
    a.M = M; a.N = N; a.Kd = Kd;
    a.batch = batch; a.xcd_affine = 0;
    a.C = C; a.sC = sC; a.ldc = ldc;
    if (gcc_small_launch(batch, a.M, a.N, a.Kd)) return gccnmf_launch_gemm_ring<false, false, EPI_STORE, false>(a, s);
    return (M > 128) ? gccnmf_launch_gemm<4, 1, false, false, EPI_STORE, false>(a, s) : gccnmf_launch_gemm<1, 4, false, false, EPI_STORE, false>(a, s);
}

extern "C" {

int gccnmf_angular_spectrogram(const float* CC, const float* trig, int F, int T, int D, int batch, float* ang,
                               double* mean_ang, void* stream) {
    GCCNMF_ENTER();
    // GCC-NONLIN rides in the upper halves of D and batch (GCCNMF_ANGULAR_NL_D / _BATCH: the float32 bits of alpha, no new entry point);
    // both zero = PHAT, every call as it was.  Every check comes before the first HIP call.
    const unsigned alpha_bits = ((unsigned)D & 0xffff0000u) | ((unsigned)batch >> 16);
    float nl_alpha = 0.f;
    if (alpha_bits) {
        __builtin_memcpy(&nl_alpha, &alpha_bits, sizeof(float));
        if (!gccnmf_nl_alpha_ok(nl_alpha)) return GCCNMF_ERR_ARG;        // alpha <= 0, NaN, Inf, subnormal -- and any negative D or batch
        D &= 0xffff;
        batch &= 0xffff;
    }
    if (!CC || !trig || !ang || F < 2 || T < 1 || D < 1 || batch < 1) return GCCNMF_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    GccNmfPitches p = gccnmf_make_pitches(F, T, 1);
    const int Dp = gccnmf_round_up(D, 64);
    if (alpha_bits) {
        const int rc = gccnmf_launch_angular_nl(CC, trig, F, T, D, batch, nl_alpha, ang, s);
        if (rc) return rc;
        if (mean_ang) {
            hipLaunchKernelGGL(ang_mean_kernel, dim3(batch * D), dim3(256), 0, s, ang, T, D, Dp, p.Tp, mean_ang);
            GCCNMF_CHECK_LAUNCH();
        }
        return GCCNMF_OK;
    }
    GemmArgs a = {};
    a.A = trig; a.sA = 0; a.lda = Dp; a.a_clamp = Dp - 4;
    a.B = CC; a.sB = 2L * p.Fp * p.Tp; a.ldb = p.Tp; a.b_clamp = p.Tp - 4;
    a.M = D; a.N = T; a.Kd = 2 * p.Fp;
    a.batch = batch; a.xcd_affine = 0;
    a.C = ang; a.sC = (long)Dp * p.Tp; a.ldc = p.Tp;
    int rc;
    if (gcc_small_launch(batch, a.M, a.N, a.Kd)) rc = gccnmf_launch_gemm_ring<false, false, EPI_STORE, false>(a, s);
    else rc = (D > 128) ? gccnmf_launch_gemm<4, 1, false, false, EPI_STORE, false>(a, s)
                        : gccnmf_launch_gemm<1, 4, false, false, EPI_STORE, false>(a, s);
    if (rc) return rc;
    if (mean_ang) {
        hipLaunchKernelGGL(ang_mean_kernel, dim3(batch * D), dim3(256), 0, s, ang, T, D, Dp, p.Tp, mean_ang);
        GCCNMF_CHECK_LAUNCH();
    }
    return GCCNMF_OK;
}

int gccnmf_pick_tdoa_peaks(const double* mean_ang, int D, int Dp, int S, int batch, int* tdoa_idx, int* status,
                           void* stream) {
    GCCNMF_ENTER();
    // time-varying tracks ride above the low byte of S (GCCNMF_PEAKS_TRACKS: bit 8, the window length L in bits 9-30); nothing above
    // the low byte = the whole-file estimate, every call as it was.  Every check comes before the first HIP call.
    // The count mode (GCCNMF_PEAKS_COUNT: bit 30 alone above the low byte, which no tracks word is -- those carry bit 8) keeps as many
    // peaks as the file has talkers (source_count.hip).
    if (S > 0 && (S & ~0xff) == GCCNMF_PEAKS_COUNT_BIT) {
        S &= 0xff;
        if (!mean_ang || !tdoa_idx || !status || D < 3 || D > SOURCE_COUNT_MAX_D || Dp < D || S < 1 || batch < 1) return GCCNMF_ERR_ARG;
        return gccnmf_launch_count_peaks(mean_ang, D, Dp, S, batch, tdoa_idx, status, (hipStream_t)stream);
    }
    if (S & ~0xff) {
        const int L = (S >> 9) & 0x3fffff, T = Dp;              // ang's pitches follow from D and T: the Dp argument carries T
        if (S < 0 || !(S & GCCNMF_PEAKS_TRACKS_BIT) || L < 1) return GCCNMF_ERR_ARG;
        S &= 0xff;
        if (!mean_ang || !tdoa_idx || !status || D < 3 || D > 4096 || T < 1 || T >= (1 << 21) || S < 1 || batch < 1 || batch > 65535)
            return GCCNMF_ERR_ARG;
        const int Tp = gccnmf_round_up(T, 64);
        hipLaunchKernelGGL(track_peaks_kernel, dim3(T, batch), dim3(64), 8 * D + 16 + gccnmf_round_up(D, 16), (hipStream_t)stream, (const float*)mean_ang, T, Tp, D,
                           gccnmf_round_up(D, 64), S, L, tdoa_idx, status);
        GCCNMF_CHECK_LAUNCH();
        hipLaunchKernelGGL(track_carry_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, T, Tp, S, tdoa_idx, status);
        GCCNMF_CHECK_LAUNCH();
        return GCCNMF_OK;
    }
    if (!mean_ang || !tdoa_idx || !status || D < 3 || D > 4096 || Dp < D || S < 1 || batch < 1) return GCCNMF_ERR_ARG;
    hipLaunchKernelGGL(pick_peaks_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, mean_ang, D, Dp, S, tdoa_idx, status);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

long gccnmf_scores_workspace_floats(int F, int T, int S, int batch) {
    GCCNMF_ENTER();
    if (F < 2 || T < 1 || S < 1 || batch < 1) return -1;
    GccNmfPitches p = gccnmf_make_pitches(F, T, 1);
    return (long)batch * p.Fp * S * p.Tp;
}

int gccnmf_target_scores_masks(const float* CC, const float* trig, const int* tdoa_idx, const float* W, int F, int T,
                               int K, int D, int S, int batch, float* workspace, float* scores, unsigned char* argmax,
                               void* stream) {
    GCCNMF_ENTER();
    // per-(target, frame) indexes ride above the low byte of S (GCCNMF_SCORES_TRACKS); every check comes before the first HIP call
    const int mode = S & ~0xff;
    // offline enhancement (atom_tdoa.hip): two further modes of this call, the arguments re-read as the header says
    if (S > 0 && mode == GCCNMF_SCORES_ATOM_TDOA) {
        if (S & 0xff) return GCCNMF_ERR_ARG;
        if (!CC || !trig || !W || !argmax || F < 2 || T < 1 || K < 1 || D < 1 || batch < 1) return GCCNMF_ERR_ARG;
        if (D > ATOM_TDOA_MAX_D || batch > 65535 || T > (1 << 19)) return GCCNMF_ERR_UNSUPPORTED;
        return gccnmf_launch_atom_tdoa(CC, trig, W, F, T, K, D, batch, (unsigned short*)argmax, scores, (hipStream_t)stream);
    }
    if (S > 0 && (mode & ~GCCNMF_SCORES_TRACKS) == GCCNMF_SCORES_ENHANCEMENT_MASKS) {
        const int window = S & 0xff;
        if (window > 1 || !CC || !trig || !tdoa_idx || (!scores && !argmax) || T < 1 || K < 1 || batch < 1) return GCCNMF_ERR_ARG;
        const float eps = trig[0], beta = trig[1], nf = trig[2];            // three HOST floats
        if (!(eps > 0.f && eps < INFINITY && beta > 0.f && beta < INFINITY && nf >= 0.f && nf < INFINITY)) return GCCNMF_ERR_ARG;
        if (batch > 65535 || K > 65535 - 63) return GCCNMF_ERR_UNSUPPORTED;
        return gccnmf_launch_enhancement_masks((const unsigned short*)CC, tdoa_idx, (mode & GCCNMF_SCORES_TRACKS) ? 1 : 0, window, eps,
                                               beta, nf, T, K, batch, argmax, scores, (hipStream_t)stream);
    }
    // absent targets (GCCNMF_SCORES_COUNTED: a negative index is a target the file does not have) -- with the fixed indexes only
    if (S < 0 || ((mode & ~GCCNMF_SCORES_TRACKS) && mode != GCCNMF_SCORES_COUNTED)) return GCCNMF_ERR_ARG;
    S &= 0xff;
    const bool tracks = mode == GCCNMF_SCORES_TRACKS, counted = mode == GCCNMF_SCORES_COUNTED;
    if (!CC || !trig || !tdoa_idx || !W || !workspace || !scores || F < 2 || T < 1 || K < 1 || D < 1 || S < 1 || batch < 1)
        return GCCNMF_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    GccNmfPitches p = gccnmf_make_pitches(F, T, K);
    const int Dp = gccnmf_round_up(D, 64);
    const int ncol = S * p.Tp;
    float* P = workspace;
    if (counted)
        hipLaunchKernelGGL((gcc_steer_kernel<false, true>), dim3(gccnmf_ceil_div(ncol, 1024), p.Fp, batch), dim3(256), 0, s, CC, trig,
                           tdoa_idx, F, p.Fp, T, p.Tp, D, Dp, S, P);
    else if (tracks)
        hipLaunchKernelGGL((gcc_steer_kernel<true, false>), dim3(gccnmf_ceil_div(ncol, 1024), p.Fp, batch), dim3(256), 0, s, CC, trig, tdoa_idx,
                           F, p.Fp, T, p.Tp, D, Dp, S, P);
    else
        hipLaunchKernelGGL((gcc_steer_kernel<false, false>), dim3(gccnmf_ceil_div(ncol, 1024), p.Fp, batch), dim3(256), 0, s, CC, trig, tdoa_idx,
                           F, p.Fp, T, p.Tp, D, Dp, S, P);
    GCCNMF_CHECK_LAUNCH();
    GemmArgs a = {};
    a.A = W; a.sA = (long)p.Fp * p.Kp; a.lda = p.Kp; a.a_clamp = p.Kp - 4;
    a.B = P; a.sB = (long)p.Fp * ncol; a.ldb = ncol; a.b_clamp = ncol - 4;
    a.M = K; a.N = ncol; a.Kd = F;
    if ((F % 16) == 1) {
        a.Kd = F - 1;
        a.ktailA = W + (long)(F - 1) * p.Kp; a.s_ktailA = a.sA;
        a.ktailB = P + (long)(F - 1) * ncol; a.s_ktailB = a.sB;
    }
    a.batch = batch; a.xcd_affine = 1;
    a.C = scores; a.sC = (long)p.Kp * ncol; a.ldc = ncol;
    int rc;
    if (gcc_small_launch(batch, a.M, a.N, a.Kd)) rc = gccnmf_launch_gemm_ring<false, false, EPI_STORE, false>(a, s);
    else if (K > 128 && gccnmf_tune_dma) rc = gccnmf_launch_gemm_dma<false, false, EPI_STORE, false>(a, s);
    else rc = (K > 128) ? gccnmf_launch_gemm<4, 1, false, false, EPI_STORE, false>(a, s)
                        : gccnmf_launch_gemm<1, 4, false, false, EPI_STORE, false>(a, s);
    if (rc) return rc;
    if (argmax) {
        hipLaunchKernelGGL(gcc_argmax_kernel, dim3(gccnmf_ceil_div(p.Tp, 1024), p.Kp, batch), dim3(256), 0, s, scores, K, p.Kp, T,
                           p.Tp, S, argmax);
        GCCNMF_CHECK_LAUNCH();
    }
    return GCCNMF_OK;
}

int gccnmf_argmax_targets(const float* scores, int K, int T, int S, int batch, unsigned char* argmax, void* stream) {
    GCCNMF_ENTER();
    if (!scores || !argmax || K < 1 || T < 1 || S < 1 || S > 255 || batch < 1) return GCCNMF_ERR_ARG;
    GccNmfPitches p = gccnmf_make_pitches(2, T, K);
    hipLaunchKernelGGL(gcc_argmax_kernel, dim3(gccnmf_ceil_div(p.Tp, 1024), p.Kp, batch), dim3(256), 0, (hipStream_t)stream, scores,
                       K, p.Kp, T, p.Tp, S, argmax);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

int gccnmf_coherence(const float* X, int F, int T, int batch, float* CC, void* stream) {
    GCCNMF_ENTER();
    if (!X || !CC || F < 2 || T < 1 || batch < 1) return GCCNMF_ERR_ARG;
    GccNmfPitches p = gccnmf_make_pitches(F, T, 1);
    hipLaunchKernelGGL(gcc_coherence_kernel, dim3(gccnmf_ceil_div(T, 256), F, batch), dim3(256), 0, (hipStream_t)stream,
                       (const float2*)X, p.Fp, T, p.Tp, CC);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

int gccnmf_magnitude(const float* X, int F, int T, int batch, float* V, void* stream) {
    GCCNMF_ENTER();
    if (!X || !V || F < 2 || T < 1 || batch < 1) return GCCNMF_ERR_ARG;
    GccNmfPitches p = gccnmf_make_pitches(F, T, 1);
    hipLaunchKernelGGL(gcc_magnitude_kernel, dim3(gccnmf_ceil_div(T, 256), F, batch * 2), dim3(256), 0, (hipStream_t)stream,
                       (const float2*)X, p.Fp, T, p.Tp, p.Np, V);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

long gccnmf_reconstruct_workspace_floats(int T, int K, int S, int batch) {
    GCCNMF_ENTER();
    if (T < 1 || K < 1 || S < 1 || batch < 1) return -1;
    GccNmfPitches p = gccnmf_make_pitches(2, T, K);
    return (long)batch * p.Kp * 2 * S * p.Tp;
}

int gccnmf_reconstruct(const float* W, const float* H, const unsigned char* argmax, const float* masks, const float* X,
                       const float* V, int F, int T, int K, int S, int batch, float* workspace, float* spec, void* stream) {
    GCCNMF_ENTER();
    // the modes ride above the low byte of S (GCCNMF_RECONSTRUCT_RATIO) and in the upper half of batch (GCCNMF_RECONSTRUCT_SPATIAL_BATCH);
    // every check comes before the first HIP call
    const int mode = S & ~0xff;
    S &= 0xff;
    if (mode & ~(GCCNMF_RECONSTRUCT_RATIO | GCCNMF_RECONSTRUCT_SPATIAL_ITERATIONS(0xff))) return GCCNMF_ERR_ARG;
    const bool ratio = (mode & GCCNMF_RECONSTRUCT_RATIO) != 0;      // needs neither V nor the masked-H workspace
    const int iterations = (mode >> 20) & 0xff;              // EM iterations of the spatial mode: the powers follow the covariances in workspace
    if (batch < 1 || (batch & ~(0xffff | GCCNMF_RECONSTRUCT_SPATIAL_BIT))) return GCCNMF_ERR_ARG;
    const bool spatial = (batch & GCCNMF_RECONSTRUCT_SPATIAL_BIT) != 0;     // the spatial filter behind the ratio stage: covariances in workspace
    batch &= 0xffff;
    if (spatial && !ratio) return GCCNMF_ERR_ARG;
    if (iterations && !spatial) return GCCNMF_ERR_ARG;
    if (!W || !H || (!argmax && !masks) || !X || (!ratio && (!V || !workspace)) || !spec || F < 2 || T < 1 || K < 1 || S < 1 || batch < 1)
        return GCCNMF_ERR_ARG;
    if (spatial && (!workspace || ((uintptr_t)workspace & 15))) return GCCNMF_ERR_ARG;
    if (ratio && S > GCCNMF_RATIO_MAX_TARGETS) return GCCNMF_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (ratio) {
        const int rc = gccnmf_launch_ratio(W, H, argmax, masks, X, F, T, K, S, batch, spec, s);
        if (rc != GCCNMF_OK || !spatial) return rc;
        if (!iterations) return gccnmf_launch_spatial(X, F, T, S, batch, workspace, spec, s);
        GccNmfPitches p = gccnmf_make_pitches(F, T, 1);
        float* powers = workspace + GCCNMF_RECONSTRUCT_SPATIAL_WORKSPACE_FLOATS(batch, S, p.Fp);
        return gccnmf_launch_spatial_em(X, F, T, S, batch, iterations, workspace, powers, spec, s);
    }
    GccNmfPitches p = gccnmf_make_pitches(F, T, K);
    const int ncol = 2 * S * p.Tp;
    float* Hm = workspace;
    hipLaunchKernelGGL(gcc_masked_h_kernel, dim3(gccnmf_ceil_div(ncol, 1024), p.Kp, batch), dim3(256), 0, s, H, argmax, masks, K, p.Kp,
                       T, p.Tp, p.Np, S, Hm);
    GCCNMF_CHECK_LAUNCH();
    const bool tail = (F % 128) == 1;
    GemmArgs a = {};
    a.A = W; a.sA = (long)p.Fp * p.Kp; a.lda = p.Kp; a.a_clamp = p.Fp - 1;
    a.B = Hm; a.sB = (long)p.Kp * ncol; a.ldb = ncol; a.b_clamp = ncol - 4;
    a.M = tail ? F - 1 : F; a.N = ncol; a.Kd = K;
    a.tail_row = F - 1;
    a.batch = batch; a.xcd_affine = 1;
    a.C = spec; a.sC = 2L * S * p.Fp * p.Tp;   // in float2 units (EPI_PHASE indexes complex elements)
    a.E0 = V; a.sE0 = (long)p.Fp * p.Np;
    a.X = (const float2*)X; a.sX = 2L * p.Fp * p.Tp;
    a.T = T; a.Tp = p.Tp; a.Fp = p.Fp; a.ldv = p.Np;
    if (gcc_small_launch(batch, a.M, a.N, a.Kd))
        return tail ? gccnmf_launch_gemm_ring<true, false, EPI_PHASE, true>(a, s) : gccnmf_launch_gemm_ring<true, false, EPI_PHASE, false>(a, s);
    const bool tall = a.M > 128;
    // batch scale: the LDS-DMA throughput tile (main loop of K1) with the generic phase epilogue
    if (tall && gccnmf_tune_dma)
        return tail ? gccnmf_launch_gemm_dma<true, false, EPI_PHASE, true>(a, s) : gccnmf_launch_gemm_dma<true, false, EPI_PHASE, false>(a, s);
    if (tall) return tail ? gccnmf_launch_gemm<4, 1, true, false, EPI_PHASE, true>(a, s)
                          : gccnmf_launch_gemm<4, 1, true, false, EPI_PHASE, false>(a, s);
    return tail ? gccnmf_launch_gemm<1, 4, true, false, EPI_PHASE, true>(a, s)
                : gccnmf_launch_gemm<1, 4, true, false, EPI_PHASE, false>(a, s);
}

}  // extern "C"
