// Streaming (real-time) GCC-NMF frame processor on gfx950 -- SURVEY.md section 8f #1 and #4.
// Reference: gccNMF/realtime/gccNMFProcessor.py:201-270 (the Theano graph + processFrames) and
// gccNMF/realtime/utils.py:72-118 (OverlapAddProcessor), :34-70 (history ring).
//
// One block of `blockSize` new stereo samples per call; Tc = blockSize/hopSize analysis windows per call.
// Latency-bound, not throughput-bound: everything is sized so that a call is six short launches on one stream and the
// only host traffic is the new block in and the finished block out.
//   rt_shift      8-block input / output buffers move one block left, new samples appended          (utils.py:99-103)
//   rt_frames     sqrt-hamming window, both channels in one packed complex FFT, X and PHAT coherence (processor :202,:253)
//   rt_gccnmf     S[tau,k] = sum_f Re(C[f] e^{-j w tau}) W[f,k] on the matrix cores, arg-max over tau,
//                 soft / boxcar coefficient mask around the tracked target TDOA                      (:254,:259-265)
//   rt_tfmask     tfMask[f] = sum_k W[f,k] HMask[k] / sum_k W[f,k];  Y = tfMask * X                  (:267-269,:209)
//   rt_synth      packed inverse FFT, synthesis window, overlap-add, hand out the block two blocks old (:231, utils.py:113-116)
//   rt_localize   gccPHAT[tau] = nanmean_f G, history ring, target = argmax nanmean(last L columns)   (:214-222)
// NaN semantics follow the reference here (a zero-magnitude bin makes the frame's GCC-NMF scores NaN and its arg-max 0;
// nanmean skips it), because the localisation history depends on them.
//
// Stream bank (frames_mode bit 3, include/gccnmf_hip.h): S independent streams of one configuration in the same launches, so that
// one GPU serves many real-time sessions with the same six launches and one host sync per block (StreamingGCCNMFBank; config 5 at
// S = 256: 0.59 ms per 4 ms block for all streams, 0.042 of one stream's device cost per stream; LABBOOK R7.1).  Stream s is
// blockIdx.z of every kernel; each per-stream buffer holds S consecutive single-stream images and a kernel first moves its base pointers
// to image s (64-bit offsets), so the arithmetic of one stream is that of the single-stream call, which is the S = 1 case.  The
// per-stream switches are words 4 (separation) and 5 (localisation) of the stream's 8-word target row.
//
// Multiple mode (frames_mode bit 20, TARGET_MODE_MULTIPLE): N <= 8 target TDOA indexes per stream (words 8.. of a 16-word row), one-hot
// arg-max-over-targets masks from the scores rt_gccnmf already sums, N masked spectra, N synthesis rings (blockIdx.y), the N largest
// gccPHAT peaks tracked.  Every one of its kernels is the `true` / 16-word / RT_MAX_TARGETS instantiation of a template whose other
// instantiation is the single-target kernel (LABBOOK R7.3); the entry point picks between the two in one place
// (RT_KERNEL).  Eleven kernels are launched from here.
//
// Online spatial filter (separation_enabled bit 1, GCCNMF_RT_SEPARATION_SPATIAL): one more launch between the mask and the synthesis kernel,
// in a file of its own (rt_spatial.hip), so that the code objects of the kernels below are what they were.  Its per-stream state lies
// behind the history images of `hist`; a stream's word 7 of the target row holds its time constant.
#include "fft_core.h"
#include "angular_nl.h"
#include "rt_spatial.h"
#include "../../include/gccnmf_hip.h"

typedef float rt_f32x16 __attribute__((ext_vector_type(16)));

#define RT_ROW 8                                           // bank layout: target row {index, eps, beta, noiseFloor, sep, loc, nlAlpha, 0}
#define RT_ROW_MULTI 16                                    // multi-target layout (frames_mode bit 20): the 8 words above + tau_0 .. tau_7
#define RT_MAX_TARGETS 8

// rows = the bank's [S][ROW] target rows, NULL outside the bank layout: true when this workgroup's stream has `word` switched off
template <int ROW = RT_ROW>
__device__ __forceinline__ bool rt_switched_off(const float* rows, int word) {
    return rows && rows[(long)blockIdx.z * ROW + word] == 0.f;
}

// ---- rt_shift: one workgroup per stream, in-place left shift by B of both 8-block buffers ---------------------------
// MULTI (multi-target layout): grid = (1, N, S), out_ring holds N rings per stream; workgroup y shifts ring y, workgroup 0 also the input
template <bool MULTI>
__global__ __launch_bounds__(1024) void rt_shift_kernel(float* __restrict__ in_ring, float* __restrict__ out_ring,
                                                        const float* __restrict__ block_in, int B, int ring) {
    const long sid = blockIdx.z;
    in_ring += sid * 2 * ring;
    if constexpr (MULTI)
        out_ring += (sid * gridDim.y + blockIdx.y) * 2 * ring;
    else
        out_ring += sid * 2 * ring;
    block_in += sid * 2 * B;
    // ring = 8*B samples per channel, 2 channels.  Chunks of 8192 values in ascending order, every thread loading everything it
    // will store before the barrier: a chunk reads at or above the positions it writes (never below), so no later chunk's stores can
    // reach what an earlier one still has to read -- any block size, one workgroup (the reference's buffers have no size limit,
    // realtime/utils.py:72-97).
    const int total = 2 * ring;
    for (int base = 0; base < total; base += 8192) {
        float vin[8], vout[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int i = base + threadIdx.x + 1024 * n;
            vin[n] = vout[n] = 0.f;
            if (i < total) {
                const int c = i / ring, s = i - c * ring;
                if (!MULTI || blockIdx.y == 0) vin[n] = (s + B < ring) ? in_ring[c * ring + s + B] : block_in[c * B + (s + B - ring)];
                vout[n] = (s + B < ring) ? out_ring[c * ring + s + B] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int i = base + threadIdx.x + 1024 * n;
            if (i < total) {
                if (!MULTI || blockIdx.y == 0) in_ring[i] = vin[n];
                out_ring[i] = vout[n];
            }
        }
        __syncthreads();
    }
}

// ---- rt_frames: grid = (Tc, 1, S), one analysis window per workgroup ----------------------------------------------------
__global__ __launch_bounds__(FFT_NT) void rt_frames_kernel(const float* __restrict__ in_ring, int ring, int N, int logN, int start0,
                                                           int start_step, int Tc, const float* __restrict__ window,
                                                           const float2* __restrict__ twiddle, float2* __restrict__ X,
                                                           float2* __restrict__ C) {
    extern __shared__ __attribute__((aligned(16))) float2 rt_smem[];
    float2* z = rt_smem;
    float2* tw = rt_smem + N;
    const int t = blockIdx.x;
    const int F = N / 2 + 1;
    const int start = start0 + t * start_step;            // ring mode: utils.py:105; frames mode: t * N
    in_ring += (long)blockIdx.z * 2 * ring;
    for (int i = threadIdx.x; i < N / 2; i += FFT_NT) tw[i] = twiddle[i];
    for (int n = threadIdx.x; n < N; n += FFT_NT) {
        const float w = window[n];
        z[bitrev(n, logN)] = make_float2(w * in_ring[start + n], w * in_ring[ring + start + n]);
    }
    __syncthreads();
    fft_stages<false, 1>(z, tw, N, logN, N);
    const long cr0 = (long)blockIdx.z * F, xr0 = 2 * cr0;           // first row of this stream's image
    for (int f = threadIdx.x; f < F; f += FFT_NT) {
        const float2 zk = z[f], zn = z[(N - f) & (N - 1)];
        const float2 XL = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));     // rfft, NOT conjugated (:202)
        const float2 XR = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
        X[(xr0 + f) * Tc + t] = XL;
        X[(xr0 + F + f) * Tc + t] = XR;
        const float aL = hypotf(XL.x, XL.y), aR = hypotf(XR.x, XR.y);
        float re = XL.x * XR.x + XL.y * XR.y, im = XL.y * XR.x - XL.x * XR.y;
        C[(cr0 + f) * Tc + t] = make_float2(re / aL / aR, im / aL / aR);                   // 0/0 -> NaN like the reference (:253)
    }
}

// ---- rt_gccnmf: grid = (Kp/32, Tc, S); 32 atoms per workgroup, the 4 waves split the reduction over f ------------------------------
// MFMA 32x32x2: A[i = tau][k = f] = G[f][tau] built on the fly from the steering tables, B[k = f][j = atom] = W[f][atom].
// Latency matters here, not throughput (33.7 MFLOP per frame): the first version ran 16 workgroups with a 129-step chain of
// dependent global loads (31 us).  Now each of 8 waves owns an eighth of the frequency rows (17 steps at n_fft = 512: ONE batch of
// loads, all issued before the first use, two TDOA tiles per pass sharing the W and C loads), the partial accumulators meet in
// LDS, and 32 atoms per workgroup double the number of CUs at work.
// MULTI (frames_mode bit 20): `ntargets` target rows tau_i = words 8.. of the stream's 16-word row.  Wave 0's per-row pass keeps the
// total of every row that is a target (the same sum the arg-max over tau sees, bit for bit), and the one-hot masks
// HMask[i][atom][t] = (i == nanargmax_i G[tau_i]) replace the windowed mask; argmaxTDOA is written as in the single-target form.
#define RT_G_WAVES 8
#define RT_G_CHUNK 17
template <bool MULTI>
__global__ __launch_bounds__(64 * RT_G_WAVES) void rt_gccnmf_kernel(const float2* __restrict__ C, const float* __restrict__ cosT,
                                                        const float* __restrict__ sinT, const float* __restrict__ W, int F, int K,
                                                        int Kp, int D, int Dp, int Tc, const float* __restrict__ target,
                                                        int target_mode, int bank, float* __restrict__ HMask, int* __restrict__ argmaxTDOA,
                                                        int ntargets) {
    __shared__ float s_part[RT_G_WAVES - 1][32][64];      // partial accumulators (two TDOA tiles) of the other waves
    const long sid = blockIdx.z;
    target += sid * (MULTI ? RT_ROW_MULTI : RT_ROW);
    if (bank && target[4] == 0.f) return;                 // this stream's separation is off
    C += sid * F * Tc;
    HMask += sid * (MULTI ? ntargets : 1) * Kp * Tc;
    if (argmaxTDOA) argmaxTDOA += sid * Kp * Tc;
    const int t = blockIdx.y, k0 = blockIdx.x * 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int atom = k0 + l31;
    // frequency rows of this wave: an even number per wave so that the two lane halves (k = 0 / 1 of an MFMA step) pair up
    const int per = ((F + 2 * RT_G_WAVES - 1) / (2 * RT_G_WAVES)) * 2;
    const int f_lo = wave * per, f_hi = min(f_lo + per, F);
    const int steps = (f_hi - f_lo + 1) / 2;
    float best_val = -INFINITY;
    int best_idx = 0;
    int tg[RT_MAX_TARGETS];                               // MULTI: the target rows (-1: no target), uniform over the workgroup
    float cap[RT_MAX_TARGETS];                            // MULTI: this lane's total of row tg[i] (NaN until seen)
#pragma unroll
    for (int i = 0; i < RT_MAX_TARGETS; ++i) {
        tg[i] = (MULTI && i < ntargets) ? (int)target[8 + i] : -1;
        cap[i] = NAN;
    }
    // two TDOA tiles per pass (they share the W and C loads; D = 64 is one pass), 16 steps' loads in flight together
    for (int tt = 0; tt * 32 < Dp; tt += 2) {
        rt_f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
        const bool two = (tt + 1) * 32 < Dp;
        const int tau0 = tt * 32 + l31, tau1 = two ? tau0 + 32 : tau0;
        for (int p0 = 0; p0 < steps; p0 += RT_G_CHUNK) {
            // raw loads first, ALL of them (the scheduler otherwise sinks them next to their uses and the chunk degenerates into a
            // chain of one or two outstanding loads: measured 19 us for the kernel), then the arithmetic
            float2 cv[RT_G_CHUNK];
            float c0[RT_G_CHUNK], s0[RT_G_CHUNK], c1[RT_G_CHUNK], s1[RT_G_CHUNK], bv[RT_G_CHUNK];
#pragma unroll
            for (int u = 0; u < RT_G_CHUNK; ++u) {         // (clamped row, masked below)
                const int f = min(f_lo + 2 * (p0 + u) + hh, F - 1);
                cv[u] = C[f * Tc + t];
                c0[u] = cosT[f * Dp + tau0];
                s0[u] = sinT[f * Dp + tau0];
                c1[u] = cosT[f * Dp + tau1];
                s1[u] = sinT[f * Dp + tau1];
                bv[u] = W[f * Kp + atom];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < RT_G_CHUNK; ++u) {
                const bool ok = (p0 + u) < steps && (f_lo + 2 * (p0 + u) + hh) < f_hi;
                const float b = ok ? bv[u] : 0.f;
                const float a0 = cv[u].x * c0[u] + cv[u].y * s0[u], a1 = cv[u].x * c1[u] + cv[u].y * s1[u];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ok ? a0 : 0.f, b, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ok ? a1 : 0.f, b, acc1, 0, 0, 0);
            }
        }
        if (wave > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s_part[wave - 1][r][lane] = acc0[r];
                s_part[wave - 1][16 + r][lane] = acc1[r];
            }
        }
        __syncthreads();
        if (wave == 0) {
            // total of the waves' partial sums, then the arg-max over the 32 TDOAs of each tile for the lane's atom:
            // rows (r&3) + 8*(r>>2) + 4*hh, ascending within a lane, tiles in ascending order
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                if (half == 1 && !two) break;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float own = half ? acc1[r] : acc0[r];
                    float v = own;                              // fixed order: w0 + w1 + ... + w7
#pragma unroll
                    for (int w = 0; w < RT_G_WAVES - 1; ++w) v += s_part[w][16 * half + r][lane];
                    const int row = (tt + half) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                    if (row < D && (v > best_val || (v == best_val && row < best_idx))) {
                        best_val = v;
                        best_idx = row;
                    }
                    if constexpr (MULTI) {
#pragma unroll
                        for (int i = 0; i < RT_MAX_TARGETS; ++i)
                            if (row == tg[i]) cap[i] = v;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (wave == 0) {
        const float ov = __shfl_xor(best_val, 32);        // the other row half
        const int oi = __shfl_xor(best_idx, 32);
        if (ov > best_val || (ov == best_val && oi < best_idx)) {
            best_val = ov;
            best_idx = oi;
        }
        if constexpr (MULTI) {
            // row tau lies in lane half (tau >> 2) & 1; nanargmax over the targets: first maximum wins, NaN ignored, all NaN -> 0
            int bi = 0;
            float bv = NAN;
#pragma unroll
            for (int i = 0; i < RT_MAX_TARGETS; ++i) {
                const float o = __shfl_xor(cap[i], 32);
                const float g = (((tg[i] >> 2) & 1) == hh) ? cap[i] : o;
                if (i < ntargets && g == g && (bv != bv || g > bv)) {
                    bv = g;
                    bi = i;
                }
            }
            if (hh == 0 && atom < K) {
                for (int i = 0; i < ntargets; ++i) HMask[((long)i * Kp + atom) * Tc + t] = (i == bi) ? 1.f : 0.f;
                if (argmaxTDOA) argmaxTDOA[(long)atom * Tc + t] = (best_val > -INFINITY) ? best_idx : 0;
            }
        } else if (hh == 0 && atom < K) {
            int i = best_idx;
            if (!(best_val > -INFINITY)) i = 0;           // every score NaN (or D == 0): numpy.argmax of an all-NaN column is 0
            const float tgt = target[0], eps = target[1], beta = target[2], nf = target[3];
            const float dist = fabsf((float)i - tgt);
            float m;
            if (target_mode == 0)
                m = dist < eps ? 1.f : 0.f;                                   // TARGET_MODE_BOXCAR (:263)
            else
                m = expf(-powf(dist / eps, beta)) / (1.f + nf) + nf;          // TARGET_MODE_WINDOW_FUNCTION (:265)
            HMask[(long)atom * Tc + t] = m;
            if (argmaxTDOA) argmaxTDOA[(long)atom * Tc + t] = i;
        }
    }
}

// ---- rt_tfmask: one wave per frequency row; grid = (ceil(F/4), 1, S) ------------------------------------------------------
// MAXT = 1: the single-target layout (8-word rows; nt is not read).  tfMask's per-stream image is [2][F][Tc] here too, the size the
// coefficient-inference mask needs.
// MAXT = RT_MAX_TARGETS: the multi-target layout (frames_mode bit 20, 16-word rows): HMask [nt][Kp][Tc], Y and tfMask [nt][2][F][Tc] per
// stream.  One pass over the row of W makes all nt numerators (the loads of W are shared); numerator i is summed in the denominator's
// order (the lane-strided chain, the same shuffle tree), so with nt = 1 (HMask = 1) every quotient is 1.0 exactly.
// No contraction in the body: every fused operation is an fmaf, every other one rounds on its own (what the build always produced here).
template <int MAXT>
__global__ __launch_bounds__(256) void rt_tfmask_kernel(const float* __restrict__ W, const float* __restrict__ HMask, int F, int K,
                                                        int Kp, int Tc, const float2* __restrict__ X, float2* __restrict__ Y,
                                                        float* __restrict__ tfMask, const float* __restrict__ rows, int nt) {
#pragma clang fp contract(off)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.x * 4 + wave;
    if (f >= F || rt_switched_off<MAXT == 1 ? RT_ROW : RT_ROW_MULTI>(rows, 4)) return;
    if (MAXT == 1) nt = 1;
    const long sid = blockIdx.z;
    const long hplane = (long)Kp * Tc, yplane = 2L * F * Tc;
    HMask += sid * nt * hplane;
    X += sid * yplane;
    Y += sid * nt * yplane;
    tfMask += sid * nt * yplane;
    const float* Wr = W + (long)f * Kp;
    float rec = 0.f;
    for (int k = lane; k < K; k += 64) rec += Wr[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rec += __shfl_xor(rec, o);
    for (int t = 0; t < Tc; ++t) {
        float s[MAXT];
#pragma unroll
        for (int i = 0; i < MAXT; ++i) s[i] = 0.f;
        for (int k = lane; k < K; k += 64) {
            const float w = Wr[k];
#pragma unroll
            for (int i = 0; i < MAXT; ++i)
                if (i < nt) s[i] = fmaf(w, HMask[i * hplane + (long)k * Tc + t], s[i]);
        }
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
            if (i < nt) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s[i] += __shfl_xor(s[i], o);
            }
        }
        if (lane == 0) {
            const float2 a = X[(long)f * Tc + t], b = X[((long)F + f) * Tc + t];
#pragma unroll
            for (int i = 0; i < MAXT; ++i) {
                if (i < nt) {
                    const float m = s[i] / rec;
                    tfMask[i * yplane + (long)f * Tc + t] = m;
                    Y[i * yplane + (long)f * Tc + t] = make_float2(m * a.x, m * a.y);
                    Y[i * yplane + ((long)F + f) * Tc + t] = make_float2(m * b.x, m * b.y);
                }
            }
        }
    }
}

// ---- rt_synth: one workgroup per stream; frames in order (their output ranges overlap) ----------------------------------------
// Y = the spectra to synthesise; in the bank layout (rows != NULL) a stream whose separation is off takes X instead
// MULTI: grid y = N targets, one overlap-add ring per target (out_ring [N][2][ring], block_out [N][2][B] per stream); Y == X (separation
// off for the call) or a stream switched off synthesises the mixture into every one of its N rings
template <bool MULTI>
__global__ __launch_bounds__(FFT_NT) void rt_synth_kernel(const float2* __restrict__ Y, int N, int logN, int start0, int start_step,
                                                          int accumulate, int Tc, int ring, int B, int out_delay,
                                                          const float* __restrict__ window, const float2* __restrict__ twiddle,
                                                          float* __restrict__ out_ring, float* __restrict__ block_out,
                                                          const float2* __restrict__ X, const float* __restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) float2 rt_smem[];
    float2* z = rt_smem;
    float2* tw = rt_smem + N;
    const int F = N / 2 + 1;
    const long sid = blockIdx.z;
    if constexpr (MULTI) {
        const long img = sid * gridDim.y + blockIdx.y;
        Y = (Y == X || rt_switched_off<RT_ROW_MULTI>(rows, 4)) ? X + sid * 2 * F * Tc : Y + img * 2 * F * Tc;
        out_ring += img * 2 * ring;
        block_out += img * 2 * B;
    } else {
        if (rt_switched_off(rows, 4)) Y = X;
        Y += sid * 2 * F * Tc;
        out_ring += sid * 2 * ring;
        block_out += sid * 2 * B;
    }
    const float invN = 1.f / (float)N;
    for (int i = threadIdx.x; i < N / 2; i += FFT_NT) tw[i] = twiddle[i];
    for (int t = 0; t < Tc; ++t) {
        __syncthreads();
        for (int f = threadIdx.x; f < F; f += FFT_NT) {
            float2 a = Y[(long)f * Tc + t], b = Y[((long)F + f) * Tc + t];
            if (f == 0 || f == N / 2) {      // numpy.fft.irfft ignores the imaginary part of DC and Nyquist
                a.y = 0.f;
                b.y = 0.f;
            }
            z[bitrev(f, logN)] = make_float2(a.x - b.y, a.y + b.x);
            if (f != 0 && f != N / 2) z[bitrev(N - f, logN)] = make_float2(a.x + b.y, b.x - a.y);
        }
        __syncthreads();
        fft_stages<true, 1>(z, tw, N, logN, N);
        const int start = start0 + t * start_step;
        for (int n = threadIdx.x; n < N; n += FFT_NT) {
            const float w = window[n];
            const float ya = w * (z[n].x * invN), yb = w * (z[n].y * invN);
            if (accumulate) {                    // overlap-add into the output buffer (utils.py:113-114)
                out_ring[start + n] += ya;
                out_ring[ring + start + n] += yb;
            } else {                             // frames mode: the processed frames themselves (:231)
                out_ring[start + n] = ya;
                out_ring[ring + start + n] = yb;
            }
        }
    }
    if (!accumulate) return;
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * B; i += FFT_NT) {
        const int c = i / B, s = i - c * B;
        block_out[i] = out_ring[c * ring + ring - (out_delay + 1) * B + s];           // utils.py:116 (out_delay = 2 there)
    }
}

// ---- any even window size (the reference takes every windowSize: numpy.fft.rfft / irfft, gccNMFProcessor.py:202,:231) -------------
// Off the powers of two the transform is evaluated as the sum it is, against a full-circle table (cos, sin)(2 pi k / N), k < N, computed
// in float64 on the host: a frame is 2 x (N/2 + 1) x N complex MACs (N = 1000: 4 MFLOP) -- nothing on this chip, and no mixed-radix
// machinery for a path whose defaults are powers of two.  The angle index f * n mod N advances by one addition and one compare.
// rt_frames_dft: grid = (ceil(F / 64), Tc, S), 256 threads = 64 frequencies x 4 segments of n (partial sums added in segment order).
__global__ __launch_bounds__(256) void rt_frames_dft_kernel(const float* __restrict__ in_ring, int ring, int N, int start0, int start_step,
                                                            int Tc, const float* __restrict__ window, const float2* __restrict__ table,
                                                            float2* __restrict__ X, float2* __restrict__ C) {
    extern __shared__ __attribute__((aligned(16))) float2 rt_smem[];
    float2* xw = rt_smem;                  // windowed samples (left, right)
    float2* tb = rt_smem + N;
    __shared__ float4 s_part[4][64];
    const int t = blockIdx.y, F = N / 2 + 1;
    const int start = start0 + t * start_step;
    const long sid = blockIdx.z;
    in_ring += sid * 2 * ring;
    X += sid * 2 * F * Tc;
    C += sid * F * Tc;
    for (int n = threadIdx.x; n < N; n += 256) {
        const float w = window[n];
        xw[n] = make_float2(w * in_ring[start + n], w * in_ring[ring + start + n]);
        tb[n] = table[n];
    }
    __syncthreads();
    const int fl = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int f = min(blockIdx.x * 64 + fl, F - 1);
    const int n0 = (int)(((long)N * seg) / 4), n1 = (int)(((long)N * (seg + 1)) / 4);
    int idx = (int)(((long)f * n0) % N);
    float reL = 0.f, imL = 0.f, reR = 0.f, imR = 0.f;
    for (int n = n0; n < n1; ++n) {
        const float2 c = tb[idx], x = xw[n];           // e^{-j theta} = cos - j sin (rfft, NOT conjugated, :202)
        reL = fmaf(x.x, c.x, reL); imL = fmaf(-x.x, c.y, imL);
        reR = fmaf(x.y, c.x, reR); imR = fmaf(-x.y, c.y, imR);
        idx += f;
        if (idx >= N) idx -= N;
    }
    s_part[seg][fl] = make_float4(reL, imL, reR, imR);
    __syncthreads();
    if (seg == 0 && blockIdx.x * 64 + fl < F) {
        float4 a = s_part[0][fl];
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            const float4 b = s_part[q][fl];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        const float2 XL = make_float2(a.x, a.y), XR = make_float2(a.z, a.w);
        X[(long)f * Tc + t] = XL;
        X[((long)F + f) * Tc + t] = XR;
        const float aL = hypotf(XL.x, XL.y), aR = hypotf(XR.x, XR.y);
        const float re = XL.x * XR.x + XL.y * XR.y, im = XL.y * XR.x - XL.x * XR.y;
        C[(long)f * Tc + t] = make_float2(re / aL / aR, im / aL / aR);                   // 0/0 -> NaN like the reference (:253)
    }
}

// rt_synth_dft: one thread per OUTPUT position of the buffer (both channels), frames in ascending order -- the reference's accumulation
// order (utils.py:113-114), and no two threads ever add into the same sample.  grid = (ceil(positions / 256), 1, S); s_lo = first position.
// X / rows: as for rt_synth.
// MULTI: as rt_synth (grid y = N targets)
template <bool MULTI>
__global__ __launch_bounds__(256) void rt_synth_dft_kernel(const float2* __restrict__ Y, int N, int start0, int start_step, int accumulate,
                                                           int Tc, int ring, int B, int out_delay, int s_lo, const float* __restrict__ window,
                                                           const float2* __restrict__ table, float* __restrict__ out_ring,
                                                           float* __restrict__ block_out, const float2* __restrict__ X,
                                                           const float* __restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) float2 rt_smem[];
    float2* tb = rt_smem;                  // [N]
    float2* ya = rt_smem + N;              // [F] left
    float2* yb = ya + (N / 2 + 1);         // [F] right
    const int F = N / 2 + 1, H = N / 2;
    const long sid = blockIdx.z;
    if constexpr (MULTI) {
        const long img = sid * gridDim.y + blockIdx.y;
        Y = (Y == X || rt_switched_off<RT_ROW_MULTI>(rows, 4)) ? X + sid * 2 * F * Tc : Y + img * 2 * F * Tc;
        out_ring += img * 2 * ring;
        block_out += img * 2 * B;
    } else {
        if (rt_switched_off(rows, 4)) Y = X;
        Y += sid * 2 * F * Tc;
        out_ring += sid * 2 * ring;
        block_out += sid * 2 * B;
    }
    const float invN = 1.f / (float)N;
    const int s = s_lo + blockIdx.x * 256 + threadIdx.x;
    const bool live = s < ring;
    for (int n = threadIdx.x; n < N; n += 256) tb[n] = table[n];
    float va = 0.f, vb = 0.f;
    if (live && accumulate) {
        va = out_ring[s];
        vb = out_ring[ring + s];
    }
    for (int t = 0; t < Tc; ++t) {
        __syncthreads();
        for (int f = threadIdx.x; f < F; f += 256) {
            float2 a = Y[(long)f * Tc + t], b = Y[((long)F + f) * Tc + t];
            if (f == 0 || f == H) {          // numpy.fft.irfft ignores the imaginary part of DC and Nyquist
                a.y = 0.f;
                b.y = 0.f;
            }
            ya[f] = a;
            yb[f] = b;
        }
        __syncthreads();
        const int n = s - (start0 + t * start_step);
        if (live && n >= 0 && n < N) {
            const float sign = (n & 1) ? -1.f : 1.f;
            float sa = 0.f, sb = 0.f;
            int idx = n;                                   // f * n mod N for f = 1
            for (int f = 1; f < H; ++f) {
                const float2 c = tb[idx], a = ya[f], b = yb[f];
                sa = fmaf(a.x, c.x, fmaf(-a.y, c.y, sa));
                sb = fmaf(b.x, c.x, fmaf(-b.y, c.y, sb));
                idx += n;
                if (idx >= N) idx -= N;
            }
            const float w = window[n];
            const float fa = w * ((ya[0].x + sign * ya[H].x + 2.f * sa) * invN), fb = w * ((yb[0].x + sign * yb[H].x + 2.f * sb) * invN);
            va = accumulate ? va + fa : fa;
            vb = accumulate ? vb + fb : fb;
        }
    }
    if (!live) return;
    out_ring[s] = va;
    out_ring[ring + s] = vb;
    const int h0 = ring - (out_delay + 1) * B;           // utils.py:116 (out_delay = 2 there)
    if (accumulate && s >= h0 && s < h0 + B) {
        block_out[s - h0] = va;
        block_out[B + s - h0] = vb;
    }
}

// ---- rt_localize: one workgroup of 1024 threads per stream = Dq TDOAs x 1024/Dq frequency phases ---------------------------
// hist is a [D][Lh] float ring with write position hist_pos[0]; target[0] is updated for the NEXT block (:216-222).  In the bank layout
// a stream whose row word 5 is 0 fills its history and leaves its target index alone.
// GCC-NONLIN (gccPHATNLEnabled): a stream whose row word 6 holds alpha > 0 accumulates phi(term) = 1 - tanh(alpha sqrt(max(0, 1 - term)))
// instead of the term (angular_nl.h), NaN terms skipped as before; the ring, the window mean and the arg-max / peak rule do not change.
// MULTI: the window mean then goes through the offline peak rule (gcc.hip pick_peaks_kernel): strict local maxima, edges excluded, NaN
// never a peak; the `ntargets` largest, the larger index kept among equal heights, written in ascending order to words 8.. of the row.
// With fewer peaks than targets the indexes stay as they are.
template <bool MULTI>
__global__ __launch_bounds__(1024) void rt_localize_kernel(const float2* __restrict__ C, const float* __restrict__ cosT,
                                                           const float* __restrict__ sinT, int F, int D, int Dp, int Dq, int Tc,
                                                           float* __restrict__ hist, int Lh, int* __restrict__ hist_pos,
                                                           int loc_enabled, int loc_window, float* __restrict__ target,
                                                           float* __restrict__ gccphat_out, int bank, int ntargets, int nl_row) {
    __shared__ float s_sum[1024];
    __shared__ int s_cnt[1024];
    const long sid = blockIdx.z;
    C += sid * F * Tc;
    hist += sid * D * Lh;
    hist_pos += sid;
    target += sid * (MULTI ? RT_ROW_MULTI : RT_ROW);
    if (gccphat_out) gccphat_out += sid * D * Tc;
    if (bank && target[5] == 0.f) loc_enabled = 0;
    // word 6 of the stream's row: gccPHATNLAlpha, 0 = plain PHAT (a value that is not positive and finite is read as 0).  nl_row = 0: the
    // 4-word row of the single-stream call without frames_mode bit 24, which has no word 6.
    const float nl_alpha = nl_row ? target[6] : 0.f;
    const float nl_k2 = gccnmf_nl_alpha_ok(nl_alpha) ? gccnmf_nl_k2(nl_alpha) : 0.f;
    const int tau = threadIdx.x % Dq, g = threadIdx.x / Dq, G = 1024 / Dq;
    int pos = hist_pos[0];
    for (int t = 0; t < Tc; ++t) {
        float s = 0.f;
        int cnt = 0;
        if (nl_k2 != 0.f) {                               // workgroup-uniform: the PHAT loop below is the code it was
            if (tau < D)
                for (int f = g; f < F; f += G) {
                    const float2 c = C[(long)f * Tc + t];
                    const float v = c.x * cosT[(long)f * Dp + tau] + c.y * sinT[(long)f * Dp + tau];
                    if (v == v) {                         // a zero-magnitude bin (NaN coherence) is skipped, not counted
                        s += gccnmf_nl_half_phi(v, nl_k2);
                        ++cnt;
                    }
                }
            s *= 2.f;                                     // phi = 2 * half_phi: exact on the partial sum
        } else if (tau < D)
            for (int f = g; f < F; f += G) {
                const float2 c = C[(long)f * Tc + t];
                const float v = c.x * cosT[(long)f * Dp + tau] + c.y * sinT[(long)f * Dp + tau];
                if (v == v) {
                    s += v;
                    ++cnt;
                }
            }
        s_sum[threadIdx.x] = s;
        s_cnt[threadIdx.x] = cnt;
        __syncthreads();
        if (g == 0 && tau < D) {
            float st = 0.f;
            int ct = 0;
            for (int j = 0; j < G; ++j) {
                st += s_sum[j * Dq + tau];
                ct += s_cnt[j * Dq + tau];
            }
            const float m = ct ? st / (float)ct : NAN;                                    // numpy.nanmean over f (:214)
            hist[(long)tau * Lh + pos] = m;
            if (gccphat_out) gccphat_out[(long)tau * Tc + t] = m;
        }
        __syncthreads();
        pos = (pos + 1) % Lh;
    }
    if (loc_enabled) {
        if (g == 0) {
            float m = NAN;
            if (tau < D) {
                float s = 0.f;
                int cnt = 0;
                for (int j = 1; j <= loc_window; ++j) {                                   // the last L columns
                    const float v = hist[(long)tau * Lh + ((pos - j) % Lh + Lh) % Lh];
                    if (v == v) {
                        s += v;
                        ++cnt;
                    }
                }
                m = cnt ? s / (float)cnt : NAN;
            }
            s_sum[tau] = m;
        }
        __syncthreads();
        if constexpr (MULTI) {
            const int i = threadIdx.x;
            const float v = (i < D) ? s_sum[i] : NAN;
            const bool peak = i > 0 && i < D - 1 && v > s_sum[i - 1] && v > s_sum[i + 1];
            __syncthreads();
            s_sum[i] = peak ? v : NAN;                                                     // peak heights, NaN elsewhere
            const int npeaks = __syncthreads_count(peak);
            int rank = 0;                                                                  // peaks ranked above this one
            if (peak)
                for (int j = 0; j < D; ++j) {
                    const float o = s_sum[j];
                    rank += (o > v || (o == v && j > i)) ? 1 : 0;
                }
            const bool keep = peak && rank < ntargets;
            s_cnt[i] = keep ? 1 : 0;
            __syncthreads();
            if (keep && npeaks >= ntargets) {
                int slot = 0;
                for (int j = 0; j < i; ++j) slot += s_cnt[j];
                target[8 + slot] = (float)i;
            }
        } else
        // numpy.argmax: NaN counts as the maximum, first occurrence wins.  Tree reduction over (rank, index) pairs: a NaN ranks
        // above every number, equal ranks keep the smaller index (the serial scan this replaces cost ~6 us of the call).
        {
            const int i = threadIdx.x;
            float v = (i < D) ? s_sum[i] : -INFINITY;
            int idx = (i < D) ? i : 0x7fffffff;
            __syncthreads();
            for (int w = 512; w > 0; w >>= 1) {
                s_sum[i] = v;
                s_cnt[i] = idx;
                __syncthreads();
                if (i < w) {
                    const float ov = s_sum[i + w];
                    const int oi = s_cnt[i + w];
                    const bool vn = v != v, on = ov != ov;
                    const bool take = (on && !vn) || (on == vn && (on ? oi < idx : (ov > v || (ov == v && oi < idx))));
                    if (take) {
                        v = ov;
                        idx = oi;
                    }
                }
                __syncthreads();
            }
            if (i == 0) target[0] = (float)idx;
        }
    }
    if (threadIdx.x == 0) hist_pos[0] = pos;
}

// ---- per-frame coefficient inference (numHUpdates > 0): KL-NMF H updates with W fixed -------------------------------------------
// gccNMF/gccNMFFunctions.py:76 with W constant (sparsityAlpha = 0):  h <- h * (W^T (v / (W h))) / (W^T 1),  h0 = 1, per channel
// and frame, v = |X_c[:, t]|.  The reference's processor accepts numHUpdates and never uses it (gccNMFProcessor.py:168); with h = 1
// the mask below is exactly its tfMask (:267-269), so numHUpdates = 0 reproduces the reference and n > 0 is the low-latency
// notebook's "NMF coefficients are inferred frame-by-frame" (README.md:74).  Columns: col = 2 * t + c, ncol = 2 * Tc.
__global__ __launch_bounds__(256) void rt_fill_kernel(float* __restrict__ p, float v, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// r[f][col] = |X_c[f][t]| / sum_k W[f][k] h[k][col]; one wave per frequency row, grid = (ceil(F/4), 1, S)
// first != 0: h is still all ones (no fill pass: the first update reads no coefficients and WRITES them)
template <int ROW>
__global__ __launch_bounds__(256) void rt_wh_kernel(const float* __restrict__ W, const float* __restrict__ Hc, const float2* __restrict__ X,
                                                    float* __restrict__ Rv, int F, int K, int Kp, int Tc, int first,
                                                    const float* __restrict__ rows) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.x * 4 + wave;
    if (f >= F || rt_switched_off<ROW>(rows, 4)) return;
    const int ncol = 2 * Tc;
    const long sid = blockIdx.z;
    Hc += sid * Kp * ncol;
    X += sid * 2 * F * Tc;
    Rv += sid * F * ncol;
    const float* Wr = W + (long)f * Kp;
    for (int t = 0; t < Tc; ++t) {                         // both channels of a frame in one pass over the row of W
        float s0 = 0.f, s1 = 0.f;
        if (first) {
            for (int k = lane; k < K; k += 64) s0 = fmaf(Wr[k], 1.f, s0);
            s1 = s0;
        } else {
#pragma unroll 4
            for (int k = lane; k < K; k += 64) {
                const float w = Wr[k];
                const float2 h = *(const float2*)(Hc + (long)k * ncol + 2 * t);
                s0 = fmaf(w, h.x, s0);
                s1 = fmaf(w, h.y, s1);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s0 += __shfl_xor(s0, o);
            s1 += __shfl_xor(s1, o);
        }
        if (lane == 0) {
            const float2 xl = X[(long)f * Tc + t], xr = X[((long)F + f) * Tc + t];
            // W h = 0: the channel was silent in this frame (|X| = 0 in every bin), the first update left it no coefficients; 0, not 0 / 0
            *(float2*)(Rv + (long)f * ncol + 2 * t) =
                make_float2(s0 == 0.f ? 0.f : hypotf(xl.x, xl.y) / s0, s1 == 0.f ? 0.f : hypotf(xr.x, xr.y) / s1);
        }
    }
}

// h[k][col] *= (sum_f W[f][k] r[f][col]) / colsumW[k]; 16 atoms x 16 frequency phases per workgroup, grid = Kp/16 (the first version
// had 64 x 4: 16 workgroups with a 65-step chain of dependent loads, 17 us; now 64 workgroups, 17 independent loads per thread);
// grid = (Kp/16, 1, S)
template <int ROW>
__global__ __launch_bounds__(256) void rt_hupdate_kernel(const float* __restrict__ W, const float* __restrict__ Rv,
                                                         const float* __restrict__ colsumW, float* __restrict__ Hc, int F, int K, int Kp,
                                                         int Tc, int first, const float* __restrict__ rows) {
    __shared__ float red[4][16];
    if (rt_switched_off<ROW>(rows, 4)) return;            // the whole workgroup: before any barrier
    const int c = threadIdx.x & 15, q = threadIdx.x >> 4, wave = threadIdx.x >> 6;
    const int k = blockIdx.x * 16 + c;
    const int ncol = 2 * Tc;
    const long sid = blockIdx.z;
    Rv += sid * F * ncol;
    Hc += sid * Kp * ncol;
    for (int col = 0; col < ncol; ++col) {
        float s = 0.f;
#pragma unroll 4
        for (int f = q; f < F; f += 16) s = fmaf(W[(long)f * Kp + k], Rv[(long)f * ncol + col], s);
        s += __shfl_xor(s, 16);                            // the 4 frequency phases of this wave
        s += __shfl_xor(s, 32);
        if ((threadIdx.x & 63) < 16) red[wave][c] = s;
        __syncthreads();
        if (threadIdx.x < 16 && k < K) {
            const float num = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
            const float h = first ? 1.f : Hc[(long)k * ncol + col];
            Hc[(long)k * ncol + col] = h * (num / colsumW[k]);
        }
        __syncthreads();
    }
}

// per-channel mask with inferred coefficients: m_{i,c}[f][t] = sum_k W h_c M_i / sum_k W h_c;  Y_{i,c} = m_{i,c} X_c;  layouts and MAXT as
// rt_tfmask (single-target tfMask [2][F][Tc]); all nt targets in one pass over the row of W (and h); grid = (ceil(F/4), 1, S).
// No contraction in the body, and the two denominators are stated apart:
//   MAXT = 1: d = fmaf(w, h, d), the numerator fmaf(round(w * h), hm, n).  That is what the compiler's default contraction has always made
//   of `d += w * h` in this kernel -- the hot one of the streaming configuration with numHUpdates > 0 -- so the rounding is written down
//   here, where a compiler update cannot change the bits.
//   multi-target: d += round(w * h), as the numerators' fmaf(round(w * h), 1, .) add it, so nt = 1 gives 1.0 exactly.
template <int MAXT>
__global__ __launch_bounds__(256) void rt_tfmask_h_kernel(const float* __restrict__ W, const float* __restrict__ HMask,
                                                          const float* __restrict__ Hc, int F, int K, int Kp, int Tc,
                                                          const float2* __restrict__ X, float2* __restrict__ Y, float* __restrict__ tfMask,
                                                          const float* __restrict__ rows, int nt) {
#pragma clang fp contract(off)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
    if (f >= F || rt_switched_off<MAXT == 1 ? RT_ROW : RT_ROW_MULTI>(rows, 4)) return;
    if (MAXT == 1) nt = 1;
    const int ncol = 2 * Tc;
    const long sid = blockIdx.z;
    const long hplane = (long)Kp * Tc, yplane = 2L * F * Tc;
    HMask += sid * nt * hplane;
    Hc += sid * Kp * ncol;
    X += sid * yplane;
    Y += sid * nt * yplane;
    tfMask += sid * nt * yplane;
    const float* Wr = W + (long)f * Kp;
    for (int t = 0; t < Tc; ++t) {                         // both channels of a frame in one pass over the row of W
        float d0 = 0.f, d1 = 0.f, n0[MAXT], n1[MAXT];
#pragma unroll
        for (int i = 0; i < MAXT; ++i) n0[i] = n1[i] = 0.f;
#pragma unroll MAXT == 1 ? 4 : 1                           // as the two kernels this template replaces were built
        for (int k = lane; k < K; k += 64) {
            const float w = Wr[k];
            const float2 h = *(const float2*)(Hc + (long)k * ncol + 2 * t);
            const float wh0 = w * h.x, wh1 = w * h.y;
            if (MAXT == 1) {
                d0 = fmaf(w, h.x, d0);
                d1 = fmaf(w, h.y, d1);
            } else {
                d0 += wh0;
                d1 += wh1;
            }
#pragma unroll
            for (int i = 0; i < MAXT; ++i) {
                if (i < nt) {
                    const float hm = HMask[i * hplane + (long)k * Tc + t];
                    n0[i] = fmaf(wh0, hm, n0[i]);
                    n1[i] = fmaf(wh1, hm, n1[i]);
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            d0 += __shfl_xor(d0, o);
            d1 += __shfl_xor(d1, o);
        }
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
            if (i < nt) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    n0[i] += __shfl_xor(n0[i], o);
                    n1[i] += __shfl_xor(n1[i], o);
                }
            }
        }
        if (lane == 0) {
            const float2 a = X[(long)f * Tc + t], b = X[((long)F + f) * Tc + t];
#pragma unroll
            for (int i = 0; i < MAXT; ++i) {
                if (i < nt) {
                    // no coefficients (a silent channel): mask 0, Y = 0
                    const float m0 = d0 == 0.f ? 0.f : n0[i] / d0, m1 = d1 == 0.f ? 0.f : n1[i] / d1;
                    tfMask[i * yplane + (long)f * Tc + t] = m0;
                    tfMask[i * yplane + ((long)F + f) * Tc + t] = m1;
                    Y[i * yplane + (long)f * Tc + t] = make_float2(m0 * a.x, m0 * a.y);
                    Y[i * yplane + ((long)F + f) * Tc + t] = make_float2(m1 * b.x, m1 * b.y);
                }
            }
        }
    }
}

// The instantiation of a kernel template that goes with the call's layout: (single-target, multi-target) template arguments, picked by the
// entry point's `multi`.  Every launch of a templated kernel below goes through it.
#define RT_KERNEL(kernel, single, multiple) (multi ? kernel<multiple> : kernel<single>)

extern "C" {

// Every buffer is passed explicitly (allocation lives with the host, gcc_nmf_amd/realtime.py).
//   frames_mode = 0: streaming.  block_in [2][B] -> 8-block input buffer -> Tc windows -> ... -> overlap-add -> block_out [2][B]
//   frames_mode = 1: the reference's GCCNMFProcessor.processFrames on its own: in_ring = windowed-sample frames [2][Tc][N]
//                    in, out_ring = processed frames [2][Tc][N] out, no shift / overlap-add (block_in, block_out unused).
//   bit 3 + bits 8..19 = S - 1: a bank of S streams in one set of launches (the layout is documented in include/gccnmf_hip.h).
//   bit 20 + bits 21..23 = N - 1: multi-target layout (target_mode 1): N one-hot masks, N outputs, N tracked peaks per stream.
int gccnmf_rt_process_block_ll(const float* block_in, float* block_out, float* in_ring, float* out_ring, float* X, float* Y, float* C,
                               float* HMask, int* argmaxTDOA, float* tfMask, float* hist, int* hist_pos, float* target,
                               float* gccphat, const float* W, const float* cosT, const float* sinT, const float* window,
                               const float* synthesis_window, const float* twiddle, const float* colsumW, float* Hcoef, float* Rv,
                               int windowSize, int hopSize, int blockSize, int K, int Kp, int D, int Dp, int numTDOAHistory,
                               int target_mode, int separation_enabled, int localization_enabled, int localization_window,
                               int frames_mode_bits, int numHUpdates, int out_delay_blocks, void* stream) {
    GCCNMF_ENTER();
    // frames_mode_bits: 1 = frames mode (above); 2 = leave the localisation kernel out of this call; 4 = ONLY the localisation kernel
    // (2 then 4 = the same work in two calls, so that a host can fetch block_out before the tracking update has run); 8 = bank layout
    // of S = bits 8..19 + 1 streams (streaming only); 1 << 20 = multi-target layout of NT = bits 21..23 + 1 targets (target_mode 1 only);
    // 1 << 24 = 8-word single-stream target row (below); any bit above 24, S bits without the bank layout, or target bits without the
    // multi-target layout is an error
    const int frames_mode = frames_mode_bits & 1;
    const bool skip_localize = frames_mode_bits & 2, only_localize = frames_mode_bits & 4;
    const int bank = (frames_mode_bits >> 3) & 1;
    const int S = ((frames_mode_bits >> 8) & 0xfff) + 1;
    const bool multi = (frames_mode_bits >> 20) & 1;
    const int NT = ((frames_mode_bits >> 21) & 7) + 1;
    // 1 << 24: the single-stream target row has 8 words and word 6 is gccPHATNLAlpha (GCC-NONLIN localisation); the bank and multi-target
    // rows always have that word, so the bit is an error there
    const bool row8 = (frames_mode_bits >> 24) & 1;
    if ((frames_mode_bits & ~0x1ffffff) || (bank && frames_mode) || (!bank && S > 1) || (row8 && (bank || multi))) return GCCNMF_ERR_ARG;
    const int nl_row = (bank || multi || row8) ? 1 : 0;
    // separation_enabled bit 1: the online spatial filter behind the mask kernel.  Its switch is word 7 of the stream's target row, which
    // the 4-word single-stream row does not have; its state is read and written as float4 behind the history images of hist.
    const bool spatial = (separation_enabled & GCCNMF_RT_SEPARATION_SPATIAL) != 0;
    if (spatial && (!nl_row || ((size_t)hist & 15))) return GCCNMF_ERR_ARG;
    if ((multi && target_mode != 1) || (!multi && NT > 1)) return GCCNMF_ERR_ARG;
    const float* rows = bank ? target : nullptr;          // the per-stream switches the mask and synthesis kernels read
    // powers of two from 64 up: the radix-2 LDS transform (twiddle = N/2 values of exp(-2 pi j k / N)); every other even size: the direct
    // sums above (twiddle = the N-entry table (cos, sin)(2 pi k / N))
    const bool pow2 = windowSize >= 64 && (windowSize & (windowSize - 1)) == 0;
    const int logN = pow2 ? ilog2_exact(windowSize) : 0;
    if (!in_ring || !out_ring || !X || !Y || !C || !HMask || !tfMask || !hist || !hist_pos || !target || !W || !cosT || !sinT ||
        !window || !synthesis_window || !twiddle || (!frames_mode && (!block_in || !block_out)))
        return GCCNMF_ERR_ARG;
    if (numHUpdates < 0 || (numHUpdates > 0 && (!colsumW || !Hcoef || !Rv)) || out_delay_blocks < 1 || out_delay_blocks > 7) return GCCNMF_ERR_ARG;
    if (windowSize < 4 || windowSize > 4096 || (windowSize & 1) || hopSize < 1 || blockSize < hopSize || blockSize % hopSize || K < 1 || Kp % 64 || Kp < K || D < 1 ||
        D > 1024 || Dp % 32 || Dp < D || numTDOAHistory < 1 || localization_window < 1 || localization_window > numTDOAHistory)
        return GCCNMF_ERR_ARG;
    const int Tc = blockSize / hopSize, F = windowSize / 2 + 1;
    const int ring = frames_mode ? Tc * windowSize : 8 * blockSize;
    if (!frames_mode && ring < windowSize + (Tc - 1) * hopSize) return GCCNMF_ERR_UNSUPPORTED;      // the 8-block buffer must hold one block's windows
    const int start0 = frames_mode ? 0 : ring - windowSize - (Tc - 1) * hopSize;
    const int start_step = frames_mode ? windowSize : hopSize;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = sizeof(float2) * (windowSize + windowSize / 2);
    int Dq = 64;
    while (Dq < D) Dq *= 2;                 // power of two so that 1024 % Dq == 0
    // NT = 1 and grid y = 1 outside the multi-target layout (checked above), nl_row = 1 inside it: one argument list serves both layouts
    auto localize = [&]() {
        hipLaunchKernelGGL(RT_KERNEL(rt_localize_kernel, false, true), dim3(1, 1, S), dim3(1024), 0, s, (const float2*)C, cosT, sinT, F, D, Dp,
                           Dq, Tc, hist, numTDOAHistory, hist_pos, localization_enabled, localization_window, target, gccphat, bank, NT, nl_row);
    };
    if (only_localize) {
        localize();
        GCCNMF_CHECK_LAUNCH();
        return GCCNMF_OK;
    }
    if (!frames_mode) {
        hipLaunchKernelGGL(RT_KERNEL(rt_shift_kernel, false, true), dim3(1, NT, S), dim3(1024), 0, s, in_ring, out_ring, block_in, blockSize,
                           ring);
        GCCNMF_CHECK_LAUNCH();
    }
    const size_t lds_dft = sizeof(float2) * (2 * windowSize + 2);
    if (!pow2 && lds_dft + 4096 > 64 * 1024) {
        // windows above ~3800 samples: the table + frame image (+ the analysis kernel's 4 KB of static LDS) pass the 64 KB a launch gets by default
        if (hipFuncSetAttribute((const void*)rt_frames_dft_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_dft) != hipSuccess ||
            hipFuncSetAttribute((const void*)RT_KERNEL(rt_synth_dft_kernel, false, true), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_dft) != hipSuccess)
            return GCCNMF_ERR_LAUNCH;
    }
    if (pow2) {
        hipLaunchKernelGGL(rt_frames_kernel, dim3(Tc, 1, S), dim3(FFT_NT), lds, s, in_ring, ring, windowSize, logN, start0, start_step, Tc,
                           window, (const float2*)twiddle, (float2*)X, (float2*)C);
    } else {
        hipLaunchKernelGGL(rt_frames_dft_kernel, dim3(gccnmf_ceil_div(F, 64), Tc, S), dim3(256), lds_dft, s, in_ring, ring, windowSize, start0,
                           start_step, Tc, window, (const float2*)twiddle, (float2*)X, (float2*)C);
    }
    GCCNMF_CHECK_LAUNCH();
    if (separation_enabled) {
        hipLaunchKernelGGL(RT_KERNEL(rt_gccnmf_kernel, false, true), dim3(Kp / 32, Tc, S), dim3(64 * RT_G_WAVES), 0, s, (const float2*)C, cosT,
                           sinT, W, F, K, Kp, D, Dp, Tc, target, target_mode, bank, HMask, argmaxTDOA, NT);
        GCCNMF_CHECK_LAUNCH();
        if (numHUpdates == 0) {
            hipLaunchKernelGGL(RT_KERNEL(rt_tfmask_kernel, 1, RT_MAX_TARGETS), dim3(gccnmf_ceil_div(F, 4), 1, S), dim3(256), 0, s, W, HMask, F, K,
                               Kp, Tc, (const float2*)X, (float2*)Y, tfMask, rows, NT);
            GCCNMF_CHECK_LAUNCH();
        } else {
            // the coefficient updates do not depend on the targets: the same kernels, reading the switches at the layout's row stride
            for (int it = 0; it < numHUpdates; ++it) {      // h0 = 1 is implicit in the first update (no fill pass)
                hipLaunchKernelGGL(RT_KERNEL(rt_wh_kernel, RT_ROW, RT_ROW_MULTI), dim3(gccnmf_ceil_div(F, 4), 1, S), dim3(256), 0, s, W, Hcoef,
                                   (const float2*)X, Rv, F, K, Kp, Tc, it == 0 ? 1 : 0, rows);
                GCCNMF_CHECK_LAUNCH();
                hipLaunchKernelGGL(RT_KERNEL(rt_hupdate_kernel, RT_ROW, RT_ROW_MULTI), dim3(Kp / 16, 1, S), dim3(256), 0, s, W, Rv, colsumW,
                                   Hcoef, F, K, Kp, Tc, it == 0 ? 1 : 0, rows);
                GCCNMF_CHECK_LAUNCH();
            }
            hipLaunchKernelGGL(RT_KERNEL(rt_tfmask_h_kernel, 1, RT_MAX_TARGETS), dim3(gccnmf_ceil_div(F, 4), 1, S), dim3(256), 0, s, W, HMask,
                               Hcoef, F, K, Kp, Tc, (const float2*)X, (float2*)Y, tfMask, rows, NT);
            GCCNMF_CHECK_LAUNCH();
        }
        if (spatial) {
            const int rc = gccnmf_launch_rt_spatial(X, Y, target, multi ? RT_ROW_MULTI : RT_ROW, bank,
                                                    hist + gccnmf_rt_spatial_state_offset(S, D, numTDOAHistory), F, Tc, multi, NT, S, s);
            if (rc != GCCNMF_OK) return rc;
        }
    }
    if (pow2) {
        hipLaunchKernelGGL(RT_KERNEL(rt_synth_kernel, false, true), dim3(1, NT, S), dim3(FFT_NT), lds, s,
                           (const float2*)(separation_enabled ? Y : X), windowSize, logN,
                           start0, start_step, frames_mode ? 0 : 1, Tc, ring, blockSize, out_delay_blocks, synthesis_window,
                           (const float2*)twiddle, out_ring, block_out, (const float2*)X, rows);
    } else {
        // positions that receive a frame this call, plus the block handed out (it may lie in front of them)
        const int h0 = ring - (out_delay_blocks + 1) * blockSize;
        const int s_lo = frames_mode ? 0 : (start0 < h0 ? start0 : (h0 > 0 ? h0 : 0));
        hipLaunchKernelGGL(RT_KERNEL(rt_synth_dft_kernel, false, true), dim3(gccnmf_ceil_div(ring - s_lo, 256), NT, S), dim3(256), lds_dft, s,
                           (const float2*)(separation_enabled ? Y : X), windowSize, start0, start_step, frames_mode ? 0 : 1, Tc, ring, blockSize,
                           out_delay_blocks, s_lo, synthesis_window, (const float2*)twiddle, out_ring, block_out, (const float2*)X, rows);
    }
    GCCNMF_CHECK_LAUNCH();
    if (skip_localize) return GCCNMF_OK;
    localize();
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

// The reference's processor as it is: one window for analysis and synthesis (:186-187), no coefficient inference (numHUpdates is
// accepted and unused there, :168), the block two blocks old handed out (utils.py:116).
int gccnmf_rt_process_block(const float* block_in, float* block_out, float* in_ring, float* out_ring, float* X, float* Y, float* C,
                            float* HMask, int* argmaxTDOA, float* tfMask, float* hist, int* hist_pos, float* target,
                            float* gccphat, const float* W, const float* cosT, const float* sinT, const float* window,
                            const float* twiddle, int windowSize, int hopSize, int blockSize, int K, int Kp, int D, int Dp,
                            int numTDOAHistory, int target_mode, int separation_enabled, int localization_enabled,
                            int localization_window, int frames_mode, void* stream) {
    GCCNMF_ENTER();
    return gccnmf_rt_process_block_ll(block_in, block_out, in_ring, out_ring, X, Y, C, HMask, argmaxTDOA, tfMask, hist, hist_pos, target,
                                      gccphat, W, cosT, sinT, window, window, twiddle, nullptr, nullptr, nullptr, windowSize, hopSize,
                                      blockSize, K, Kp, D, Dp, numTDOAHistory, target_mode, separation_enabled, localization_enabled,
                                      localization_window, frames_mode, 0, 2, stream);
}

}  // extern "C"
