// Offline speech enhancement: the TDOA of every atom of every frame over the WHOLE grid, and the talker / noise coefficient masks
// around a target direction.  Reference: gccNMF/realtime/gccNMFProcessor.py:254,:259-265 (the streaming form is rt_gccnmf_kernel,
// rt.hip: one frame per workgroup, the tables reloaded for every frame); DESIGN.md section 4e.
//
//   score[k, d, t] = sum_f W[f, k] (Cr[f, t] cos[f, d] + Ci[f, t] sin[f, d]),   atom_tdoa[k, t] = argmax_{d < D} score[k, d, t]
//
// A (K, D, T) score array would be 650 MB per 10 s file at K = 1024, D = 128: nothing of it is stored.  A wave holds a
// 64 TDOA x 64 atom x 2 frame block of scores in MFMA accumulators (32x32x2 f32, exact), scans it for the running (best value, best
// index) of its lanes' atoms and moves on to the next 64 TDOAs; the only traffic to HBM is the 2-byte index (and, if asked for, the
// 4-byte winning score) per (atom, frame).  No LDS, no workspace, no hand-over between workgroups.
#include "atom_tdoa.h"

typedef float at_f32x16 __attribute__((ext_vector_type(16)));

#define AT_WAVES 4                                         // waves of a workgroup: consecutive frame pairs, nothing shared but the caches
#define AT_CHUNK 8                                         // f steps (two bins each) whose loads are in flight together

// rows (r&3) + 8*(r>>2) + 4*hh of the tile, ascending within a lane; first index wins an exact tie, NaN never wins
__device__ __forceinline__ void at_scan(const at_f32x16& acc, int row0, int D, float& bv, int& bi) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float v = acc[r];
        const int row = row0 + (r & 3) + 8 * (r >> 2);
        if (row < D && (v > bv || (v == bv && row < bi))) {
            bv = v;
            bi = row;
        }
    }
}

// grid = (Kp/64, Tp/8, batch), 256 threads.  Workgroup = 64 atoms x 8 frames of one file; wave w = frames t0, t0 + 1 with
// t0 = 8*blockIdx.y + 2*w.  MFMA 32x32x2: A[i = d][k = f] = Cr cos + Ci sin built on the VALU from one (cos, sin) fetch per TDOA tile
// (it serves both frames and both atom tiles: 2 VALU operations per operand element, one operand per two MFMAs), B[k = f][j = atom] =
// W[f][atom] (one fetch serves both frames and both TDOA tiles).  Per f step: 8 loads, 8 VALU operations, 8 MFMAs into 8 independent
// accumulators (128 registers); the loads of AT_CHUNK steps are issued before the first use (80 registers).  The f sum of one
// (k, d, t) is ONE accumulator chain in ascending f -- the MFMA is a k-ordered fmaf chain -- whatever the grid, the batch or the
// file's place in it.
__global__ __launch_bounds__(64 * AT_WAVES, 2) void atom_tdoa_kernel(const float* __restrict__ CC, const float* __restrict__ trig,
                                                                     const float* __restrict__ W, int F, int Fp, int T, int Tp, int K,
                                                                     int Kp, int D, int Dp, unsigned short* __restrict__ atom_tdoa,
                                                                     float* __restrict__ atom_score) {
#pragma clang fp contract(off)
    const int b = blockIdx.z, k0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hh = lane >> 5;
    const int t0 = (blockIdx.y * AT_WAVES + wave) * 2;                       // even, < Tp
    float bv[2][2];                                                          // [frame][atom tile]
    int bi[2][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        bv[q >> 1][q & 1] = -INFINITY;
        bi[q >> 1][q & 1] = 0;
    }
    if (t0 < T) {                                                            // wave-uniform; there is no barrier in this kernel
        const long plane = (long)Fp * Tp;
        const float* Cr = CC + (long)b * 2 * plane + t0;
        const float* Ci = Cr + plane;
        const float* Wb = W + (long)b * Fp * Kp + k0 + l31;
        const float* cosT = trig + l31;
        const float* sinT = trig + (long)Fp * Dp + l31;
        const int steps = (F + 1) / 2;
        const bool two_k = k0 + 32 < K;                                      // the second atom tile holds an atom
        for (int d0 = 0; d0 < D; d0 += 64) {
            const bool two_d = d0 + 32 < D;                                  // the second TDOA tile holds a TDOA
            at_f32x16 acc[2][2][2];                                          // [frame][TDOA tile][atom tile]
#pragma unroll
            for (int q = 0; q < 8; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[q >> 2][(q >> 1) & 1][q & 1][r] = 0.f;
            for (int p0 = 0; p0 < steps; p0 += AT_CHUNK) {
                // raw loads first, all of them (rt.hip, rt_gccnmf_kernel: the scheduler otherwise sinks each next to its use)
                float c0[AT_CHUNK], s0[AT_CHUNK], c1[AT_CHUNK], s1[AT_CHUNK], w0[AT_CHUNK], w1[AT_CHUNK];
                float2 cr[AT_CHUNK], ci[AT_CHUNK];
#pragma unroll
                for (int u = 0; u < AT_CHUNK; ++u) {                         // (clamped row, masked below)
                    const int f = min(2 * (p0 + u) + hh, F - 1);
                    c0[u] = cosT[f * Dp + d0];
                    s0[u] = sinT[f * Dp + d0];
                    c1[u] = cosT[f * Dp + d0 + 32];
                    s1[u] = sinT[f * Dp + d0 + 32];
                    w0[u] = Wb[f * Kp];
                    w1[u] = Wb[f * Kp + 32];
                    cr[u] = *(const float2*)(Cr + (long)f * Tp);
                    ci[u] = *(const float2*)(Ci + (long)f * Tp);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < AT_CHUNK; ++u) {
                    const bool ok = 2 * (p0 + u) + hh < F;
                    const float b0 = ok ? w0[u] : 0.f, b1 = ok ? w1[u] : 0.f;
                    const float a00 = ok ? fmaf(cr[u].x, c0[u], ci[u].x * s0[u]) : 0.f;      // frame 0, TDOA tile 0
                    const float a01 = ok ? fmaf(cr[u].x, c1[u], ci[u].x * s1[u]) : 0.f;
                    const float a10 = ok ? fmaf(cr[u].y, c0[u], ci[u].y * s0[u]) : 0.f;      // frame 1
                    const float a11 = ok ? fmaf(cr[u].y, c1[u], ci[u].y * s1[u]) : 0.f;
                    acc[0][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a00, b0, acc[0][0][0], 0, 0, 0);
                    acc[1][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a10, b0, acc[1][0][0], 0, 0, 0);
                    if (two_k) {
                        acc[0][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a00, b1, acc[0][0][1], 0, 0, 0);
                        acc[1][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a10, b1, acc[1][0][1], 0, 0, 0);
                    }
                    if (two_d) {
                        acc[0][1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a01, b0, acc[0][1][0], 0, 0, 0);
                        acc[1][1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a11, b0, acc[1][1][0], 0, 0, 0);
                        if (two_k) {
                            acc[0][1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a01, b1, acc[0][1][1], 0, 0, 0);
                            acc[1][1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a11, b1, acc[1][1][1], 0, 0, 0);
                        }
                    }
                }
            }
            // TDOA tiles in ascending order; rows >= D (and the tiles skipped above, all zero) never win
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int fr = q >> 2, dt = (q >> 1) & 1, kt = q & 1;
                at_scan(acc[fr][dt][kt], d0 + 32 * dt + 4 * hh, (dt && !two_d) ? 0 : D, bv[fr][kt], bi[fr][kt]);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {                                        // the other half of the rows: both halves end up equal
            float& v = bv[q >> 1][q & 1];
            int& i = bi[q >> 1][q & 1];
            const float ov = __shfl_xor(v, 32);
            const int oi = __shfl_xor(i, 32);
            if (ov > v || (ov == v && oi < i)) {
                v = ov;
                i = oi;
            }
        }
    }
    // lane l stores atom k0 + l: lanes 32.. hold the second atom tile.  Every position of the padded image is written: atoms >= K,
    // frames >= T and columns whose scores are all NaN (numpy.argmax of an all-NaN column) hold index 0
    const int atom = k0 + lane;
    const float v0 = hh ? bv[0][1] : bv[0][0], v1 = hh ? bv[1][1] : bv[1][0];
    const int i0 = hh ? bi[0][1] : bi[0][0], i1 = hh ? bi[1][1] : bi[1][0];
    const bool live0 = atom < K && t0 < T, live1 = atom < K && t0 + 1 < T;
    const unsigned o0 = (live0 && v0 > -INFINITY) ? (unsigned)i0 : 0u, o1 = (live1 && v1 > -INFINITY) ? (unsigned)i1 : 0u;
    const long at = ((long)b * Kp + atom) * Tp + t0;
    *(unsigned*)(atom_tdoa + at) = o0 | (o1 << 16);
    if (atom_score)                                                          // the winning score; NaN where no score was a number
        *(float2*)(atom_score + at) = make_float2(live0 ? (v0 > -INFINITY ? v0 : NAN) : 0.f, live1 ? (v1 > -INFINITY ? v1 : NAN) : 0.f);
}

// Talker / noise masks from the index image (gccNMFProcessor.py:263 boxcar, :265 window function -- unclamped, as rt_gccnmf_kernel
// computes it).  One thread per (atom, frame) of the padded image; padded positions hold 0 in every output.
// grid = (ceil(Tp/256), Kp, batch)
__global__ __launch_bounds__(256) void enhancement_masks_kernel(const unsigned short* __restrict__ atom_tdoa, const int* __restrict__ target,
                                                                int per_frame, int window, float eps, float beta, float nf, int T, int Tp,
                                                                int K, int Kp, unsigned char* __restrict__ image, float* __restrict__ masks) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y, b = blockIdx.z;
    if (t >= Tp) return;
    const long at = ((long)b * Kp + k) * Tp + t;
    float m = 0.f, n = 0.f;
    unsigned char noise = 0;
    if (k < K && t < T) {
        const int i = atom_tdoa[at];
        const int tg = per_frame ? target[(long)b * Tp + t] : target[b];
        const float dist = fabsf((float)i - (float)tg);
        const bool talker = dist < eps;                                       // TARGET_MODE_BOXCAR (:263)
        if (window)
            m = expf(-powf(dist / eps, beta)) / (1.f + nf) + nf;              // TARGET_MODE_WINDOW_FUNCTION (:265)
        else
            m = talker ? 1.f : 0.f;
        n = 1.f - m;
        noise = talker ? 0 : 1;
    }
    if (image) image[at] = noise;
    if (masks) {
        masks[((long)b * 2 * Kp + k) * Tp + t] = m;
        masks[(((long)b * 2 + 1) * Kp + k) * Tp + t] = n;
    }
}

int gccnmf_launch_atom_tdoa(const float* CC, const float* trig, const float* W, int F, int T, int K, int D, int batch,
                            unsigned short* atom_tdoa, float* atom_score, hipStream_t s) {
    const GccNmfPitches p = gccnmf_make_pitches(F, T, K);
    hipLaunchKernelGGL(atom_tdoa_kernel, dim3(p.Kp / 64, p.Tp / (2 * AT_WAVES), batch), dim3(64 * AT_WAVES), 0, s, CC, trig, W, F, p.Fp,
                       T, p.Tp, K, p.Kp, D, gccnmf_round_up(D, 64), atom_tdoa, atom_score);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}

int gccnmf_launch_enhancement_masks(const unsigned short* atom_tdoa, const int* target, int per_frame, int window, float eps,
                                    float beta, float noise_floor, int T, int K, int batch, unsigned char* image, float* masks,
                                    hipStream_t s) {
    const GccNmfPitches p = gccnmf_make_pitches(2, T, K);
    hipLaunchKernelGGL(enhancement_masks_kernel, dim3(gccnmf_ceil_div(p.Tp, 256), p.Kp, batch), dim3(256), 0, s, atom_tdoa, target,
                       per_frame, window, eps, beta, noise_floor, T, p.Tp, K, p.Kp, image, masks);
    GCCNMF_CHECK_LAUNCH();
    return GCCNMF_OK;
}
