// libgccnmf_array.so: the two stages of M-channel (microphone-array) GCC-NMF that the stereo kernels cannot serve (include/gccnmf_array.h,
// DESIGN section 4j).  A library of its own: it links nothing from the separation library.  It shares three headers with it -- the status
// codes of common.h, the coherence arithmetic of phat.h and the ratio-mask kernel of ratio_kernel.h, of which it compiles its own
// instantiations -- and includes no GEMM header.
//
//   gccnmf_array_features     V = the magnitudes of all M channels side by side, CC = the PHAT coherence of all P = M (M - 1) / 2
//                             microphone pairs STACKED along the bin axis (pair p owns rows p Fp .. p Fp + F - 1): the hypotf of
//                             gcc_magnitude_kernel (gcc.hip) and phat_coherence (phat.h) per element, every padding element written as 0
//   gccnmf_array_reconstruct  the ratio-mask reconstruction for M channels: ratio_kernel.h with the caller's M and nsig_pitch and
//                             Np = round_up(M T, 64)
#include "common.h"
#include "phat.h"
#include "ratio_kernel.h"
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

// Row p*Fp + f of CC = X_a conj(X_b) / |X_a| / |X_b| of pair p = (a, b): phat_coherence with xl = X_a, xr = X_b,
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
        phat_coherence(xl, xr, re, im);
    }
    float* Cb = CC + (long)b * 2 * P * plane + (long)row * Tp + t;
    Cb[0] = re;
    Cb[(long)P * plane] = im;
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
    RatioArgs a;
    a.W = W; a.H = H; a.argmax = argmax; a.masks = masks; a.X = (const float2*)X; a.spec = (float2*)spec;
    a.M = M; a.nsig_pitch = nsig_pitch;
    a.F = F; a.Fp = gccnmf_round_up(F, 16); a.T = T; a.Tp = gccnmf_round_up(T, 64); a.Np = gccnmf_round_up(M * T, 64);
    a.K = K; a.Kp = gccnmf_round_up(K, 64);
    return ratio_launch(a, S, batch, (hipStream_t)stream);
}

}  // extern "C"
