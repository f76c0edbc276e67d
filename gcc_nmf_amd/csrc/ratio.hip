// Ratio-mask (Wiener-like) reconstruction of the separation library: the stereo caller of ratio_kernel.h (the kernel, its tile and its
// arithmetic are described there).  Two channels, H of pitch Np = round_up(2 T, 64), output plane i*2 + c of 2 S planes per file.
#include "ratio.h"
#include "ratio_kernel.h"

int gccnmf_launch_ratio(const float* W, const float* H, const unsigned char* argmax, const float* masks, const float* X, int F, int T,
                        int K, int S, int batch, float* spec, hipStream_t s) {
    if (S < 1 || S > GCCNMF_RATIO_MAX_TARGETS) return GCCNMF_ERR_UNSUPPORTED;
    if (2L * batch > 65535) return GCCNMF_ERR_UNSUPPORTED;     // grid.z
    GccNmfPitches p = gccnmf_make_pitches(F, T, K);
    RatioArgs a;
    a.W = W; a.H = H; a.argmax = argmax; a.masks = masks; a.X = (const float2*)X; a.spec = (float2*)spec;
    a.M = 2; a.nsig_pitch = 2 * S;
    a.F = F; a.Fp = p.Fp; a.T = T; a.Tp = p.Tp; a.Np = p.Np; a.K = K; a.Kp = p.Kp;
    return ratio_launch(a, S, batch, s);
}
