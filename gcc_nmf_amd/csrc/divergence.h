// Generalised KL divergence of the current factors, D(V || W.H) per file: stage 7 of gccnmf_klnmf_stage (divergence.hip).
#pragma once
#include "common.h"

// One term of D = sum V log(V / R) - V + R, from V and R = (W.H)[f][n], evaluated in float32 without the cancellation of the textbook
// form near V = R.  With x = (V - R) / R the term is R * g(x), g(x) = (1 + x) log1p(x) - x = x^2/2 - x^3/6 + x^4/12 - ...:
//   |x| < 1/8   the alternating series sum_{n=2..9} (-1)^n x^n / (n (n - 1)) (Horner); the first dropped term is x^10 / 90, below
//               2^-24 of the sum -- nothing is subtracted, so a term of size R x^2 / 2 keeps its full relative precision
//   otherwise   (1 + x) log1p(x) - x directly: g >= 0.007 there and the two parts are of size |x|, a few bits at the worst
// V = 0 contributes R alone (the limit: no logarithm, no 0 / 0).  0 < V < R * 2^-24 or so (a silent bin under the random initial factors):
// V - R rounds to -R, x to -1 exactly, and (1 + x) log1p(x) would be 0 * -inf = NaN; the term is then R + V (log(V / R) - 1) -- R alone once
// V / R is below the smallest normal number (the rest is below 2^-119 of R).  NaN in V or R propagates.  V > 0 with R == 0 (an underflowed
// product; not reachable from positive factors) gives fma(inf, inf, -inf) = NaN where float64 arithmetic gives +inf: non-finite either
// way, and a non-finite D stops nothing.
__device__ __forceinline__ float gccnmf_kl_term(float v, float r) {
    if (v == 0.f) return r;
    const float x = (v - r) / r;
    if (x <= -1.f) {
        const float q = v / r;
        return q >= 1.17549435e-38f ? fmaf(v, logf(q) - 1.f, r) : r;
    }
    float g;
    if (fabsf(x) < 0.125f) {
        float p = -1.f / 72.f;
        p = fmaf(p, x, 1.f / 56.f);
        p = fmaf(p, x, -1.f / 42.f);
        p = fmaf(p, x, 1.f / 30.f);
        p = fmaf(p, x, -1.f / 20.f);
        p = fmaf(p, x, 1.f / 12.f);
        p = fmaf(p, x, -1.f / 6.f);
        p = fmaf(p, x, 0.5f);
        g = (x * x) * p;
    } else {
        g = fmaf(1.f + x, log1pf(x), -x);
    }
    return r * g;
}

// One term of the Itakura-Saito divergence D = sum V / R - log(V / R) - 1 over the elements with V > 0: with x = (V - R) / R the term is
// x - log1p(x) = x^2/2 - x^3/3 + x^4/4 - ..., in float32 without the cancellation of the textbook form near V = R.
//   |x| < 1/8   x^2 * sum_{n=2..9} (-x)^(n-2) / n (Horner); the first dropped term is x^10 / 10, below 2^-24 of the sum
//   otherwise   x - log1p(x) directly: the term is >= 0.007 there and the two parts are of size |x|
// V = 0 contributes NOTHING: IS is +infinity there (a silent bin has no finite IS fit), so the sum is the divergence over the support of V.
// x < -1/2 (V below half of R): 1 + x = V / R is small and x carries an ABSOLUTE rounding error of 2^-24, so log1p(x) would lose log2(R / V)
// bits (and be -inf once x rounds to -1); the term is (q - 1) - log(q) with the quotient q = V / R itself there -- both parts are of one sign
// apart from q, and the sum is >= 0.19 -- and log(R) - log(V) - 1 once q is below the smallest normal number.  NaN in V or R propagates;
// R == 0 with V > 0 gives inf - inf = NaN (non-finite either way).
__device__ __forceinline__ float gccnmf_is_term(float v, float r) {
    if (v == 0.f) return 0.f;
    const float x = (v - r) / r;
    if (x < -0.5f) {
        const float q = v / r;
        return q >= 1.17549435e-38f ? (q - 1.f) - logf(q) : (logf(r) - logf(v)) - 1.f;
    }
    if (fabsf(x) < 0.125f) {
        float p = -1.f / 9.f;
        p = fmaf(p, x, 1.f / 8.f);
        p = fmaf(p, x, -1.f / 7.f);
        p = fmaf(p, x, 1.f / 6.f);
        p = fmaf(p, x, -1.f / 5.f);
        p = fmaf(p, x, 1.f / 4.f);
        p = fmaf(p, x, -1.f / 3.f);
        p = fmaf(p, x, 0.5f);
        return (x * x) * p;
    }
    return x - log1pf(x);
}

// One term of the Euclidean distance D = sum 1/2 (V - R)^2: the difference (exact where V and R are within a factor of two), its square, the half.
__device__ __forceinline__ float gccnmf_euclidean_term(float v, float r) {
    const float d = v - r;
    return 0.5f * (d * d);
}

// out[b] = D(V_b || W_b . H_b) for b < batch, float64; divergence: 0 KL (the default), 1 Itakura-Saito, 2 Euclidean.  V [batch][Fp][Np], H [batch][Kp][Np], W [batch][Fp][Kp] (sW = Fp * Kp) or one
// shared dictionary (sW = 0).  partials: scratch, gccnmf_kl_divergence_tiles(F, N) doubles per file, s_partials doubles apart.
// Reads only f < F, n < N, k < K of the operands' valid extent (padding may hold anything); writes partials and out only.
int gccnmf_kl_divergence_tiles(int F, int N);
int gccnmf_kl_divergence_launch(const float* V, const float* W, long sW, const float* H, int F, int N, int K, int Fp, int Kp, int Np,
                                int batch, double* partials, long s_partials, double* out, hipStream_t stream, int divergence = 0);
