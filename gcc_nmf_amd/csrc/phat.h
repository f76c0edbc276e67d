// The PHAT coherence of one (bin, frame) of a microphone pair: xl conj(xr) / |xl| / |xr|.  The definition for gcc_coherence_kernel
// (gcc.hip) and array_coherence_kernel (array.hip); the STFT epilogue (fft.hip) and the real-time kernels (rt.hip) round their own way.
#pragma once
#include "common.h"

// re = xl.x xr.x + xl.y xr.y and im = xl.y xr.x - xl.x xr.y with the SECOND product of each rounded and the first fused into the sum:
// the roundings are stated here, so that the bits do not depend on how the compiler contracts the surrounding code.
__device__ __forceinline__ void phat_coherence(float2 xl, float2 xr, float& re, float& im) {
    const float aL = hypotf(xl.x, xl.y), aR = hypotf(xr.x, xr.y);
    re = fmaf(xl.x, xr.x, xl.y * xr.y);
    im = fmaf(xl.y, xr.x, -(xl.x * xr.y));
    if (aL > 0.f && aR > 0.f) {
        re = re / aL / aR;
        im = im / aL / aR;
    } else {
        re = 0.f;   // a bin that is exactly 0 in f32 carries no phase: it contributes nothing (NaN policy)
        im = 0.f;
    }
}
