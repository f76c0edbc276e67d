// Ratio-mask (Wiener) reconstruction, one fused launch (ratio.hip: the kernel of ratio_kernel.h at two channels).
#pragma once
#include "common.h"

#define GCCNMF_RATIO_MAX_TARGETS 8

// spec[b][i*2+c] = X_c * (W.(H_c o M_i)) / den.  argmax != nullptr && masks == nullptr: one-hot form (den = sum_i of the numerators);
// masks != nullptr: soft form (den = W.H_c).  Arguments are checked by the caller (gccnmf_reconstruct); 1 <= S <= 8.
int gccnmf_launch_ratio(const float* W, const float* H, const unsigned char* argmax, const float* masks, const float* X, int F, int T,
                        int K, int S, int batch, float* spec, hipStream_t s);
