// Spatial (multichannel Wiener) filter behind the ratio-mask reconstruction, two launches (spatial.hip).
#pragma once
#include "common.h"

#define GCCNMF_SPATIAL_MAX_TARGETS 8

// cov [batch][S][Fp][4] float32 = (R~00, R~11, Re R~01, Im R~01) of every (file, target, bin < F); spec [batch][S*2][Fp][Tp] complex is
// read (the ratio-mode estimates) and overwritten in place with the filtered estimates; X [batch][2][Fp][Tp] complex.  Arguments are
// checked by the caller (gccnmf_reconstruct); 1 <= S <= 8, cov 16-byte aligned.
int gccnmf_launch_spatial(const float* X, int F, int T, int S, int batch, float* cov, float* spec, hipStream_t s);
