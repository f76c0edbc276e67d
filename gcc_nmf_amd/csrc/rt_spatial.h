// Online spatial (multichannel Wiener) filter of the real-time block call, one launch between the mask and the synthesis kernels
// (rt_spatial.hip).
#pragma once
#include "common.h"

// First float of the filter's state behind the S history images [S][D][Lh] of `hist`: the first multiple of 4 floats.
static inline long gccnmf_rt_spatial_state_offset(int S, int D, int Lh) { return (((long)S * D * Lh + 3) / 4) * 4; }

// X [S][2][F][Tc] complex; Y [S][2][F][Tc] (single-target layouts, NT ignored) or [S][NT][2][F][Tc] (multi) complex: the masked spectra,
// overwritten in place with the filtered ones; rows [S][row_len] the target rows (word 7 = tau in frames, word 4 the bank's separation
// switch, read when bank != 0); state [S][NC][F][4] float32 = (p0, p1, Re q, Im q), NC = 2 (single-target: talker, residual) or NT,
// 16-byte aligned.  Arguments are checked by the caller (gccnmf_rt_process_block_ll); 1 <= NT <= 8.
int gccnmf_launch_rt_spatial(const float* X, float* Y, const float* rows, int row_len, int bank, float* state, int F, int Tc, bool multi,
                             int NT, int S, hipStream_t s);
