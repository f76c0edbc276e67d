// Counting the talkers of a file from its mean angular spectrum (source_count.hip): the count mode of gccnmf_pick_tdoa_peaks
// (gcc.hip checks the arguments and calls this launcher).
#pragma once
#include "common.h"

#define SOURCE_COUNT_MAX_D 4096                            // the peak rule's limit: at most 2047 strict local maxima

// mean_ang [batch][Dp] float64; tdoa_idx [batch][Smax] int32 (the counted peaks in ascending order, then -1); status [batch] int32
// (0 = counted, 1 = no peak or a non-finite sum of heights, 2 = more than Smax counted: the Smax highest kept)
int gccnmf_launch_count_peaks(const double* mean_ang, int D, int Dp, int Smax, int batch, int* tdoa_idx, int* status, hipStream_t s);
