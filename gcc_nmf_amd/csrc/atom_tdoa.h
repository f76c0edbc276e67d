// Offline speech enhancement: every atom's own TDOA over the whole grid, and the talker / noise masks around a target direction
// (atom_tdoa.hip).  Both stages are modes of gccnmf_target_scores_masks (gcc.hip checks the arguments and calls these launchers).
#pragma once
#include "common.h"

#define ATOM_TDOA_MAX_D 1024                               // the streaming limit (rt_localize's 1024 threads)

// atom_tdoa [batch][Kp][Tp] unsigned short, atom_score [batch][Kp][Tp] float or NULL; every element of both is written
int gccnmf_launch_atom_tdoa(const float* CC, const float* trig, const float* W, int F, int T, int K, int D, int batch,
                            unsigned short* atom_tdoa, float* atom_score, hipStream_t s);

// target: [batch] int32, or with per_frame [batch][Tp]; image [batch][Kp][Tp] uint8 (0 = talker, 1 = noise) or NULL; masks
// [batch][2][Kp][Tp] float (talker, noise) or NULL; window: 0 = boxcar, 1 = window function
int gccnmf_launch_enhancement_masks(const unsigned short* atom_tdoa, const int* target, int per_frame, int window, float eps,
                                    float beta, float noise_floor, int T, int K, int batch, unsigned char* image, float* masks,
                                    hipStream_t s);
