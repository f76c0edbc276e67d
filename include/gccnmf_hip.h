/* libgccnmf_hip.so -- C ABI of the MI355X (gfx950) GCC-NMF hot path.
 *
 * The reference (seanwood/gcc-nmf) is pure Python/NumPy and has no FFI; its "operator API" for
 * this path is the set of free functions in gccNMF/gccNMFFunctions.py + gccNMF/librosaSTFT.py.
 * Each entry point below states which of those functions (file:line in the reference checkout)
 * it computes.  gcc_nmf_amd/_hip.py is the ctypes binding; INTEGRATION.md shows the stub a
 * reference maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM), every call is asynchronous on `stream`
 *    (a hipStream_t passed as void*), every function returns a status code (0 = GCCNMF_OK);
 *    nothing throws across this boundary;
 *  - a "batch" is `batch` independent stereo mixture files of identical shape, laid out
 *    back to back with the per-file strides implied by the padded geometry below;
 *  - matrices are row-major float32 with padded pitches (gccnmf_pitches): padding is zero
 *    on entry and stays zero.  Complex data is interleaved (re, im) float32 pairs.
 *
 * Geometry (F = n_fft/2+1 bins, T frames, N = 2T NMF columns, K atoms, D TDOAs, S targets):
 *   Fp = round_up(F,16)  Kp = round_up(K,64)  Np = round_up(2T,64)  Tp = round_up(T,64)
 *   X  [batch][2][Fp][Tp] complex   complexMixtureSpectrogram   (gccNMFFunctions.py:61-67)
 *   V  [batch][Fp][Np]              concatenate(abs(X), -1)     (runGCCNMF.py:40)
 *   CC [batch][2][Fp][Tp]           Re / Im planes of the PHAT coherence (runGCCNMF.py:44)
 *   W  [batch][Fp][Kp]   H [batch][Kp][Np]                      (gccNMFFunctions.py:69-83)
 */
#ifndef GCCNMF_HIP_H
#define GCCNMF_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define GCCNMF_OK 0
#define GCCNMF_ERR_ARG 1
#define GCCNMF_ERR_LAUNCH 2
#define GCCNMF_ERR_UNSUPPORTED 3
#define GCCNMF_ERR_COLLECTIVE 4   /* the all-reduce hook of gccnmf_klnmf_shared_run (or RCCL behind gccnmf_rccl_*) failed */

/* flags for gccnmf_klnmf */
#define GCCNMF_FLAG_NO_XCD_AFFINITY 1   /* plain file-major block order instead of the XCD-affine map */
#define GCCNMF_FLAG_UNFUSED_W_UPDATE 2   /* R.H^T and the W update/normalisation as two launches (always so when F-1 > 512) */
#define GCCNMF_FLAG_CONCURRENT_GROUPS 4  /* another file group runs the same call on another stream: keep the throughput tile (a launch
                                          * that has the chip to itself may run its partial last round, or all of it, on half-height tiles) */
#define GCCNMF_FLAG_GROUPS(n) (GCCNMF_FLAG_CONCURRENT_GROUPS | ((n) << 8))   /* ... n equal groups in all (bits 8-15; 0 = two): launch forms that
                                          * are chosen by the size of a launch (tuning keys 16 / 17, the direct latency kernels of a handful of
                                          * files, the GEMM tile, the W-update kernel) are chosen for the n x batch files of all groups together,
                                          * so a file's result does not depend on how the batch was split */
#define GCCNMF_FLAG_FIXED_W (1 << 16)   /* a pre-trained dictionary: W is ONE [Fp][Kp] zero-padded dictionary shared by every file of the call,
                                          * read only (bit-identical after the call); H [batch][Kp][Np] holds the initial coefficients on entry and
                                          * the result on exit (h <- h o W^T(v / Wh) / (colsum W + alpha + eps), every iteration of the call in one
                                          * launch, csrc/nmf_fixed.hip).  V, workspace, sparsity_alpha and epsilon as for the blind call; the
                                          * chain-status words are left cleared.  Of the workspace the call writes only its head, den [Kp] (colsum W +
                                          * alpha + eps; 1 for a padding atom) | Wt [Kp][round_up(F, 32)] (W^T, zero outside F x K), and the
                                          * chain-status words.  F <= 2049 and K <= 1024, else GCCNMF_ERR_UNSUPPORTED.  Not
                                          * combinable with bits 0-15 (GCCNMF_ERR_ARG); gccnmf_klnmf_stage (but for its stage 7) / gccnmf_klnmf_ragged reject it */
#define GCCNMF_FLAG_H_ONES (1 << 17)    /* with GCCNMF_FLAG_FIXED_W only (else GCCNMF_ERR_ARG): the initial H is all ones (the streaming
                                          * processor's h0 = 1); H is output only and is not read */

#define GCCNMF_FLAG_FREE_ATOMS(n) ((n) << 18)     /* bits 18-25; 0 = not semi-supervised.  SEMI-SUPERVISED KL-NMF: per file W = [ W_fixed (F x (K - n)) |
                                          * W_free (F x n) ] -- the caller has put a pre-trained dictionary into columns [0, K - n) of every file's W
                                          * [batch][Fp][Kp] and the initial free atoms into the LAST n columns [K - n, K).  One iteration is performKLNMF's
                                          * with its W half restricted to the free columns:
                                          *     H      <- H o W^T(V / WH) / (colsum W + alpha + eps)      all K atoms             (gccNMFFunctions.py:76)
                                          *     R       = V / (W H)                                       with the new H
                                          *     W_free <- W_free o (R . H_free^T) / rowsum(H_free)        the n free columns only (:77)
                                          *     s = sqrt(sum_f W_free^2);  W_free /= s;  H_free *= s      free atoms only         (:79-81)
                                          * The fixed columns are never written (bit-identical after the call), are not normalised, and their rows of H are
                                          * not rescaled -- as in the fixed-dictionary call; padding rows, atoms and columns stay exactly zero; a free atom
                                          * whose row of H sums to 0 behaves as in the blind call.  V, W, H, the workspace and its size are exactly the blind
                                          * call's.  Plain launches: three of the four GEMMs are the blind call's in the forms that materialise R, R.H^T and
                                          * the W update run over the free atoms alone (csrc/nmf_semi.hip: one pass over R, every sum in an order fixed by
                                          * (F, N, K, n) -- a file's factors are bit for bit the same alone and in any batch).  The chain-status words are
                                          * cleared: nothing chains.  Decided before anything is launched -- GCCNMF_ERR_ARG: together with
                                          * GCCNMF_FLAG_FIXED_W, GCCNMF_FLAG_H_ONES, GCCNMF_FLAG_CONCURRENT_GROUPS or GCCNMF_FLAG_UNFUSED_W_UPDATE; n > 128;
                                          * n >= K.  GCCNMF_ERR_UNSUPPORTED: (K - n) % 16 != 0 (the free block starts on a float4 / atom-group boundary; the
                                          * dictionaries the reference trains have 64 ... 1024 atoms), K > 1024, F > 2049.  gccnmf_klnmf_ragged rejects the
                                          * bits (GCCNMF_ERR_ARG); gccnmf_klnmf_plan returns bit 5 alone, or -1 for a call these rules reject;
                                          * gccnmf_klnmf_stage takes the same bits (see there) */

/* bits 26-27: the divergence that gccnmf_klnmf / gccnmf_klnmf_stage minimise.  Both clear = Kullback-Leibler: every call that existed before
 * launches exactly what it launched.  ITAKURA-SAITO (beta = 0) and EUCLIDEAN (beta = 2) NMF, one file's iteration -- plain multiplicative
 * updates (exponent 1) in the structure of gccNMFFunctions.py:75-81, csrc/nmf_beta.hip:
 *     P = W.H                                    f32 on the matrix cores (v_mfma_f32_32x32x2_f32), as everywhere
 *     IS: Q = 1 / P, R = (V * Q) * Q             Euclid: Q = P, R = V              (KL would be R = V / P, Q = 1)
 *     H <- H o ((W^T R) / ((W^T Q + alpha) + eps))
 *     P, R, Q again with the new H
 *     W <- W o ((R H^T) / (Q H^T))               no eps, as in the KL W update
 *     s = sqrt(sum_f W^2);  W /= s;  H *= s      (:79-81)
 * Every element-wise operation is a float32 operation rounded on its own in the order written (IEEE quotients and square root; sum_f W^2 an
 * fmaf chain); every GEMM element is ONE fma chain over its reduction index in ascending order, so every sum is in an order fixed by
 * (F, N, K) alone: one launch form whatever the batch and the tuning keys, and a file's factors are bit for bit the same alone, in any batch
 * and at any place in it.  R and Q are exactly zero outside f < F, n < N (1 / P of a padded element never reaches a reduction), the padding
 * of W and H stays exactly zero; inside the matrix P = 0 propagates Inf / NaN as IEEE says, like KL's V / 0, and V = 0 gives R = 0.  V is any
 * non-negative matrix: magnitudes or powers are the caller's choice.
 * Five plain launches per iteration (the numerator and denominator GEMMs of a half share one); nothing chains, the chain-status words are
 * cleared; gccnmf_klnmf_plan returns bit 6 alone.  Decided before anything is launched -- GCCNMF_ERR_ARG: both bits; either bit together with
 * GCCNMF_FLAG_FIXED_W, GCCNMF_FLAG_H_ONES, GCCNMF_FLAG_FREE_ATOMS, GCCNMF_FLAG_CONCURRENT_GROUPS or GCCNMF_FLAG_UNFUSED_W_UPDATE; either bit on
 * gccnmf_klnmf_ragged.  GCCNMF_ERR_UNSUPPORTED: F > 2049 or K > 1024 (the envelope: 2 <= F <= 2049, 1 <= K <= 1024, any N >= 1, any batch).
 * The workspace of such a call is LARGER than the KL call's: gccnmf_klnmf_workspace_floats(F, N, K, batch) floats laid out as for KL,
 * followed by GCCNMF_KLNMF_DIVERGENCE_WORKSPACE_FLOATS(Fp, Kp, Np, batch) more (see gccnmf_klnmf_stage for what sits where). */
#define GCCNMF_FLAG_DIVERGENCE_IS (1 << 26)
#define GCCNMF_FLAG_DIVERGENCE_EUCLIDEAN (2 << 26)
/* floats an IS / Euclidean call needs BEHIND the gccnmf_klnmf_workspace_floats(F, N, K, batch) floats of the KL layout: Q [batch][Fp][Np] |
 * Ud [batch][Fp][Kp].  A multiple of 64 floats (Kp and Np are multiples of 64); the KL layout is a multiple of 32 floats, so both blocks
 * start 16-byte aligned when the workspace does (it must: GCCNMF_ERR_ARG otherwise). */
#define GCCNMF_KLNMF_DIVERGENCE_WORKSPACE_FLOATS(Fp, Kp, Np, batch) ((long)(batch) * (Fp) * ((long)(Np) + (Kp)))

/* TEMPORAL-CONTINUITY KL-NMF, bits 28-29 of `flags` of gccnmf_klnmf, gccnmf_klnmf_stage and gccnmf_klnmf_plan (csrc/nmf_smooth.hip): KL-NMF
 * whose H update carries Virtanen's temporal-continuity term (IEEE TASLP 2007) with the ABSOLUTE weight beta >= 0 (in units of V).  The
 * columns are `segments` equal runs of T = N / segments frames -- 1, or with GCCNMF_FLAG_CONTINUITY_STEREO 2, the GCC-NMF layout [L | R];
 * nothing couples across a segment boundary or into the padding.  Per file, atom and segment, with h = s * H the materialised gains:
 *     E = sum_t h_t^2     D = sum_{t >= 1} (h_t - h_{t-1})^2     cost c = T D / E
 *     Gp_t = 2 T n_t h_t / E                                 n_t = the neighbours inside the segment (2, at the ends 1, T = 1: 0)
 *     Gm_t = 2 T (h_{t-1} + h_{t+1}) / E + 2 T h_t D / E^2   a missing neighbour adds 0;  E = 0 -> Gp = Gm = 0
 *     H <- h o ((W^T (V / (W h)) + beta Gm) / (((colsumW + alpha) + beta Gp) + eps))
 * (Gp - Gm = dc / dh_t; Jacobi: every neighbour is the value from before the stage); the W update, the normalisation and H *= s are KL's.
 * E, D, Gm and Gp are formed in float64 from the exact products s * H, summed in an order fixed by (N, segments) alone, and rounded once to
 * float32; every element-wise operation of the H update is a float32 operation rounded on its own in the order written (the file's header
 * states each).  ONE launch form whatever the batch and the tuning keys, no atomics: a file's factors are bit for bit the same alone, in
 * any batch and at any place in it.  Seven plain launches per iteration; nothing chains, the chain-status words are cleared;
 * gccnmf_klnmf_plan returns bit 7 alone.
 * THE WEIGHT has no argument of its own: with GCCNMF_FLAG_CONTINUITY set -- and only then -- its float32 bits are read from the upper
 * halves of the K and batch arguments, so pass GCCNMF_CONTINUITY_K(K, bits) and GCCNMF_CONTINUITY_BATCH(batch, bits) there (K and batch
 * themselves are then at most 65535).  Decided before anything is launched -- GCCNMF_ERR_ARG: the stereo bit without the continuity bit; a
 * weight that is negative, NaN or Inf; two segments with N odd; either bit together with GCCNMF_FLAG_FIXED_W, GCCNMF_FLAG_H_ONES,
 * GCCNMF_FLAG_FREE_ATOMS, GCCNMF_FLAG_DIVERGENCE_*, GCCNMF_FLAG_CONCURRENT_GROUPS or GCCNMF_FLAG_UNFUSED_W_UPDATE; either bit on
 * gccnmf_klnmf_ragged.  GCCNMF_ERR_UNSUPPORTED: F > 2049 or K > 1024 (the envelope: 2 <= F <= 2049, 1 <= K <= 1024, any N >= 1, batch <=
 * 65535).  The padding of H may hold anything on entry (NaN included) and never reaches a result; the H update writes +0 into the padding
 * columns of the rows k < K.  The workspace is LARGER than the KL call's: gccnmf_klnmf_workspace_floats(F, N, K, batch) floats laid out as
 * for KL, followed by GCCNMF_KLNMF_CONTINUITY_WORKSPACE_FLOATS(Kp, Np, batch) more (see gccnmf_klnmf_stage for what sits where).  A call
 * without bit 28 launches exactly what it launched before the bits existed.  Bit 30 is free. */
#define GCCNMF_FLAG_CONTINUITY (1 << 28)
#define GCCNMF_FLAG_CONTINUITY_STEREO (1 << 29)
#define GCCNMF_CONTINUITY_K(K, weight_bits) ((int)((unsigned)(K) | ((unsigned)(weight_bits) & 0xffff0000u)))
#define GCCNMF_CONTINUITY_BATCH(batch, weight_bits) ((int)((unsigned)(batch) | ((unsigned)(weight_bits) << 16)))
/* floats a temporal-continuity call needs BEHIND the KL layout: Gm | Gp [batch][Kp][Np] each | E | D [batch][2][Kp] each.  A multiple of
 * 4 floats; the KL layout is a multiple of 32 floats, so every block starts 16-byte aligned when the workspace does. */
#define GCCNMF_KLNMF_CONTINUITY_WORKSPACE_FLOATS(Kp, Np, batch) ((long)(batch) * (Kp) * (2 * (long)(Np) + 4))

int gccnmf_version(void);

/* Tuning knobs: process-global atomics; every library call works on a snapshot taken at its entry.  Results stay valid (and, where a
 * knob only changes the launch form, bitwise the same) for every value of a PRODUCT key.  Keys marked X exist only in the lab build
 * (make EXPERIMENTS=1 -> libgccnmf_hip_exp.so): the product library rejects them with GCCNMF_ERR_ARG and carries none of the code they
 * select.  The authoritative table (defaults, ranges) is csrc/common.h.
 *   2  GEMM tile policy: 0 by launch size, 1 always the 512 x 64 throughput tile, 2 always the 128 x 64 small-batch tile (tests cover both)
 *   3  1 (default) = throughput tiles stage operands by LDS-DMA (csrc/gemm_dma.h), 0 = through registers (csrc/gemm_mfma.h)
 *   7  1 (default) = V / (W.H) is the IEEE quotient like numpy.divide, 0 = v_rcp_f32 + one Newton step (rare 1-ulp differences)
 *   8  file groups (1..4, default 3) of a shared-dictionary shard that cannot fill the chip, on library-owned streams
 *   9  throughput-tile launch forms: 1 (default) by the launcher's cost model -- full tiles | whole rounds of full tiles + the remaining files
 *      half-height | half-height throughout; outputs of at most 256 rows always half-height; a file's ragged last column tile (at most 32 of its
 *      64 columns exist: N = 1244) as a NARROW 512 x 32 item -- 0 = full tiles only, 2 = every tile as two narrow halves, 3 = half-height
 *      everywhere (tests).  Same k order per element: bitwise the same in every form.
 *  10  1 (default) = launches that cannot fill the chip (one mixture alone, up to key-12 files) take the direct-to-register kernels
 *      (csrc/direct.hip); 0 = the ring (csrc/gemm_ring.h) and throughput kernels.   12  largest batch on the direct path (1..8, default 4)
 *  16 / 17  short dictionaries (K <= 128, F = 64 n + 1 <= 513): K1 + K2 as one launch of column tiles / K3 + K4a as one launch of bin slabs
 *      (R never written): 0 never, 1 (default) by a cost model in rounds of 512 workgroups, 2 whenever the shape allows
 *  21  batch scale, K > 256: 1 (default) = the whole gccnmf_klnmf call -- every GEMM of every iteration -- as ONE chained launch whose
 *      workgroups hand tiles over through ready counters in their XCD's L2 (csrc/gemm_dma.h: GemmSync), where that wins: at least three files
 *      per XCD, balanced whole-file lists, no other file group beside it; 0 = never; forced forms for tests and A/B runs: 2 = K1 | K2, 4 = the
 *      four GEMMs of an iteration, 8 = every iteration of the call.  Bitwise the same factors in every form.
 *  23  lists of a chained launch: 1 (default) = whole files per XCD where they balance, else the tile list in equal eighths with agent-scope hand-over;
 *      0 = the plain launch's lists (batch a multiple of 8); 2 = always spread; 3 = always whole files
 *  24  iterations per chained launch (default 2048; a call of more iterations is several chained launches)
 *   X  the two test hooks of the lab build: 22 chained launches with one workgroup per CU, 25 fault injection into the chained launches'
 *      hand-over (consumers give up at once)
 *   -  0, 1, 4, 5, 6, 11, 13, 14, 15, 18, 19, 20 are unused: they selected measured-and-rejected kernel paths that are gone (LABBOOK.md);
 *      every build answers GCCNMF_ERR_ARG.  The numbers of the other keys are stable.
 * gccnmf_klnmf_plan reports what a call would launch.  Unknown keys / values: GCCNMF_ERR_ARG. */
int gccnmf_set_tuning(int key, int value);

/* Padded geometry every other entry point assumes. */
int gccnmf_pitches(int F, int T, int K, int* Fp, int* Kp, int* Np, int* Tp);

/* Stereo STFT + magnitude + PHAT coherence, one launch for the whole batch.
 * Replaces computeComplexMixtureSpectrogram (gccNMFFunctions.py:61-67 -> librosaSTFT.py:126-181,
 * center=False, result conjugated), V = concatenate(abs(X)) (runGCCNMF.py:40) and
 * spectralCoherenceV (runGCCNMF.py:44).
 *   x        [batch][2][n_samples] float32 (file stride x_stride floats)
 *   window   [n_fft] float32 analysis window (numpy.hanning(n_fft) for the reference path)
 *   twiddle  [n_fft/2] complex: exp(-2j*pi*k/n_fft), computed in float64 on the host
 *   X, V, CC as in the geometry table; V or CC may be NULL to skip that output.
 * n_fft must be a power of two in [64, 4096] here -- the radix-2 kernel keeps eight frames per workgroup in LDS (four at
 * n_fft = 4096); other sizes GCCNMF_ERR_ARG.  The same holds for gccnmf_istft_ola.  Every other size goes through
 * gccnmf_stft_dft / gccnmf_istft_dft below (the Python stft / istft choose). */
int gccnmf_stft_stereo(const float* x, long x_stride, int n_samples, int n_fft, int hop, int T, int batch,
                       const float* window, const float* twiddle, float* X, float* V, float* CC, void* stream);

/* ANY n_fft (2..8192, e.g. 400, 1000, 1536): the reference's stft / istft accept every size (scipy.fftpack, librosaSTFT.py:162-179,
 * :276-279).  Off the power-of-two sizes the transform is computed as the real GEMM it is, on the matrix cores (csrc/fft.hip):
 *   gccnmf_stft_dft : x [nsig][n_samples] real signals (x_stride floats apart) -> X [nsig][Fp][Tp] complex (= conj(fft), center=False)
 *     basis [round_up(n_fft,16)][2*Fp]: basis[n][f] = w[n] cos(2 pi f n / n_fft), basis[n][Fp+f] = w[n] sin(..), zero elsewhere
 *   gccnmf_istft_dft: spec [nsig][Fp][Tp] complex -> y [nsig][L], L = n_fft + hop*(T-1) - (center ? n_fft : 0); n_fft even
 *     ibasis [2*Fp][round_up(n_fft,64)]: ibasis[k][n] = c_k w[n] cos(2 pi k n / n_fft) / n_fft, ibasis[Fp+k][n] = c_k w[n] sin(..) / n_fft,
 *     c_0 = c_{n_fft/2} = 1, else 2 (the real part of ifft([conj(S), S[-2:0:-1]]) times the synthesis window)
 *   both tables are evaluated in float64 by the caller; workspace: gccnmf_dft_workspace_floats(n_fft, T, nsig) floats. */
long gccnmf_dft_workspace_floats(int n_fft, int T, int nsig);
int gccnmf_stft_dft(const float* x, long x_stride, int n_samples, int n_fft, int hop, int T, int nsig, const float* basis,
                    float* workspace, float* X, void* stream);
int gccnmf_istft_dft(const float* spec, int nsig, int n_fft, int hop, int T, const float* ibasis, float gain, int center, float* workspace,
                     float* y, void* stream);

/* The same with the wav ingest fused in: pcm = interleaved int16 stereo frames [batch][n_samples][2]
 * exactly as they sit in a wav data chunk (frame_stride stereo frames between files); the /32768 conversion of
 * wavread -> pcm2float (gccNMF/wavfile.py:34-37, :57-89) and the de-interleave happen in the STFT's load. */
int gccnmf_stft_stereo_pcm16(const short* pcm, long frame_stride, int n_samples, int n_fft, int hop, int T, int batch,
                             const float* window, const float* twiddle, float* X, float* V, float* CC, void* stream);

/* wav egress on the device: y [groups][2][L] float32 -> pcm [groups][L][2] int16 with wavwrite's clip protection per
 * group (peak >= 1 -> rescale to 0.99) and float2pcm's clip + truncation (gccNMF/wavfile.py:39-48, :92-131).  One group
 * = one target of one file = one wavwrite call.  peak_scratch: `groups` uint32 of device scratch; on return it holds the bit
 * image of each group's peak |y|, and an image >= 0x7F800000 means the group contained NaN / Inf samples (NaN is written as 0,
 * +-Inf clips, no rescale; the reference's result is platform-defined there) -- the caller should treat it as an error. */
int gccnmf_pack_pcm16(const float* y, int groups, int L, unsigned int* peak_scratch, short* pcm, void* stream);

/* KL-NMF multiplicative updates, independent dictionary per file.
 * Replaces the iteration loop of performKLNMF (gccNMFFunctions.py:75-81); the MT19937 initial
 * W, H (:70-73) are drawn on the host and passed in.  W and H are updated in place.
 *   V [batch][Fp][Np], W [batch][Fp][Kp], H [batch][Kp][Np] with Np = round_up(N,64); N = 2T on the
 *   GCC-NMF path but any N >= 1 is accepted (performKLNMF is also called on arbitrary V).
 *   workspace: gccnmf_klnmf_workspace_floats(...) floats of scratch (R, R.H^T, K-vectors; for batch == 1 also a reserved,
 *   unused block, for up to 8 files the transposed copies of the direct path, and at its end the counters and status words of the chained launches).  Always size it with the
 *   batch of the call it is used with.  The size is a multiple of 4 floats for every valid argument tuple (so is every other
 *   *_workspace_floats of this header), and `workspace` must be 16-byte aligned, else GCCNMF_ERR_ARG before anything is launched -- here, in
 *   gccnmf_klnmf_ragged and in gccnmf_klnmf_stage: its blocks are read with 16-byte vector loads and LDS-DMA.  Workspaces carved back to back
 *   out of one aligned allocation, each of the size this function returns, therefore all qualify.
 *   batch >= 2: a file's result is bit-identical whatever batch it rides in (for equal launch-size decisions); a file alone
 *   or among a few takes the direct kernels (csrc/direct.hip), which sum in another fixed order (deterministic, summation-order accuracy). */
long gccnmf_klnmf_workspace_floats(int F, int N, int K, int batch);
int gccnmf_klnmf(const float* V, float* W, float* H, float* workspace, int F, int N, int K, int batch,
                 int iterations, float sparsity_alpha, float epsilon, int flags, void* stream);

/* The same for mixtures of DIFFERENT lengths in one call (the reference separates a file of any length, gccNMF/runGCCNMF.py:30-36; a
 * batch of them shards "independent mixture files" whatever their durations): file b has N[b] <= Nmax columns (N: HOST array of `batch`
 * ints), every file's V / H block has the pitches of Nmax (gccnmf_pitches(F, Nmax / 2, K)), zero beyond its own columns.  One chained
 * launch (tuning key 21) whose work lists hold each file's own column tiles -- padding to the 64-column tile only -- dealt out to the
 * XCDs by length; a file's factors are bit for bit those of gccnmf_klnmf on a batch of files of its length.  GCCNMF_ERR_UNSUPPORTED where
 * the chained form does not exist (K <= 128 or not a multiple of 128, fewer than 8 files or 256 column tiles, more than 248 files,
 * F - 1 not a multiple of 128 up to 512): run the files of each length as a batch of their own then.
 * workspace: gccnmf_klnmf_ragged_workspace_floats(F, Nmax, K, batch) floats (a multiple of 4), 16-byte aligned. */
long gccnmf_klnmf_ragged_workspace_floats(int F, int Nmax, int K, int batch);
int gccnmf_klnmf_ragged(const float* V, float* W, float* H, float* workspace, int F, const int* N, int Nmax, int K, int batch,
                        int iterations, float sparsity_alpha, float epsilon, int flags, void* stream);

/* After a synchronisation: did the chained launches of the last gccnmf_klnmf / gccnmf_klnmf_ragged call on `workspace` hand over cleanly?
 * *status = 0: yes (or the call did not chain); bit 0: a consumer gave up waiting for its producer; bit 1: the workgroups of a work list ran
 * on more than one XCC.  In both cases the call has already turned W and H into NaN (never plausible-looking garbage); this is the explicit
 * check (a blocking 128-byte read).  F, N, K, batch as for the workspace size (N = Nmax for a ragged batch). */
int gccnmf_klnmf_chain_status(const float* workspace, int F, int N, int K, int batch, int* status);

/* Which launches gccnmf_klnmf uses for this problem under the current tuning: bit 0 = the direct latency kernels (a handful of files),
 * bit 1 = K1 + K2 as one launch of column tiles (tuning key 16), bit 2 = K3 + K4a as one launch of 64-bin slabs (key 17), bit 3 = the whole
 * call as one chained launch (key 21), bit 4 = the fused fixed-dictionary launch (GCCNMF_FLAG_FIXED_W; then no other bit), bit 5 = the semi-supervised
 * iteration (GCCNMF_FLAG_FREE_ATOMS; then no other bit), bit 6 = the Itakura-Saito / Euclidean iteration (GCCNMF_FLAG_DIVERGENCE_*; then no other
 * bit), bit 7 = the temporal-continuity iteration (GCCNMF_FLAG_CONTINUITY, K and batch carrying the weight as for gccnmf_klnmf; then no other
 * bit).  -1 on bad arguments (a flag combination gccnmf_klnmf rejects, or a fixed-dictionary, semi-supervised, IS / Euclidean or
 * temporal-continuity shape outside its envelope).
 * (Benchmarks and tests name the kernel they time by this; the result of gccnmf_klnmf does not depend on it beyond round-off.) */
int gccnmf_klnmf_plan(int F, int N, int K, int batch, int flags);

/* One launch group of the iteration on its own (per-kernel tests and per-kernel timing in bench.py).
 * stage: 0 prepare (zero R, colsum W, scale = 1) | 1 R=V/(W.(s*H)) | 2 H update | 3 R=V/(W.H) |
 *        4 U=R.H^T + rowsum H | 5 W update + atom normalisation | 6 materialise H *= s |
 *        7 KL divergence of the current factors (csrc/divergence.hip), per file b
 *              D_b = sum_{f < F, n < N} V log(V / R) - V + R,   R = W.H in f32 on the matrix cores (never stored),
 *          a V = 0 element contributing R alone; each term is formed in float32 as R g((V - R) / R), g(x) = (1 + x) log1p(x) - x (its
 *          series for |x| < 1/8: no cancellation near V = R), and summed in float64 from the tile on, in an order fixed by (F, N): no
 *          atomics, D_b is bit for bit the same for a file alone, in any batch, and from run to run.  Valid whenever W and H are
 *          materialised -- before a gccnmf_klnmf call or after a complete one, not between stages 1-6; V, W and H are read only, and only
 *          inside f < F, n < N, k < K (their padding is not read into the result).  The result is `batch` float64 values at
 *              (const double*)(workspace + (size_t)batch * Fp * Np)          -- the start of the U region: a multiple of 4096 bytes from
 *          `workspace`, hence 16-byte aligned like the workspace itself (which must be 16-byte aligned for every stage, else GCCNMF_ERR_ARG); the tile partials, ceil(F / 128) * ceil(N / 64) float64 per
 *          file, go to the head of each file's [Fp][Np] block of the R region (workspace + b * Fp * Np).  Both are scratch of the
 *          iteration, far below the chain counters and status words at the workspace's end, which stage 7 neither reads nor writes;
 *          because R's zero padding is overwritten, stage 0 (every gccnmf_klnmf call starts with it) must run before further stages
 *          1-6.  sparsity_alpha, epsilon and bits 0-15 of flags are ignored.  flags = GCCNMF_FLAG_FIXED_W (exactly) is accepted by
 *          this stage alone: W is then ONE [Fp][Kp] dictionary shared by every file, as in the fixed-dictionary call.
 * Any other stage number: GCCNMF_ERR_ARG.
 * Where stages 0-6 keep their intermediates (tests read them by offset; floats from `workspace`, batch = the call's):
 *     R        [batch][Fp][Np]      zero outside f < F, n < N from stage 0 on (a reduction operand of stages 2 and 4)
 *     U        [batch][Fp][Kp]      R.H^T; its padding is nobody's operand and keeps whatever the workspace held
 *     colsumW  [batch][Kp]
 *     rowsumH  [batch][Kp]
 *     hscale   [batch][Kp]          the lazy atom scale s: the H of the algorithm is s * H until stage 6
 *     (batch == 1 only: 4 * (max(Fp * Np, Fp * Kp) + Kp) floats kept for the lab build's split reductions)
 *     (batch <= 8) the direct kernels' transposed copies  Wt [batch][Kp][Fp] | Ht [batch][Np][Kp] | Rt [batch][Np][Fp]
 *   followed by the counters and status words of the chained launches.  Stage 0 establishes R = 0, colsumW, hscale = 1 (and Wt = W^T,
 *   Ht = Rt = 0 on the direct path); U and rowsumH are written before they are read.
 * Which stage writes what depends on the launch form (gccnmf_klnmf_plan; a stage that has nothing left to do returns GCCNMF_OK and
 * writes nothing):
 *     four launches              1: R | 2: H | 3: R | 4: U, rowsumH | 5: W, hscale, colsumW | 6: H
 *     plan bit 1 (K1 + K2)       1: H, R is not written | 2: nothing
 *     plan bit 2 (K3 + K4a)      3: U, rowsumH, R is not written | 4: nothing (but for the files a partial slab launch left to the two launches)
 *     W update in the epilogue of R.H^T (128 < Fm <= 512 on the throughput tile, neither GCCNMF_FLAG_UNFUSED_W_UPDATE nor plan bit 2; no
 *       plan bit)                4: W, hscale, colsumW, U and rowsumH are not written | 5: nothing
 *     plan bit 0 (direct)        0: also Wt | 2: H and Ht | 3: Rt and, of R, bin F - 1 alone (F = 16 n + 1) | 4: U, rowsumH from Rt and Ht | 5: W and Wt
 * With GCCNMF_FLAG_FREE_ATOMS(n) in flags (same argument rules as gccnmf_klnmf, decided first): stages 0, 1, 2, 3, 6 and 7 mean what they mean
 * without it, but stages 1-3 always take forms that leave R [batch][Fp][Np], zero padded, in the workspace (K1 + K2 fused included: stage 3
 * rewrites R; never the direct kernels or the K3 + K4a slab launch); stage 4 writes U[:, K - n : K] and rowsumH[K - n : K] only, at their ordinary
 * places, stage 5 updates W[:, K - n : K], hscale[K - n : K] and colsumW[K - n : K] only: what belongs to the fixed atoms is not written (hscale
 * stays 1 and colsumW what stage 0 computed).  A call without the bits launches exactly what it launched before they existed.
 * With GCCNMF_FLAG_DIVERGENCE_IS or GCCNMF_FLAG_DIVERGENCE_EUCLIDEAN in flags (same argument rules as gccnmf_klnmf, decided first; one launch
 * form, csrc/nmf_beta.hip) the stages are, with the lazy scale s = hscale as above:
 *     0: colsumW = sum_f W, s = 1, R = Q = 0 | 1: R, Q from P = W.(s * H) | 2: H <- (s * H) * ((W^T.R) / ((W^T.Q + alpha) + eps)) |
 *     3: R, Q from P = W.H | 4: Un = R.H^T, Ud = Q.H^T | 5: Wt = W * (Un / Ud), s = sqrt(sum_f Wt^2), W = Wt / s, colsumW = sum_f W |
 *     6: H *= s | 7: that divergence of the current factors, per file, float32 terms summed in float64 in stage 7's order, same places:
 *          IS      sum over the elements with V > 0 of x - log1p(x), x = (V - R) / R, R = W.H (= V / R - log(V / R) - 1; its series for
 *                  |x| < 1/8: no cancellation near V = R).  A V = 0 element contributes NOTHING: IS is +infinity there, so the value is
 *                  the divergence over the support of V
 *          Euclid  sum of 1/2 (V - R)^2
 *   with  IS: Q = 1 / P, R = (V * Q) * Q    Euclid: Q = P, R = V.   Where the intermediates sit (floats from `workspace`; KL = the value of
 *   gccnmf_klnmf_workspace_floats(F, N, K, batch)):
 *     R        [batch][Fp][Np]      at 0, as for KL; stages 1 and 3 write the whole padded block, exact zeros outside f < F, n < N
 *     Un       [batch][Fp][Kp]      at batch * Fp * Np: KL's U
 *     colsumW, rowsumH (not used), hscale [batch][Kp] each, behind Un as for KL; then the rest of the KL layout, of which the status words
 *                                   alone are used
 *     Q        [batch][Fp][Np]      at KL; zero padded like R
 *     Ud       [batch][Fp][Kp]      at KL + batch * Fp * Np
 *   The padding of Un and Ud is nobody's operand and keeps whatever the workspace held.
 * With GCCNMF_FLAG_CONTINUITY in flags (same argument rules and weight carriage as gccnmf_klnmf, decided first; one launch form,
 * csrc/nmf_smooth.hip): stages 0, 1, 3, 4, 5, 6 and 7 mean what they mean for KL, always as launches that leave R, U and rowsumH
 * materialised at their KL places (stages 1 and 3 write the whole padded R block; never the direct, fused or chained forms); stage 2 is the
 * continuity launch (E, D, Gm, Gp from H and hscale) followed by the H-update launch.  Behind the KL layout (KL = the value of
 * gccnmf_klnmf_workspace_floats(F, N, K, batch)):
 *     Gm       [batch][Kp][Np]      at KL; written inside k < K, n < N alone, like Gp
 *     Gp       [batch][Kp][Np]      at KL + batch * Kp * Np
 *     E        [batch][2][Kp]       at KL + 2 * batch * Kp * Np; [b][segment][k], the second plane is written with two segments only
 *     D        [batch][2][Kp]       at KL + 2 * batch * Kp * Np + 2 * batch * Kp */
int gccnmf_klnmf_stage(const float* V, float* W, float* H, float* workspace, int F, int N, int K, int batch,
                       float sparsity_alpha, float epsilon, int flags, int stage, void* stream);

/* Shared-dictionary KL-NMF building blocks (one W for all files / all ranks; the host all-reduces
 * `partial` across ranks between the two calls -- realtime/gccNMFPretraining.py:79-80 is the
 * reference use of performKLNMF on one big V).
 *   step A: H update with the current W, then partial[0:Fp*Kp] = sum_files (V/WH).H^T and
 *           partial[Fp*Kp : Fp*Kp+Kp] = sum_files rowsum(H)   (deterministic file-order sum)
 *   step B: W *= num/den, atom normalisation, and the compensating H rescale (applied lazily
 *           through `workspace`; gccnmf_klnmf_shared_finish materialises it).
 * Where the four calls keep their intermediates (tests read them by offset; floats from `workspace`; V [batch][Fp][Np], H [batch][Kp][Np],
 * W [Fp][Kp] with zero padding, as everywhere):
 *     R            [batch][Fp][Np]   zero outside f < F, n < N from begin on (a reduction operand of K2 and K4a)
 *     Upart        [batch][Fp][Kp]   per file (V/WH).H^T; its padding is nobody's operand and keeps whatever the workspace held
 *     rowsum_part  [batch][Kp]       per file rowsum(H)
 *     (batch == 1 only: 4 * (max(Fp * Np, Fp * Kp) + Kp) floats kept for the lab build's split reductions, then the direct kernels'
 *      transposed copies  Wt [Kp][Fp] | Ht [Np][Kp] | Rt [Np][Fp])
 *     colsumW      [Kp]              one vector for every file, as W is one dictionary
 *     hscale       [Kp]              the lazy atom scale: the H of the algorithm is hscale * H until finish
 *   = gccnmf_klnmf_shared_workspace_floats(F, N, K, batch) floats.  partial = num [Fp][Kp] | den [Kp] = gccnmf_klnmf_shared_partial_floats.
 * A shard of gccnmf_klnmf_shared_run (below) has the same workspace without the two trailing vectors -- they are the call's `vec`,
 * colsumW [Kp] | hscale [Kp] -- and, for ld > 0, R as ONE [Fp][ld] matrix with file b at columns [b*N, b*N + N) (from column 0 whatever
 * column of the caller's matrix V and H point at); the single-file blocks are present for batch == 1 with ld == 0 or ld == Np.
 * Which call writes what (everything else keeps its bits; the padding of W, H, R and Rt stays zero):
 *     begin    colsumW = sum_f W, hscale = 1, R = 0 (single-file layout: Wt = Ht = Rt = 0 as well)
 *     step A   H, R (= V / W.H with the new H), Upart, rowsum_part, partial: per shard s = 0; s += part[b] for b = 0, 1, ... in float32,
 *              partial = s for the call's first shard, partial + s for each later one.  One file under the default tuning takes the direct
 *              kernels: Wt = W^T, Ht = (new H)^T, the final quotient is written transposed to Rt and, of R itself, to bin F - 1 alone
 *              (F = 16 n + 1) -- the rest of R keeps K1's quotient.
 *     step B   W, hscale, colsumW from partial (num, den); Wt is not touched (step A transposes W anew every time)
 *     finish   H *= hscale, then hscale = 1 (all Kp entries) */
long gccnmf_klnmf_shared_workspace_floats(int F, int N, int K, int batch);
long gccnmf_klnmf_shared_partial_floats(int F, int K);
int gccnmf_klnmf_shared_begin(const float* W, float* workspace, int F, int N, int K, int batch, void* stream);
int gccnmf_klnmf_shared_step_a(const float* V, const float* W, float* H, float* workspace, float* partial, int F,
                               int N, int K, int batch, float sparsity_alpha, float epsilon, void* stream);
int gccnmf_klnmf_shared_step_b(float* W, float* workspace, const float* partial, int F, int N, int K, int batch,
                               void* stream);
int gccnmf_klnmf_shared_finish(float* H, float* workspace, int F, int N, int K, int batch, void* stream);

/* The same training as ONE call per rank: begin, `iterations` x (step A of every shard -> all-reduce -> step B), finish, all
 * enqueued on `stream` from C -- no host round trip per iteration (gccnmf_klnmf_shared_step(..., ncclComm_t)).
 * A rank's columns are given as up to GCCNMF_MAX_SHARDS shards of `batch` equally wide files each:
 *   ld == 0  whole padded matrices back to back: V [batch][Fp][Np], H [batch][Kp][Np]  (the layout of every other entry point)
 *   ld  > 0  column blocks of ONE matrix with row pitch ld: file b = columns [b*N, b*N + N) of V [Fp][ld] / H [Kp][ld]
 *            (N a multiple of 64 unless batch == 1; batch*N <= ld; columns beyond a ragged block's N up to the next multiple
 *            of 64 must be allocated and zero) -- the frame windows of one long mixture without gather / scatter.
 *   workspace: gccnmf_klnmf_shared_shard_workspace_floats(F, N, K, batch, ld) floats of scratch per shard.
 * nshards == 0 is a rank without columns (fewer files than ranks): it contributes zeros and still applies every W update.
 *   W [Fp][Kp] in/out (identical on every rank on entry -> identical on exit), partial: gccnmf_klnmf_shared_partial_floats
 *   floats, vec: 2*Kp floats of scratch.  The shards' partial sums are added in shard order (deterministic).
 * allreduce: sums `count` floats of `buf` (device memory) in place over all ranks, ordered on `stream`; returns 0 on success.
 *   NULL = single rank.  Not re-entrant per device: the file groups of a shard that cannot fill the chip run on side streams and
 *   events the library owns, one set per device (tuning key 8) -- one training at a time per device, like the reference's
 *   single-threaded caller.  ENFORCED: a call that arrives while another thread is still inside this function for the same device
 *   returns GCCNMF_ERR_UNSUPPORTED without launching anything.  gccnmf_rccl_allreduce below is the RCCL implementation; any other transport (MPI, a host callback that
 *   runs torch.distributed over gloo ...) has the same signature. */
#define GCCNMF_MAX_SHARDS 8
typedef struct gccnmf_shared_shard {
    const float* V;
    float* H;
    float* workspace;
    int N, batch, ld;
} gccnmf_shared_shard;
typedef int (*gccnmf_allreduce_fn)(void* ctx, float* buf, long count, void* stream);
long gccnmf_klnmf_shared_shard_workspace_floats(int F, int N, int K, int batch, int ld);
int gccnmf_klnmf_shared_run(const gccnmf_shared_shard* shards, int nshards, float* W, float* partial, float* vec, int F, int K,
                            int iterations, float sparsity_alpha, float epsilon, gccnmf_allreduce_fn allreduce, void* allreduce_ctx,
                            void* stream);

/* RCCL binding for the hook above (csrc/collective.hip).  librccl.so.1 is bound at run time with dlopen (the copy already
 * loaded into the process, e.g. PyTorch's, else the system one): the library loads without RCCL, these calls then return
 * GCCNMF_ERR_COLLECTIVE.  One process per GPU: rank 0 calls gccnmf_rccl_unique_id and hands the 128 bytes to every rank
 * (any out-of-band channel), every rank calls gccnmf_rccl_comm_init with the device it computes on current.
 *   gccnmf_rccl_allreduce(comm, buf, count, stream): ncclAllReduce(buf, buf, count, ncclFloat32, ncclSum, comm, stream) --
 *   pass it as `allreduce` with allreduce_ctx = comm.  The reference has no collectives; this is the exchange
 *   of the shared-dictionary W update (gccNMFFunctions.py:77 summed over every rank's columns). */
#define GCCNMF_RCCL_UNIQUE_ID_BYTES 128
int gccnmf_rccl_available(void);
int gccnmf_rccl_unique_id(char* id_bytes);
int gccnmf_rccl_comm_init(const char* id_bytes, int world_size, int rank, void** comm);
int gccnmf_rccl_comm_destroy(void* comm);
int gccnmf_rccl_allreduce(void* comm, float* buf, long count, void* stream);
/* the address of gccnmf_rccl_allreduce as a gccnmf_allreduce_fn (for hosts that cannot take a symbol's address, e.g. ctypes) */
gccnmf_allreduce_fn gccnmf_rccl_allreduce_hook(void);

/* GCC-PHAT angular spectrogram A[tau][t] = sum_f Re(C[f,t] exp(-2j pi f tau)) as a real GEMM
 * [cos;sin]^T . [Re C; Im C], plus its time mean.  Replaces getAngularSpectrogram
 * (gccNMFFunctions.py:85-92) and mean(.., axis=-1) (runGCCNMF.py:46).
 *   trig   [2][Fp][Dp] float32: cos(2 pi f tau) / sin(2 pi f tau), Dp = round_up(D,64), zero padded
 *   ang    [batch][Dp][Tp] float32 out,  mean_ang [batch][Dp] float64 out (may be NULL)
 *
 * GCC-NONLIN (the reference's settings gccPHATNLEnabled / gccPHATNLAlpha, gccNMF/realtime/config.py:42-43,53-54, handed on in
 * runRealtimeGCCNMF.py:101 and gccNMFInterface.py:64-65 and never evaluated there; Blandin, Ozerov & Vincent 2012):
 *     A[tau][t] = sum_f 1 - tanh(alpha sqrt(max(0, 1 - Re(C[f,t] exp(-2j pi f tau)))))
 * is a mode of this call, not an entry point of its own (the header does not grow; gccnmf_reconstruct carries its mode the same
 * way): the float32 bits of alpha ride in the upper halves of D and batch,
 *     gccnmf_angular_spectrogram(CC, trig, F, T, GCCNMF_ANGULAR_NL_D(D, bits), GCCNMF_ANGULAR_NL_BATCH(batch, bits), ang, mean_ang, stream)
 * with D and batch below 65536.  Both halves zero = PHAT: every call that existed before computes what it computed.  Same buffers,
 * pitches and padding rules (only tau < D, t < T is written), same mean_ang; the nonlinearity sits inside the sum, so this is a
 * register-tiled VALU kernel (csrc/angular_nl.hip), every output summed in an order that depends on F alone (a file alone and in a
 * batch agree bit for bit).  A zero coherence bin adds 1 - tanh(alpha) to every tau.  GCCNMF_ERR_ARG: alpha <= 0, NaN, Inf or
 * subnormal, and whatever the PHAT form rejects. */
#define GCCNMF_ANGULAR_NL_D(D, alpha_bits) ((int)((unsigned)(D) | ((unsigned)(alpha_bits) & 0xffff0000u)))
#define GCCNMF_ANGULAR_NL_BATCH(batch, alpha_bits) ((int)((unsigned)(batch) | ((unsigned)(alpha_bits) << 16)))
int gccnmf_angular_spectrogram(const float* CC, const float* trig, int F, int T, int D, int batch, float* ang,
                               double* mean_ang, void* stream);

/* Peak picking on the mean angular spectrum: strict local maxima (edges excluded), keep the
 * S largest (the larger index among equal heights), ascending order.  Replaces estimateTargetTDOAIndexesFromAngularSpectrum
 * (gccNMFFunctions.py:94-116) for numSources > 0.
 *   tdoa_idx [batch][S] int32 out; status [batch] int32 out (0 ok, 1 = fewer than S peaks)
 *
 * Time-varying TDOA tracks (talkers who move; the offline twin of the streaming multi-target localisation) are a mode of this call, not
 * an entry point of its own: pass GCCNMF_PEAKS_TRACKS(S, L) as S -- bit 8 and the window length L (frames, 1 <= L < 2^22) above the low
 * byte of S -- and the call reads the angular SPECTROGRAM instead of its time mean:
 *     gccnmf_pick_tdoa_peaks((const double*)ang, D, T, GCCNMF_PEAKS_TRACKS(S, L), batch, tracks, status, stream)
 *   ang    [batch][round_up(D,64)][round_up(T,64)] float32, as gccnmf_angular_spectrogram wrote it (either form); the pitches follow
 *          from D and T, so the Dp argument carries T (1 <= T < 2^21) in this mode
 *   tracks [batch][S][Tp] int32 out, 16-byte aligned: the peak rule above applied, per frame t, to the mean of ang over the centred
 *          window [max(0, t - L/2), min(T, t - L/2 + L)) -- float64, frames added in ascending order, divided by the window's own
 *          length: a value depends on (t, L, T) and the file only, a file alone and in any batch give the same tracks bit for bit
 *   status [batch][Tp] int32 out: 0 = the frame had S peaks; 1 = it had fewer and holds the set of the last complete frame before it
 *          (frames in front of the first complete frame: that frame's set); 3 = no frame of the file had S peaks (every frame of
 *          the file; tracks -1) -- the condition the whole-file form reports as status 1
 *   Target i of a frame is its i-th peak from the left, as in the whole-file form: two talkers whose directions cross swap outputs.
 *   L >= 2T - 1 makes every window the whole file (constant tracks).  Frames >= T are not written.  1 <= S <= 255, batch <= 65535.
 * Nothing above the low byte of S = the whole-file form: every call that existed before computes what it computed (S <= 255, the
 * score stage's limit).  GCCNMF_ERR_ARG: bits above the low byte without bit 8, L = 0, a negative S, and what the plain form rejects.
 *
 * Counting the talkers (numSources = 'auto'; the reference declares it -- KMeans(n_clusters=2) on the peak heights, keep the upper
 * cluster, gccNMFFunctions.py:105-110 -- and cannot run it) is a mode of this call too: pass GCCNMF_PEAKS_COUNT(Smax) as S -- bit 30
 * alone above the low byte, 1 <= Smax <= 255; bit 30 belongs to L wherever bit 8 is set -- and every file keeps as many peaks as it
 * has talkers, Smax at the most:
 *     gccnmf_pick_tdoa_peaks(mean_ang, D, Dp, GCCNMF_PEAKS_COUNT(Smax), batch, tdoa_idx, status, stream)
 *   The peaks are those of the plain form, P of them, ordered by height descending (the larger index first among equal heights).  With
 *   c_j the sum of the j highest, added in that order, the count is the smallest j in [1, P) that maximises
 *       b_j = c_j * c_j / j + (c_P - c_j) * (c_P - c_j) / (P - j)
 *   -- the exact two-cluster k-means optimum of the heights (in one dimension a threshold on the sorted values), the upper cluster
 *   kept -- every product, quotient and sum a float64 operation rounded on its own.  P = 1 counts 1.
 *   tdoa_idx [batch][Smax] int32 out: the counted peaks in ascending index order, then -1 (what GCCNMF_SCORES_COUNTED reads)
 *   status   [batch] int32 out: 0 = counted; 1 = no peak, or two or more whose heights have no finite sum (count 0, every index -1); 2 = more
 *            than Smax counted, the Smax highest kept
 *   mean_ang, D (3 to 4096), Dp >= D as in the plain form; one workgroup per file, a file's result depends on its own row only.
 *   GCCNMF_ERR_ARG: Smax = 0, any other bit beside bit 30 above the low byte, and what the plain form rejects. */
#define GCCNMF_PEAKS_TRACKS_BIT 0x100
#define GCCNMF_PEAKS_TRACKS(S, L) ((S) | GCCNMF_PEAKS_TRACKS_BIT | ((L) << 9))
#define GCCNMF_PEAKS_COUNT_BIT (1 << 30)
#define GCCNMF_PEAKS_COUNT(Smax) ((Smax) | GCCNMF_PEAKS_COUNT_BIT)
int gccnmf_pick_tdoa_peaks(const double* mean_ang, int D, int Dp, int S, int batch, int* tdoa_idx, int* status,
                           void* stream);

/* Per-target GCC-NMF scores G_i[k,t] = Re sum_f W[f,k] C[f,t] exp(-2j pi f tau_i) and the
 * arg-max-over-targets coefficient mask (first index wins ties, NaN ignored).  Replaces
 * getTargetTDOAGCCNMFs (gccNMFFunctions.py:118-135) + getTargetCoefficientMasks (:137-143).
 *   tdoa_idx [batch][S] device int32 (from gccnmf_pick_tdoa_peaks or uploaded)
 *   scores   [batch][Kp][S*Tp] float32 out (target i occupies columns i*Tp .. i*Tp+T-1)
 *   argmax   [batch][Kp][Tp] uint8 out;  workspace: gccnmf_scores_workspace_floats floats
 * Per-frame target directions: pass S | GCCNMF_SCORES_TRACKS (the mode rides above the low byte of S, like GCCNMF_RECONSTRUCT_RATIO;
 * any other bit there: GCCNMF_ERR_ARG) and tdoa_idx is [batch][S][Tp] int32, 16-byte aligned -- one index per (target, frame), as the
 * tracks mode of gccnmf_pick_tdoa_peaks writes them: G_i[k,t] = Re sum_f W[f,k] C[f,t] exp(-2j pi f tau_{i,t}).  Only the steering
 * table lookup in front of the GEMM changes (indexes are clamped to [0, D) as before); constant tracks give the bits of the plain form.
 * Files with different numbers of targets: pass S | GCCNMF_SCORES_COUNTED (S = the most any file has; not together with
 * GCCNMF_SCORES_TRACKS or the enhancement modes: GCCNMF_ERR_ARG) and tdoa_idx [batch][S] is read as the count mode of
 * gccnmf_pick_tdoa_peaks writes it: an index >= 0 is a target as before (clamped to [0, D)), an index < 0 a target the file does not
 * have.  The scores of an absent target are quiet NaN for every k < K, t < T (its steering column is NaN; padded positions are what
 * they are for a present target), so the arg-max, which ignores NaN, never gives it an atom.  With every index non-negative the
 * scores and the arg-max are bit for bit those of the plain form at the same S.
 *
 * Offline speech enhancement (one talker against noise: every atom of every frame goes to the talker or to the noise by the atom's OWN
 * TDOA, gccNMF/realtime/gccNMFProcessor.py:254,:259-265) is two further modes of this call, not entry points of their own
 * (csrc/atom_tdoa.hip); the macros below spell the two calls out.
 *
 * GCCNMF_ATOM_TDOA_INDEXES -- S = GCCNMF_SCORES_ATOM_TDOA, nothing in the low byte -- scores every atom against the WHOLE grid,
 *     score[k,d,t] = sum_f W[f,k] (Cr[f,t] cos[f,d] + Ci[f,t] sin[f,d])                                   (gccNMFProcessor.py:254)
 * and keeps only the arg-max over d < D (:259): first index wins an exact tie, NaN scores are ignored, an all-NaN column gives 0.
 *   CC, trig, W  as above (W [batch][Fp][Kp]); tdoa_idx and workspace are not read and may be NULL (there is no workspace: no
 *                (K, D, T) or (F, D, T) array exists anywhere, the scores live in matrix-core accumulators)
 *   atom_tdoa    [batch][Kp][Tp] uint16 out, 4-byte aligned, passed as `argmax`; every element is written, padded positions as 0
 *   atom_score   [batch][Kp][Tp] float32 out or NULL, 8-byte aligned, passed as `scores`: the winning score (NaN where the column had
 *                no number, 0 in padded positions)
 *   The f sum of one (k, d, t) is one f32 fma chain in ascending f over a = fma(Cr, cos, Ci * sin) -- exact-f32 MFMA -- whatever the
 *   batch, the file's place in it or the grid: a file's image is bit-identical alone and in any batch.
 *   GCCNMF_ERR_UNSUPPORTED: D > 1024 (the streaming limit), batch > 65535, T > 2^19.  GCCNMF_ERR_ARG: a null CC / trig / W /
 *   atom_tdoa, a non-positive size, anything in the low byte of S.  All checks come before the first HIP call.
 *
 * GCCNMF_ENHANCEMENT_MASKS -- S = GCCNMF_SCORES_ENHANCEMENT_MASKS | window [| GCCNMF_SCORES_TRACKS] -- turns the index image into the
 * talker's and the noise's coefficient masks around a target index; with i = atom_tdoa[k,t] and dist = |i - target| in float32:
 *     window = 0 (TARGET_MODE_BOXCAR, :263):            m = dist < eps
 *     window = 1 (TARGET_MODE_WINDOW_FUNCTION, :265):   m = expf(-powf(dist / eps, beta)) / (1 + nf) + nf       (not clamped)
 *   atom_tdoa [batch][Kp][Tp] uint16, passed as `CC`;  target [batch] int32, or with GCCNMF_SCORES_TRACKS [batch][Tp] int32 (one per
 *             frame), passed as `tdoa_idx`;  params = {eps, beta, nf}: three floats in HOST memory, read before the call returns,
 *             passed as `trig` (eps > 0, beta > 0, nf >= 0, all finite, else GCCNMF_ERR_ARG)
 *   image     [batch][Kp][Tp] uint8 out or NULL, passed as `argmax`: 0 where dist < eps (talker), else 1 (noise) -- gccnmf_reconstruct
 *             takes it as its one-hot arg-max image with S = 2
 *   masks     [batch][2][Kp][Tp] float32 out or NULL, passed as `scores`: (m, 1 - m) -- gccnmf_reconstruct's `masks` with S = 2
 *   Padded positions of both outputs are written as 0.  W, F, D and workspace are not read.  GCCNMF_ERR_ARG: both outputs NULL, a
 *   null input, a non-positive T / K / batch, window > 1. */
#define GCCNMF_SCORES_TRACKS 0x100
#define GCCNMF_SCORES_ATOM_TDOA 0x200
#define GCCNMF_SCORES_ENHANCEMENT_MASKS 0x400
#define GCCNMF_SCORES_COUNTED 0x800
#define GCCNMF_ATOM_TDOA_INDEXES(CC, trig, W, F, T, K, D, batch, atom_tdoa, atom_score, stream)                                          \
    gccnmf_target_scores_masks(CC, trig, 0, W, F, T, K, D, GCCNMF_SCORES_ATOM_TDOA, batch, 0, atom_score, (unsigned char*)(atom_tdoa), stream)
#define GCCNMF_ENHANCEMENT_MASKS(atom_tdoa, target, per_frame, window, params, T, K, batch, image, masks, stream)                        \
    gccnmf_target_scores_masks((const float*)(atom_tdoa), params, target, 0, 0, T, K, 0,                                                 \
                               GCCNMF_SCORES_ENHANCEMENT_MASKS | (window) | ((per_frame) ? GCCNMF_SCORES_TRACKS : 0), batch, 0, masks,   \
                               image, stream)
long gccnmf_scores_workspace_floats(int F, int T, int S, int batch);
int gccnmf_target_scores_masks(const float* CC, const float* trig, const int* tdoa_idx, const float* W, int F,
                               int T, int K, int D, int S, int batch, float* workspace, float* scores,
                               unsigned char* argmax, void* stream);

/* The arg-max half of the call above on its own (host-array getTargetCoefficientMasks,
 * gccNMFFunctions.py:137-143): scores [batch][Kp][S*Tp] -> argmax [batch][Kp][Tp]. */
int gccnmf_argmax_targets(const float* scores, int K, int T, int S, int batch, unsigned char* argmax, void* stream);

/* PHAT coherence from an existing spectrogram X [batch][2][Fp][Tp] (runGCCNMF.py:44); the pipeline
 * gets CC from gccnmf_stft_stereo's epilogue instead. */
int gccnmf_coherence(const float* X, int F, int T, int batch, float* CC, void* stream);

/* V = concatenate(abs(X), axis=-1) (runGCCNMF.py:40) from an existing spectrogram X [batch][2][Fp][Tp] -> V [batch][Fp][Np], columns
 * c*T + t; the pipeline gets V from gccnmf_stft_stereo's epilogue instead (same hypotf). */
int gccnmf_magnitude(const float* X, int F, int T, int batch, float* V, void* stream);

/* Masked reconstruction S[i,c] = (W . (H_c * M_i)) * X_c/|X_c|.  Replaces
 * getTargetSpectrogramEstimates (gccNMFFunctions.py:145-151).
 *   the mask is either `argmax` [batch][Kp][Tp] uint8 (one-hot masks, the device pipeline) or, when
 *   `masks` != NULL, arbitrary float masks [batch][S][Kp][Tp] (the reference signature accepts any array)
 *   spec [batch][S*2][Fp][Tp] complex out (index i*2+c); workspace: gccnmf_reconstruct_workspace_floats
 * Ratio-mask (Wiener-like) mode: pass S | GCCNMF_RECONSTRUCT_RATIO (the mode rides above the low byte of S, which the score stage
 * limits to 255 anyway; any other bit above the low byte: GCCNMF_ERR_ARG).  One fused launch (csrc/ratio.hip, the kernel of csrc/ratio_kernel.h), 1 <= S <= 8, else
 * GCCNMF_ERR_UNSUPPORTED; with H_c = H[:, c*T:(c+1)*T]:
 *   num_i[f,t]  = sum_k W[f,k] H_c[k,t] M_i[k,t]                   (f32 fma chain in k order)
 *   den[f,t]    = num_0 + num_1 + ... + num_{S-1}                  one-hot form (`masks` == NULL, M_i = [argmax == i])
 *               = sum_k W[f,k] H_c[k,t]                            soft form (`masks` != NULL)
 *   S[i,c][f,t] = X_c[f,t] * (num_i / den)  if den > 0, else 0 for every i        (IEEE quotient; NaN / Inf in W or H propagate)
 * -- the numerator is the magnitude model of gccNMFFunctions.py:150, the mixture phase of :147-151 comes with X_c itself, and in the
 * one-hot form the targets add up to the mixture, sum_i S[i,c] = X_c, to a few ulp.  In this mode `V` and `workspace` are not read and
 * may be NULL, and every element of spec [batch][S*2][Fp][Tp] is written (rows >= F and frames >= T as zeros).  A file's spec does not
 * depend on the batch it is in.  gccnmf_reconstruct_workspace_floats keeps its meaning (the direct mode's need).
 *
 * Spatial (multichannel Wiener) mode: pass S | GCCNMF_RECONSTRUCT_RATIO and GCCNMF_RECONSTRUCT_SPATIAL_BATCH(batch) as batch (the mode
 * rides in the upper half of batch, like GCCNMF_ANGULAR_NL_BATCH; batch <= 65535).  The ratio-mask stage runs exactly as above -- spec
 * holds its bits -- and a spatial filter (csrc/spatial.hip, two launches) then replaces the estimates in place.  Per file, with
 * S_i,c[f,t] the ratio-mode estimate of target i, channel c, and X[f,t] = (X_0, X_1)^T:
 *   v_i[f,t] = 1/2 (|S_i,0|^2 + |S_i,1|^2)
 *   p_c = sum_t |S_i,c|^2,  q = sum_t S_i,0 conj(S_i,1),  n = (p_0 + p_1) / 2        (frames t < T, float64, an order fixed by T alone)
 *   R_i[f]   = [[p_0, q], [conj q, p_1]] / n  (trace 2);  R_i[f] = I when n = 0
 *   R~_i[f]  = R_i[f] + GCCNMF_SPATIAL_LOADING * I, rounded to float32 once
 *   Sigma[f,t] = sum_j v_j[f,t] R~_j[f]  (ascending j),  y = Sigma^-1 X  (closed 2 x 2 Hermitian inverse),  S'_i[f,t] = v_i[f,t] R~_i[f] y
 *   every target is 0 where sum_j v_j[f,t] = 0 (as for den = 0 above); NaN / Inf in the inputs propagate; rows >= F and frames >= T
 *   are written as zeros.  Sigma, y and S'_i are float32, each product and sum rounded on its own, evaluated on w_j = v_j 2^-e with e
 *   the binary exponent of sum_j v_j: S'_i = w_i R~_i (sum_j w_j R~_j)^-1 X is the same quantity, has the same roundings while every
 *   intermediate of the unscaled form is a normal float32 number, and stays accurate where that form's determinant would underflow (a
 *   nearly silent frame).
 *   The order of the float64 frame sums (p_0, p_1, Re q, Im q here; the four sums of A_i in the EM refinement below), which makes R~ a
 *   function of the row's bits alone: the frames are dealt to 64 lanes; lane l adds its frames 2l, 2l+1, 2l+128, 2l+129, ... (those
 *   below T) one after the other to +0.0, each term formed in float64 from the float32 estimates (|S|^2 = re re + im im: two exact
 *   products, one rounded sum; likewise the two parts of q); the 64 partial sums x[0 .. 63] are then combined in six steps
 *   k = 1, 2, 4, 8, 16, 32 of x[l] <- x[l] + x[l ^ k], every l at once, after which every lane holds the same sum.  Then, in float64,
 *   n = 1/2 (p_0 + p_1), the four quotients by n, + GCCNMF_SPATIAL_LOADING on the diagonal, and the one rounding to float32.
 *   tests/spatial_checks.py restates this order (device_sum); with it a float32 NumPy evaluation equals the device bit for bit.
 * The targets still add up to the mixture (sum_i S'_i = Sigma y = X up to rounding), one target returns it, and swapping the input
 * channels swaps the output channels.  `workspace` holds the covariances, [batch][S][Fp][4] float32 = (R~00, R~11, Re R~01, Im R~01):
 * GCCNMF_RECONSTRUCT_SPATIAL_WORKSPACE_FLOATS(batch, S, Fp) floats, Fp = round_up(F, 16); it must be non-NULL and 16-byte aligned, else
 * GCCNMF_ERR_ARG.  `V` is not read.  A file's spec does not depend on the batch it is in or on its place there.  GCCNMF_ERR_ARG: the
 * spatial bit without GCCNMF_RECONSTRUCT_RATIO, any other bit above the low half of batch (so: a batch above 65535 in any mode).
 *
 * EM refinement of the spatial mode: pass S | GCCNMF_RECONSTRUCT_RATIO | GCCNMF_RECONSTRUCT_SPATIAL_ITERATIONS(n), 1 <= n <= 255 (bits
 * 20-27 of S), with GCCNMF_RECONSTRUCT_SPATIAL_BATCH(batch).  The spatial mode above is step zero of the EM of the local Gaussian model
 * (Duong, Vincent & Gribonval 2010); n iterations of it run in ONE launch (csrc/spatial_em.hip) between the covariance launch, whose
 * bits are unchanged, and the filter launch.  Every (file, bin) row is independent.  Start: v_i and R~_i as above.  Iteration
 * m = 1 ... n, for every bin f < F:
 *   1. for every frame t < T, against the OLD R~, on w_j = v_j 2^-e as above:
 *        Sigma = sum_j v_j R~_j (ascending j),  G_i = v_i R~_i Sigma^-1 (closed 2 x 2 Hermitian inverse),  s_i = G_i X,
 *        C_i = s_i s_i^H + (I - G_i) v_i R~_i,   v'_i = max(0, 1/2 Re tr(R~_i^-1 C_i))   (stored unscaled),
 *        v'_i = 0 for every i where sum_j v_j = 0.
 *      Evaluated as v'_i = w_i v"_i, C_i = w_i C"_i with y = Sigma_w^-1 X, u_i = R~_i y, N_i = sum_{j != i} w_j R~_j (ascending j):
 *        v"_i = 1/2 (w_i Re(y^H u_i) + 2^e tr(Sigma_w^-1 N_i)),   C"_i = w_i u_i u_i^H + 2^e N_i Sigma_w^-1 R~_i
 *      (2 - tr G_i = tr(Sigma_w^-1 N_i) and (I - G_i) R~_i = N_i Sigma_w^-1 R~_i: sums of non-negative parts where the literal
 *      forms cancel), float32, each product and sum rounded on its own.
 *   2. A_i = sum over the frames with v'_i != 0 of C_i / v'_i (= C"_i / v"_i: float32 terms, the real parts of the diagonal and
 *      the (0, 1) element; a NaN power counts), n_i = the number of those frames; the sum is float64, in an order fixed by T alone, as
 *      the covariance launch does it.  R'_i = A_i / n_i, R'_i = I when n_i = 0;  R~'_i = R'_i + GCCNMF_SPATIAL_LOADING * 1/2 tr(R'_i) * I,
 *      rounded to float32 once.  The order is the one stated for the covariance launch above: lane l adds the float32 terms of its
 *      frames 2l, 2l+1, 2l+128, ... to +0.0 in float64 and counts them, a frame whose v'_i is 0 adding nothing and not counting; the
 *      same six-step combination; then A_i / n_i, + GCCNMF_SPATIAL_LOADING * (1/2 (R'00 + R'11)) on the diagonal, one rounding.
 *      No trace renormalisation: only v R~ enters, and the per-frame M-step keeps the trace near 2.
 *   3. v <- v', R~ <- R~'.
 * Output: S'_i = v_i R~_i Sigma^-1 X by the filter above, on the final v and R~; every target 0 where sum_j v_j = 0; rows >= F and
 * frames >= T are zeros; NaN / Inf propagate, and a NaN in one bin of X stays in that bin.  A power that is exactly 0 stays 0 (G_i = 0),
 * so the frames a target skips are fixed by the input.  `workspace`: GCCNMF_RECONSTRUCT_SPATIAL_EM_WORKSPACE_FLOATS(batch, S, Fp, Tp)
 * floats, 16-byte aligned: the covariances [batch][S][Fp][4] (the final R~ on return), then the powers [batch][S][Fp][Tp] float32 (the
 * final v on return, frames < T of rows < F; not touched without the iteration bits).  GCCNMF_ERR_ARG, before any HIP call: the
 * iteration bits without GCCNMF_RECONSTRUCT_RATIO or without the spatial bit of batch; bits 9-19 and 28-31 of S. */
#define GCCNMF_RECONSTRUCT_RATIO 0x100
#define GCCNMF_RECONSTRUCT_SPATIAL_BIT (1 << 16)
#define GCCNMF_RECONSTRUCT_SPATIAL_BATCH(batch) ((batch) | GCCNMF_RECONSTRUCT_SPATIAL_BIT)
#define GCCNMF_RECONSTRUCT_SPATIAL_WORKSPACE_FLOATS(batch, S, Fp) (4L * (batch) * (S) * (Fp))
#define GCCNMF_RECONSTRUCT_SPATIAL_ITERATIONS(n) ((n) << 20)
#define GCCNMF_RECONSTRUCT_SPATIAL_EM_WORKSPACE_FLOATS(batch, S, Fp, Tp) (4L * (batch) * (S) * (Fp) + (long)(batch) * (S) * (Fp) * (Tp))
#define GCCNMF_SPATIAL_LOADING 1e-3
long gccnmf_reconstruct_workspace_floats(int T, int K, int S, int batch);
int gccnmf_reconstruct(const float* W, const float* H, const unsigned char* argmax, const float* masks,
                       const float* X, const float* V, int F, int T, int K, int S, int batch, float* workspace,
                       float* spec, void* stream);

/* Inverse STFT + overlap-add + centre trim + gain for `nsig` spectrograms per file.  Replaces
 * getTargetSignalEstimates (gccNMFFunctions.py:153-163 -> librosaSTFT.py:241-286, center=True).
 *   spec   [batch][nsig][Fp][Tp] complex (nsig must be even: signals are inverse-transformed in pairs)
 *   window [n_fft] synthesis window; twiddle as for the forward transform
 *   frames [batch][nsig][T][n_fft] float32 scratch, or NULL: inverse transform and overlap-add fused in one pass (same accumulation
 *          order, no frame buffer; needs n_fft + 3*hop <= 2048 and hop <= n_fft, else GCCNMF_ERR_UNSUPPORTED: with hop > n_fft there are
 *          samples between consecutive frames that no frame touches, which only the two-kernel form writes -- as 0)
 *   center != 0 trims n_fft/2 samples at both ends (the reference path), 0 keeps all n_fft + hop*(T-1)
 *   y      [batch][nsig][L] float32 out, L = n_fft + hop*(T-1) - (center ? n_fft : 0); every sample is written, and where both forms
 *          accept a call they give the same bits.  L < 1 (T = 1 with center != 0): GCCNMF_ERR_ARG from both forms, like every other
 *          argument error before anything is launched */
int gccnmf_istft_ola(const float* spec, int nsig, int n_fft, int hop, int T, int batch, const float* window,
                     const float* twiddle, float gain, int center, float* frames, float* y, void* stream);

/* The overlap-add half of the call above on its own, for ONE file whose frame sequence is `halo` frames of `prev` [nsig][halo][n_fft]
 * (the previous time shard's last frames; NULL with halo = 0: this file's frames alone) followed by the T frames of `frames`
 * [nsig][T][n_fft] (windowed time frames) -- no concatenated copy of the two -> y [nsig][L] = samples first_sample .. first_sample+L-1
 * of the overlap-added stream, frames added in ascending order (librosaSTFT.py:275-281), times gain.  Used by the time-sharded
 * single-mixture mode, where a shard's first samples need the previous shard's last n_fft/hop - 1 frames. */
int gccnmf_ola_frames_halo(const float* prev, int halo, const float* frames, int nsig, int n_fft, int hop, int T, int first_sample, int L,
                           float gain, float* y, void* stream);

/* Streaming (real-time) GCC-NMF: one block of `blockSize` new stereo samples per call, Tc = blockSize/hopSize analysis
 * windows.  Replaces GCCNMFProcessor.processFrames (gccNMF/realtime/gccNMFProcessor.py:201-270, a Theano graph in the
 * reference) together with OverlapAddProcessor.processFrames (gccNMF/realtime/utils.py:99-116) and the gccPHAT history /
 * online localisation (:214-222, utils.py:34-70).  Six launches on `stream`, no host synchronisation.
 * Sizes: ANY even windowSize in [4, 4096] and any blockSize, like the reference (numpy.fft.rfft / irfft of any length,
 * gccNMFProcessor.py:202,:231; buffers of any size, realtime/utils.py:72-97).  Powers of two from 64 up run the radix-2 LDS transform
 * (`twiddle` = windowSize/2 complex values exp(-2j pi k / N), as for gccnmf_stft_stereo); every other even size is evaluated as the
 * direct sum against `twiddle` = the windowSize-entry table (cos, sin)(2 pi k / N) (csrc/rt.hip: rt_frames_dft / rt_synth_dft).
 * The only requirement left: 8*blockSize >= one block's windows (the reference's 8-block buffers) -> else GCCNMF_ERR_UNSUPPORTED.
 *   block_in / block_out [2][blockSize]            new samples in, the block two blocks old out (utils.py:116)
 *   in_ring / out_ring   [2][8*blockSize]          state: the reference's 8-block buffers
 *   X, Y [2][F][Tc] complex, C [F][Tc] complex     rfft (not conjugated), masked spectrogram, PHAT coherence
 *   HMask [Kp][Tc], argmaxTDOA [Kp][Tc] (or NULL), tfMask [F][Tc], gccphat [D][Tc] (or NULL)
 *   hist [D][numTDOAHistory] + hist_pos [1]        state: gccPHAT history ring
 *   target [4]                                     state: {targetTDOAIndex, epsilon, beta, noiseFloor}; index rewritten by
 *                                                  the localisation for the NEXT block
 *   W [F][Kp]; cosT / sinT [F][Dp] = Re / -Im of exp(-2j pi f tau) (Dp = round_up(D,32), zero padded), float32 grids as
 *   in :245-248; window [windowSize] = sqrt(hamming) (:186); twiddle as for gccnmf_stft_stereo
 *   target_mode 0 = boxcar (:263), 2 = window function (:265)
 *   frames_mode 1 = processFrames alone: in_ring holds windowed-sample frames [2][Tc][windowSize], out_ring receives the
 *   processed frames, no shift / overlap-add. */
int gccnmf_rt_process_block(const float* block_in, float* block_out, float* in_ring, float* out_ring, float* X, float* Y,
                            float* C, float* HMask, int* argmaxTDOA, float* tfMask, float* hist, int* hist_pos, float* target,
                            float* gccphat, const float* W, const float* cosT, const float* sinT, const float* window,
                            const float* twiddle, int windowSize, int hopSize, int blockSize, int K, int Kp, int D, int Dp,
                            int numTDOAHistory, int target_mode, int separation_enabled, int localization_enabled,
                            int localization_window, int frames_mode, void* stream);

/* Low-latency extension of the call above (BASELINE config 5; README.md:74-78 -- the notebooks that implemented it are not in the
 * reference checkout, so this part has no reference code to be pinned on):
 *   synthesis_window [windowSize]  separate synthesis window (asymmetric analysis / synthesis pairs: long analysis window for
 *                                  spectral resolution, short synthesis window at the end of the frame for latency)
 *   numHUpdates > 0                per-frame coefficient inference: that many KL-NMF H updates with W fixed
 *                                  (gccNMFFunctions.py:76), h0 = 1, per channel; the mask becomes W.(h*HMask) / W.h per channel,
 *                                  tfMask is then [2][F][Tc].  colsumW [Kp] = sum_f W, Hcoef [Kp][2*Tc], Rv [F][2*Tc] scratch.
 *                                  numHUpdates = 0 is exactly gccnmf_rt_process_block (h = 1).  A channel that is silent in a
 *                                  frame (|X| = 0 in every bin) gets no coefficients: its Rv, Hcoef, mask and Y are 0 (W.h = 0 is
 *                                  answered with 0, not 0 / 0: a NaN frame would stay in the overlap-add buffer for eight blocks).
 *                                  Columns K..Kp-1 of W may hold anything: no kernel of the call reads them into a result.
 *   frames_mode bits               1 = frames mode; 2 = everything but the localisation kernel; 4 = only the localisation kernel
 *                                  (2 then 4 on the same stream = one call; lets a host fetch block_out before the tracking update)
 *                                  8 = stream bank: S = (bits 8..19) + 1 independent streams of this configuration, advanced
 *                                  together in the same launches (S <= 4096).  Every per-stream buffer holds S consecutive
 *                                  single-stream images (block_in / block_out, in_ring / out_ring, X, Y, C, HMask, argmaxTDOA,
 *                                  tfMask as [S][2][F][Tc] whatever numHUpdates, gccphat, hist, Hcoef, Rv); hist_pos is [S];
 *                                  target is [S][8] = {index, epsilon, beta, noiseFloor, separation, localisation, nlAlpha, 0}.  A
 *                                  stream separates (localises) when separation_enabled (localization_enabled) AND its row word
 *                                  4 (5) are non-zero; with separation_enabled = 0 no mask kernel is launched.  Stream s computes
 *                                  bit for bit what a single-stream call on its images computes.  Bits 2 and 4 work as above.
 *                                  GCCNMF_ERR_ARG: 8 together with 1 (frames mode), bits 8..19 without 8, any bit above 24.
 *                                  1 << 20 = multi-target layout (separation of N = (bits 21..23) + 1 talkers, N <= 8; needs
 *                                  target_mode 1 = TARGET_MODE_MULTIPLE).  The target row is 16 floats per stream (single-stream
 *                                  call and bank): words 0..7 as above (0..3 unused), words 8..8+N-1 = target TDOA indexes
 *                                  tau_0..tau_N-1 in [0, D), rewritten by the localisation (the N largest strict local maxima of
 *                                  the window mean, ascending; unchanged with fewer than N peaks).  Atom k of frame t goes to the
 *                                  target whose GCC-NMF score at tau_i is largest (one-hot, first index on ties, NaN ignored, all
 *                                  NaN -> target 0).  Per-stream images: Y, tfMask [N][2][F][Tc]; HMask [N][Kp][Tc] (0 / 1);
 *                                  out_ring [N][2][8*blockSize] (frames mode: [N][2][Tc][windowSize]); block_out [N][2][blockSize];
 *                                  every other buffer as above.  With separation off every output is the unmasked mixture.
 *                                  GCCNMF_ERR_ARG: 1 << 20 with target_mode != 1, bits 21..23 without 1 << 20.  Without bit 20 a
 *                                  call computes what it computed before the layout existed (target_mode 1 = window function).
 *                                  GCC-NONLIN localisation (gccPHATNLEnabled / gccPHATNLAlpha, config.py:42-43): word 6 of a stream's
 *                                  target row is alpha, 0 = plain PHAT (a value that is not a positive normal float is read as 0).
 *                                  With alpha > 0 the localisation kernel accumulates 1 - tanh(alpha sqrt(max(0, 1 - term))) instead
 *                                  of each term of gccphat = nanmean_f Re(C e^{-jwt}); NaN terms are skipped as before, and the
 *                                  history ring, window mean and arg-max / peak rule are unchanged.  The GCC-NMF scores stay PHAT.
 *                                  The row word was chosen over a new entry point or argument: it gives per-stream control in the
 *                                  bank and leaves both signatures alone.  The bank and multi-target rows always have word 6; the
 *                                  single-stream row is 4 words unless 1 << 24 says it has 8 (words 4, 5, 7 unused there).
 *                                  GCCNMF_ERR_ARG: 1 << 24 together with 8 or 1 << 20, any bit above 24.
 *   separation_enabled bit 1       GCCNMF_RT_SEPARATION_SPATIAL (callers pass 3): the online spatial (multichannel Wiener) filter, one
 *                                  more launch (csrc/rt_spatial.hip) between the mask and the synthesis kernel, which rewrites Y in place.
 *                                  It is the local Gaussian model of gccnmf_reconstruct's spatial mode with a recursive covariance in
 *                                  place of the sum over the file.  Per stream and bin f, components j < NC, frames in ascending order:
 *                                    multi-target layout: NC = N, E_j,c = Y_j,c as the mask kernel wrote it; single-target layouts:
 *                                    NC = 2, E_0 = Y (the talker), E_1 = X - E_0 (the residual; component-wise, float32)
 *                                    c_j = (|E_j,0|^2, |E_j,1|^2, Re E_j,0 conj E_j,1, Im E_j,0 conj E_j,1),  v_j = 1/2 (c_j.p0 + c_j.p1)
 *                                    P_j <- a P_j + b c_j, b = 1 / tau, a = 1 - b, BEFORE use, and only when X and every c_j of the
 *                                    (bin, frame) are finite: otherwise the bin's state stays bit for bit (a NaN block does not
 *                                    poison a stream; NaN / Inf still propagate into that frame's Y)
 *                                    R_j = P_j / n_j, n_j = 1/2 (P_j.p0 + P_j.p1), R_j = I when n_j < 2^-126 (nothing averaged yet);
 *                                    R~_j = R_j + GCCNMF_SPATIAL_LOADING I;  Sigma = sum_j v_j R~_j, y = Sigma^-1 X, Y'_j = v_j R~_j y,
 *                                    0 where sum_j v_j = 0 -- float32, the offline filter's arithmetic (and its power-of-two scaling
 *                                    of the v_j) statement for statement; 1 / tau and 1 / n_j are one IEEE division each
 *                                    written: Y_j <- Y'_j for all j (multi-target), Y <- Y'_0 (single-target)
 *                                  So the N outputs of the multi-target layout add up to X, N = 1 returns X, swapping the input channels
 *                                  swaps the output channels, tau = 1 has no memory, and a call of Tc frames equals Tc calls of one.
 *                                  Per stream: word 7 of the target row is tau in frames; a finite float >= 1 switches the stream's
 *                                  filter on, anything else reads as off.  A stream whose separation is off (row word 4 in the bank,
 *                                  or separation_enabled = 0) skips the stage and leaves its state alone.  The 4-word single-stream
 *                                  row has no word 7: the bit there needs 1 << 24 (GCCNMF_ERR_ARG otherwise, before any launch).
 *                                  State: behind the S history images of `hist` -- the call's other persistent statistic that a reset
 *                                  clears -- starting at float GCCNMF_RT_SPATIAL_STATE_OFFSET(S, D, numTDOAHistory) (the first multiple
 *                                  of 4), [S][NC][F][4] float32 = (p0, p1, Re q, Im q): GCCNMF_RT_SPATIAL_STATE_FLOATS(S, NC, F) floats;
 *                                  `hist` must then be 16-byte aligned (GCCNMF_ERR_ARG).  All zeros = a fresh stream: its first
 *                                  frame sees its own rank-1 covariance plus the loading, and the trace normalisation makes a bias
 *                                  correction of the zero start unnecessary.  The localisation-only call (bit 4 of frames_mode) does
 *                                  not touch the state.  Without bit 1 a call computes what it computed before the filter existed,
 *                                  whatever word 7 holds, and `hist` needs no more than its S images.
 *   out_delay_blocks               which finished block is handed out: 2 = the reference (utils.py:116); 1 is complete when
 *                                  the synthesis window spans at most two hops */
#define GCCNMF_RT_SEPARATION_SPATIAL 2
#define GCCNMF_RT_SPATIAL_STATE_OFFSET(S, D, Lh) ((((long)(S) * (D) * (Lh) + 3) / 4) * 4)
#define GCCNMF_RT_SPATIAL_STATE_FLOATS(S, NC, F) (4L * (S) * (NC) * (F))
int gccnmf_rt_process_block_ll(const float* block_in, float* block_out, float* in_ring, float* out_ring, float* X, float* Y, float* C,
                               float* HMask, int* argmaxTDOA, float* tfMask, float* hist, int* hist_pos, float* target,
                               float* gccphat, const float* W, const float* cosT, const float* sinT, const float* window,
                               const float* synthesis_window, const float* twiddle, const float* colsumW, float* Hcoef, float* Rv,
                               int windowSize, int hopSize, int blockSize, int K, int Kp, int D, int Dp, int numTDOAHistory,
                               int target_mode, int separation_enabled, int localization_enabled, int localization_window,
                               int frames_mode, int numHUpdates, int out_delay_blocks, void* stream);

#ifdef GCCNMF_EXPERIMENTS      /* libgccnmf_hip_exp.so (make EXPERIMENTS=1): measurement tooling of the lab build */
/* Debug: per-workgroup timeline of the LDS-DMA GEMM launches (device buffer of 8 x int64 per workgroup: s_memrealtime
 * [100 MHz] at entry (slots 0 and 1), after the main loop, after the epilogue; [4] = xcc_id<<16 | HW_ID[15:0]).
 * Recorded for launches of at most `blocks` workgroups while buf != NULL (scripts/kbench.py --trace). */
int gccnmf_debug_set_trace(long long* buf, int blocks);

/* Diagnostics: a pure v_mfma_f32_32x32x2_f32 loop (blocks x 4 waves x iters x 8 instructions, 2*32*32*2 flop each):
 * the matrix-pipe rate this box sustains, quoted next to the roofline fractions. */
int gccnmf_debug_mfma_peak(float* scratch, int blocks, int iters, void* stream);
#endif

/* Latency-path GEMM with the KL-NMF element-wise work fused (csrc/direct.hip): what gccnmf_klnmf runs for ONE mixture alone
 * (performKLNMF(V (513, 1244), 1024, 100, 0) is four of these + the W update per iteration), exported so that it can be tested
 * and timed in isolation.
 *     C[m][n] = sum_r (bscale[r] *) A[r][m] * B[r][n]        r < Kd, m < M, n < N      (bscale: epilogue 1 only, else NULL)
 * BOTH operands are reduction-major: one reduction index per row (pitches lda / ldb, multiples of 4), the output index contiguous
 * -- rows r < round_up(Kd, 16) must be addressable, and zero beyond Kd in at least one operand.  Every pointer is device memory;
 * per-file strides (s*) are in floats.  epilogue (numpy.dot / element-wise lines of gccNMFFunctions.py:76-77):
 *   0 STORE  C = acc;  optional rowsumB[n] = sum_r B[r][n];
 *   1 DIV    C = E0 / acc                                   (E0 has pitch lde0)
 *   2 DIVT   Ct[n][m] = E0[m][n] / acc                      (transposed output only)
 *   3 UPDH   C = (C * E1[m]) * ((acc + ktailA[m] * ktailB[n]) / (E2[m] + alpha + eps)), also stored transposed into Ct
 * tailA != NULL adds output row `tail_row` = sum_r tailA[r] * B[r][n], computed on the VALU (F = 513 = 16 * 32 + 1), with the
 * epilogue applied (it goes to C, and to Ct as well for DIVT).  Nothing outside the M x N corner (plus the tail row) is written,
 * except zeros inside a 4-float group that straddles it.  tile: 0 = chosen by the library, 1..8 = a fixed tile (experiments).
 * The trailing six fields are filled in by the library. */
typedef struct gccnmf_direct_gemm {
    const float* A;
    const float* B;
    long sA, sB;
    int lda, ldb;
    int M, N, Kd, batch;
    const float* bscale;
    long s_bscale;
    const float* tailA;
    long s_tailA;
    int tail_row;
    float* rowsumB;
    long s_rowsumB;
    float* C;
    long sC;
    int ldc;
    float* Ct;
    long sCt;
    int ldct;
    const float* E0;
    long sE0;
    int lde0;
    const float* E1;
    long sE1;
    const float* E2;
    long sE2;
    const float* ktailA;
    const float* ktailB;
    long s_ktailA, s_ktailB;
    float alpha, eps;
    int tiles_m, tiles_n, xc, sm, sn;
    long long* trace;          /* library-filled: per-workgroup timeline while gccnmf_debug_set_trace is armed */
} gccnmf_direct_gemm;
int gccnmf_gemm_direct(const gccnmf_direct_gemm* desc, int epilogue, int tile, void* stream);

/* Diagnostics (tests only, no device needed): the work lists a throughput-tile launch (csrc/gemm_dma.h) would use for an M x N output
 * over `batch` files under the current tuning -- the SAME tile decode the kernel runs, executed on the host.
 *   plan  [8]: lists, wide tiles per list, ragged narrow tiles per list, split, rag, tiles_m, tiles_n, items of the classic grid
 *   items [max_items][6]: list, ticket, file, row tile, first column, column blocks (2 = 512 x 64, 1 = a narrow 512 x 32 item)
 *   narrow_capable: bit 0 = the kernel instantiation carries the narrow loop, bit 1 = the whole-file lists of chained launches (list x =
 *   files x, x + 8, ..., each file's wide tiles followed by its ragged items; plan[1] = items of the longest list)
 * Returns the number of items (all lists), -1 on bad arguments. */
int gccnmf_debug_gemm_plan(int M, int N, int batch, int xcd_affine, int concurrent, int narrow_capable, int* plan, int* items, int max_items);

/* Diagnostics (tests only): run one MFMA GEMM configuration in isolation.
 * layout bits: 1 = A reduction-contiguous, 2 = B reduction-contiguous, 4 = VALU tail row, 8 = <1,4> wave grid,
 * 16 = last reduction index as a rank-1 epilogue term (non-KC operands). */
int gccnmf_debug_gemm(const float* A, const float* B, float* C, int M, int N, int Kd, int lda, int ldb, int ldc,
                      int a_clamp, int b_clamp, int layout, int batch, long sA, long sB, long sC,
                      const float* bscale, float* rowsumB, void* stream);

#ifdef __cplusplus
}
#endif
#endif
