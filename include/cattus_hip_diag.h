/*
 * cattus_hip_diag.h -- diagnostic entry point of libcattus_hip.so.  NOT part of the drop-in boundary (cattus_hip.h): a Cattus
 * host never calls it.  It exists so that the equality tests and the A/B timing scripts can force a code path that
 * cattus_hip_create would not choose, without the library reading switches from the process environment.
 */
#ifndef CATTUS_HIP_DIAG_H
#define CATTUS_HIP_DIAG_H

#include "cattus_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cattus_hip_create with a list of switches "KEY=VALUE;KEY=VALUE" (NULL or "" = none = cattus_hip_create).  Unknown keys are
 * refused (CATTUS_E_INVALID).  Every switch selects among kernels whose per-leaf results the tests assert to be bit-identical,
 * or a memory plan; none changes what a leaf evaluates to:
 *   CATTUS_TOWER64=0        networks of <= 64 filters: per-layer launches instead of the resident tower
 *   CATTUS_T64_CH=2|4, CATTUS_T64_LS=0, CATTUS_T64S_SHAPE=1|2, CATTUS_T64S_HEADS=0   workgroup shapes of the resident towers
 *   CATTUS_SPLIT_W=0        f16x2 direct form: weights through the LDS ring (conv3x3_split_kernel) instead of the register ring
 *   CATTUS_CONV_CB=1|2, CATTUS_CONV_PBW=1|2   tile shapes of the per-layer conv kernels
 *   CATTUS_FUSED_STEM=0     every dtype: the plane pack as its own launch in front of the stem, which then runs as an ordinary layer (what
 *                           a network of more than 32 planes runs anyway; f16x2: stem input channels padded to 64 instead of 32)
 *   CATTUS_FORCE_GENERIC=1  the one-thread-per-output f32 path (a second checker of the MFMA kernels)
 *   CATTUS_WINO_KERNEL=k16|k4   Winograd form: the 16-frequencies-per-wave kernel (conv3x3_wino_kernel) or the 4-frequencies x
 *                               2x2-blocks one (conv3x3_wino4_kernel / tower_wino4_kernel); same bits (an eight-wave kernel, two waves
 *                               per SIMD, was measured slower than both and removed: DESIGN.md, K1w8)
 *   CATTUS_WINO_PERSIST=0   the Winograd tower as per-layer launches instead of one launch (tower_wino4_kernel); CATTUS_WINO_SPIN=<n>:
 *                           polls a hand-off wait of that launch may take before it gives up (a launch that gave up is run again,
 *                           per layer: the tests set 1 to walk that path)
 *   CATTUS_WINO_INPLACE=0, CATTUS_ARENA=0     memory plan of the Winograd tower (a third activation buffer; separate allocations)
 *   CATTUS_SPLITK_WAYS=1|2|4|8   tower_form DIRECT_SPLITK: the number of waves a layer's K walk is divided over, instead of the rule's (8 from
 *                           256 filters on, 4 below; never more than there are 32-channel chunks).  THIS ONE CHANGES THE SUMMATION ORDER and with
 *                           it the bits (tests and A/B timing only); 1 gives tower_form DIRECT's bits
 * One switch does change what a leaf evaluates to, and exists to show why its default is what it is:
 *   CATTUS_STREAM_SHIFT=0   the f16 / f16x2 towers carry the residual stream at its own size, however small (see below) */
int cattus_hip_create_diag(const void* weights, size_t nbytes, const cattus_eval_config* cfg, const char* switches, cattus_eval** out);

/* cattus_hip_create_calibrated (cattus_hip.h) with the same list of switches. */
int cattus_hip_create_calibrated_diag(const void* weights, size_t nbytes, const cattus_eval_config* cfg, const char* switches,
                                      const uint64_t* planes, uint32_t n, cattus_eval** out);

/* The stream shift t >= 0 of an f16 / f16x2 evaluator: its tower carries the residual stream at 2^t times its size, so that a
 * stream the trained BatchNorm parameters make small keeps the split activations' lo halves out of the f16 subnormals (exact
 * power-of-two weight products, chosen once from the network at create time; evaluator.hip, choose_stream_shift).  0 for f32
 * and bf16, for a network whose stream is not small, and under CATTUS_STREAM_SHIFT=0.  A calibrated evaluator
 * (cattus_hip_create_calibrated) reports the same rule on its measured mean squares. */
int cattus_hip_stream_shift(const cattus_eval* e);

/* The same per channel: out[k] = t_k >= t, n = the network's filters (anything else: CATTUS_E_INVALID).  Channel k of the stream is
 * carried at 2^t_k times its size; t_k > t where channel k alone is small beside the median one (weight_layout.h, stream_shifts).
 * All 0 wherever cattus_hip_stream_shift is 0 by dtype or switch.  Calibrated: weight_layout.h, calibrated_stream_shifts -- measured
 * channels, and a headroom guard that may take a t_k below t (never below 0).  The F(4x4, 3x3) tower (tower_form WINOGRAD_F4), whose
 * activations are capped at 655, also holds back on the estimate: a channel far above the median gets t_k < t, down to 0, so that its
 * estimated size times 2^t_k stays below 2 (weight_layout.h, stream_shifts' ceiling). */
int cattus_hip_stream_shifts(const cattus_eval* e, int* out, uint32_t n);

/* How the stem conv gets its input.  *channels: its input channels as laid out on the device (the planes padded with zero channels;
 * weight_layout.h, stem_cin_pad): f16x2 32 where the stem expands the planes itself and a multiple of 64 where they are packed first,
 * bf16 / f16 a multiple of 64, f32 a multiple of 32; the plane count itself on the towers that pad nothing.  *packed: 1 where the
 * plane pack runs as its own launch in front of the stem (per-layer and Winograd towers of a network of more than 32 planes, or under
 * CATTUS_FUSED_STEM=0), 0 where the stem kernel or a one-launch tower expands the planes itself.  Either pointer may be NULL. */
int cattus_hip_stem_input(const cattus_eval* e, uint32_t* channels, uint32_t* packed);

/* The K split of a tower_form DIRECT_SPLITK evaluator (CATTUS_E_UNSUPPORTED on every other): *ways = W, the waves of a workgroup, and, where
 * bounds is not NULL, bounds[0 .. W] = the boundaries of their ranges of 32-channel input chunks -- wave w walks chunks bounds[w] .. bounds[w + 1]
 * - 1 of every layer behind the stem, bounds[0] = 0, bounds[W] = padded filters / 32.  bounds needs room for W + 1 entries; W <= 8, so 9 always
 * suffice.  A function of the filter count (and of CATTUS_SPLITK_WAYS): the same for every max_batch. */
int cattus_hip_splitk_plan(const cattus_eval* e, uint32_t* ways, uint32_t* bounds);

/* The comparison kernel of cattus_hip_verify (cattus_hip.h) on host arrays, so that tests can feed it what no network produces.
 * policy_a / policy_b: [n][moves], value_a / value_b: [n], b the reference side; records: n x 16 bytes, per leaf
 *   f32 the largest |a - b| over the leaf's logits (a NaN difference takes no part; 0 where none is positive)
 *   u32 the lowest move index that holds it (0 where it is 0)
 *   f32 |value_a - value_b| (a NaN as 0x7fc00000)
 *   u32 flags: bit 0 the leaf is outside the bar, bit 1 its value is
 * The same inputs give the same bytes on every run.  n, moves >= 1. */
int cattus_hip_compare_outputs(int device, const float* policy_a, const float* policy_b, const float* value_a, const float* value_b,
                               uint32_t n, uint32_t moves, void* records /* [n][16 bytes] */);

/* The prior comparison kernel of cattus_hip_verify_prior_stats (cattus_hip.h) on host arrays.  probs_a / probs_b: [n][L] legal-move softmax
 * rows, b the reference side; legal_count: [n] (a count above L is compared over L entries and flagged); value_a / value_b: [n];
 * records: n x 32 bytes, per leaf
 *   f32 tv, u32 top_a, u32 top_b, f32 regret = probs_b[top_b] - probs_b[top_a], f32 max |a - b|, u32 the lowest k that holds it,
 *   u16 count = min(legal_count, L), u16 flags, f32 |value_a - value_b| (a NaN as 0x7fc00000)
 *   flags: bit 0 a non-finite probability (tv and regret are then 0x7fc00000), bit 1 count == 0, bit 2 legal_count > L, bit 3 a non-finite value
 * The same inputs give the same bytes on every run.  n >= 1, 1 <= L <= 1024. */
int cattus_hip_compare_priors(int device, const float* probs_a, const float* probs_b, const uint16_t* legal_count, uint32_t n, uint32_t L,
                              const float* value_a, const float* value_b, void* records /* [n][32 bytes] */);

#ifdef __cplusplus
}
#endif
#endif /* CATTUS_HIP_DIAG_H */
