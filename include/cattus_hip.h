/*
 * cattus_hip.h -- C ABI of the MI355X leaf evaluator for Cattus self-play.
 *
 * This library is the drop-in for the reference's leaf-evaluation seam: the closure body of
 * Batcher::apply inside NNetwork::evaluate_impl (engine/src/net/mod.rs:94-98), i.e.
 *     planes_to_tensor (engine/src/net/mod.rs:121-156)
 *  -> NNetwork::run_net (engine/src/net/mod.rs:41-72)
 *  -> Model::run        (engine/src/net/model.rs:146-218)
 * Input per leaf: the position's bitboard planes (position_to_planes,
 * engine/src/chess/net/mod.rs:19-60, hex/net.rs:14-24, ttt/net.rs:14-24) for the position
 * already flipped so Player1 is to move (net/mod.rs:79).  Output per leaf: the M raw policy
 * logits with non-finite values replaced by f32::MIN (net/mod.rs:56-61) and the tanh value.
 * Everything above the seam (flip, cache, legal-move softmax, MCTS) is unchanged.
 *
 * Conventions: every entry point returns 0 (CATTUS_OK) or a negative cattus_status; it never
 * throws, aborts or keeps a caller pointer.  cattus_hip_last_error() returns a thread-local
 * message for the last failing call on the calling thread.  All entry points are thread-safe.
 */
#ifndef CATTUS_HIP_H
#define CATTUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cattus_eval cattus_eval;

typedef enum cattus_status {
    CATTUS_OK = 0,
    CATTUS_E_INVALID = -1,     /* bad argument (the reference would panic: model.rs:100-125) */
    CATTUS_E_UNSUPPORTED = -2, /* shape/dtype combination this build has no kernel for */
    CATTUS_E_DEVICE = -3,      /* HIP runtime error; message in last_error */
    CATTUS_E_NOMEM = -4,
    CATTUS_E_STATE = -5,       /* unknown / already-collected ticket, evaluator shut down */
} cattus_status;

typedef enum cattus_dtype {
    CATTUS_DTYPE_F32 = 0,  /* exact f32 MFMA, bit-identical to the CPU oracle's summation order */
    CATTUS_DTYPE_BF16 = 1, /* bf16 operands / f32 accumulate MFMA tower (throughput mode, 8 significant bits) */
    /* Split precision: every activation and weight of the conv tower is a pair of f16 values (hi + lo, 22 significant
     * bits), a product is three f16 MFMA terms accumulated in f32, the heads run in exact f32.  Error against a
     * float64 run of the network is that of an f32 runtime (the reference's cross-runtime tolerance,
     * training/tests/test_net_output.py:28-33), at about a third of the bf16 tower's rate. */
    CATTUS_DTYPE_F16X2 = 2,
    /* Single-term f16: f16 operands and activations (11 significant bits; weights pre-scaled per output channel by a power
     * of two), f32 accumulation, f32 heads.  A throughput mode like bf16 -- same MFMA count and kernel -- with three more
     * significand bits; outside the reference's cross-runtime tolerance (DESIGN.md section 4 for what it does to a search). */
    CATTUS_DTYPE_F16 = 3,
    /* Single-term f16 in Winograd F(2x2, 3x3) form with an f32 stream: the stem on the direct f16 kernel, every layer behind it as
     * Y = A^T [sum_k U V] A with U = f16(G g G^T 2^s) and V = f16(B^T d B) (V made in f32 and rounded once), one f16 MFMA term per
     * product, f32 accumulation, and PLAIN F32 rows between the layers: the residual stream is never rounded to 11 bits.  2.25x fewer
     * MFMAs than CATTUS_DTYPE_F16; in emulation about twice as close to a float64 run of the network as that tower from two blocks
     * up (profiles/winograd_gate_f16w.json; device figures: profiles/f16w_numerics.txt).  Bits of its own.
     * Coverage: the Winograd form's -- an 8x8 board, at least one residual block, a multiple of 64 filters >= 128, vhc + phc <= 32;
     * anything else returns CATTUS_E_UNSUPPORTED, never other bits under this name.  Activations are capped at 16,376 (a transformed
     * input is a signed sum of four and must stay inside the f16 range) and counted in cattus_stats.saturated.
     * tower_form: AUTO and WINOGRAD both mean this form; DIRECT, WINOGRAD_F4, DIRECT_SPLITK and RESIDENT are refused with CATTUS_E_UNSUPPORTED.
     * tail_leaves is ignored (cattus_hip_tail_leaves reports 0).  A SimpleTwoHeadedModel blob runs in f32, as under every dtype.
     * cattus_hip_create_calibrated: the stream is f32, so a measured lift buys nothing here; the tower keeps the shifts of the BatchNorm
     * estimate and takes from the sample only the headroom guard (a channel's shift is lowered while its measured largest |value| 2^t
     * exceeds 4096, a quarter of the cap).  A network whose estimate is right keeps its shifts and its bits.
     * Measured, first build (scripts/f16w_time.py -> profiles/f16w_first_build.txt; one process, the towers alternating; chess 20x256, ms
     * per step at 64 / 128 / 256 leaves): F16W 0.50 / 0.68 / 1.24, F16 0.35 / 0.55 / 0.87, F16X2 in Winograd form (one launch) 0.89 /
     * 0.90 / 1.17; chess 4x128 at 256 leaves 0.116 / 0.097 / 0.152.  So it is 1.2 - 1.45x SLOWER than CATTUS_DTYPE_F16 at every size
     * measured, where 12 % is what two boxes differ by: NOT recommended for speed.  What it buys is F16's operand width at about half
     * F16's error (device: rms |dlogit| against float64 0.58x on the 4x128 fixture, 0.45x on the 20x256 one), and up to 128 leaves
     * 0.55 - 0.75x the step time of F16X2's Winograd form -- at 11 significant bits where that tower has 22.  Search level (256
     * searches of 800 simulations on chess 20x256 against the f32 search): 99.6 % of the moves equal, visit L1 mean 0.00037; F16 on the
     * same searches 99.2 %, 0.00039.  No counter or stamped run of the kernel was made: what its loop is bound by is not measured. */
    CATTUS_DTYPE_F16W = 4,
    /* F32 operands in Winograd F(2x2, 3x3) form on the f32 tower's own rows: the stem on the direct f32 kernel, unchanged and with
     * CATTUS_DTYPE_F32's bits; every layer behind it as Y = A^T [sum_k U V] A with U = f32(G g G^T) (the host's float64 transform
     * rounded once, no per-channel scale) and V = B^T d B made in f32, one f32 MFMA term per product, f32 accumulation, plain f32 rows
     * between the layers, the common f32 heads.  2.25x fewer MFMAs than CATTUS_DTYPE_F32, whose kernel is MFMA-bound.  No cap, no
     * stream shift, no saturation counter: cattus_stats.saturated stays 0 and values behave as under CATTUS_DTYPE_F32 (non-finite logits
     * are scrubbed by the heads as everywhere).  Bits of its own: another f32 summation order of other f32 operands than the exact
     * tower's, NOT that tower's bits -- but, like that tower's, an in-order fmaf chain that a CPU restatement reproduces bit for bit
     * (csrc/wino_f32_rule.h, tests/wino_f32_layer_ref.cpp).  cattus_hip_verify / _trace hold it to the f32 shadow like any other dtype.
     * Coverage: CATTUS_DTYPE_F16W's -- an 8x8 board, at least one residual block, a multiple of 64 filters >= 128, vhc + phc <= 32;
     * anything else returns CATTUS_E_UNSUPPORTED, never other bits under this name.  tower_form: AUTO and WINOGRAD both mean this form;
     * DIRECT, WINOGRAD_F4, DIRECT_SPLITK and RESIDENT are refused with CATTUS_E_UNSUPPORTED.  tail_leaves is ignored (cattus_hip_tail_leaves reports
     * 0).  A SimpleTwoHeadedModel blob runs in f32, as under every dtype.  cattus_hip_create_calibrated has nothing to calibrate: it
     * validates planes and n and is then cattus_hip_create.  cattus_hip_stream_range stays CATTUS_E_UNSUPPORTED (it measures on the exact
     * per-layer tower only).
     * Measured, first build (scripts/f32w_time.py -> profiles/f32w_first_build.txt; one process, the towers alternating; chess 20x256, ms
     * per step at 64 / 128 / 256 leaves): F32W 1.120 / 1.917 / 3.722, F32 1.646 / 3.101 / 5.701, F16X2 in Winograd form (one launch) 0.894 / 0.895 /
     * 1.189; chess 4x128 at 256 leaves 0.245 / 0.365 / 0.151.  So it is 1.47 - 1.62x FASTER than CATTUS_DTYPE_F32 at every size measured, where
     * 12 % is what two boxes differ by: RECOMMENDED over F32 from 64 leaves on where the coverage holds and F32's own bits are not needed.  68.8 k node-evals/s at 256 leaves
     * (F32: 44.9 k).  The estimate of ~55 us per 256 -> 256 layer was missed: 89.4 us per launch.  Per leaf (profiles/f32w_numerics.txt): inside
     * the reference's cross-runtime bar on both fixtures, rms |dlogit| against float64 0.80x / 0.54x F32's.  Search level (256 searches of
     * 800 simulations on chess 20x256 against the f32 search): 100.0 % of the moves equal, visit L1 mean 0.  Not measured: batches
     * below 64 leaves, other filter counts than 128 and 256; no counter or stamped run of the kernel was made: what binds its loop is
     * a supposition. */
    CATTUS_DTYPE_F32W = 5,
    /* Direct single-term f16 with an F32 RESIDUAL STREAM (K1hr, conv3x3_f16r_kernel): CATTUS_DTYPE_F16's weights, per-output-channel
     * power-of-two scales, [biases | inverse scales] and stream shifts, its kernel's roles and its MFMA sequence per accumulator -- only
     * the epilogue differs.  Per layer, y = relu(fmaf(acc, 2^-s, bias) [+ skip]) under the pixel mask:
     *   stem            writes the stream S as plain f32 rows holding y, not clamped, and its operand copy A = f16(min(y, 65504));
     *   conv1 of a block reads A, writes the middle activation M as f16 rows: CATTUS_DTYPE_F16's layer (no skip, clamp, count);
     *   conv2 of a block reads M, adds the F32 row of S (y = relu(fmaf(acc, 2^-s, bias) + S) in f32), writes y back to S in place and
     *                   A = f16(min(y, 65504));
     *   the last layer  writes S alone; the common f32 heads read it.
     * Values beyond 65504 in a copy are counted in cattus_stats.saturated; the stream itself keeps them.  So the stream is never rounded
     * to 11 bits, as under CATTUS_DTYPE_F16W, without that form's cost or coverage.  Bits of its own, anchored to CATTUS_DTYPE_F16's: a
     * network without blocks, and point 1 of any network, have that dtype's bits; point 0 rounds to its point 0.  The bits do not depend
     * on the tile.  Three lane buffers as before (S f32, A f16, M f16).
     * Coverage: every shape CATTUS_DTYPE_F16 runs on the MFMA per-layer tower -- any board up to 11x11, any filter count, up to 128
     * plane words, vhc + phc <= 32 (wider heads: CATTUS_E_UNSUPPORTED).  A SimpleTwoHeadedModel blob runs in f32, as under every dtype.
     * tower_form: AUTO means this tower; DIRECT, WINOGRAD, WINOGRAD_F4 and DIRECT_SPLITK, forms of the F16X2 tower, are ignored;
     * RESIDENT is CATTUS_E_UNSUPPORTED (the one-launch form of this tower is CATTUS_DTYPE_F16R_RESIDENT, below).  tail_leaves is ignored
     * (cattus_hip_tail_leaves reports 0).  cattus_hip_time_tower reports 1 + 2 blocks launches.  Observation: the stream points (0,
     * 2i + 2) are tapped from S in f32, times 2^-t_k, the middle points from M.  The stream shifts are CATTUS_DTYPE_F16's (they protect the
     * f16 copy's small channels).  cattus_hip_create_calibrated is accepted as for CATTUS_DTYPE_F16, with CATTUS_DTYPE_F16W's rule, the
     * stream being f32: the tower keeps the shifts of the BatchNorm estimate and takes from the sample the headroom guard, unchanged (a
     * channel's shift is lowered while its measured largest |value| 2^t exceeds 4096), so a network whose estimate is right keeps its
     * shifts and its bits; CATTUS_DTYPE_F16's measured lift of channels the estimate misses is not taken.
     * Measured, first build (scripts/f16r_time.py -> profiles/f16r_first_build.txt; one process, the towers alternating; ms per step,
     * F16R | F16 | F16W | F16X2 under AUTO): chess 20x256 at 64 leaves 0.369 | 0.354 | 0.495 | 0.602, at 128 0.576 | 0.544 | 0.676 |
     * 1.024, at 256 0.939 | 0.855 | 1.238 | 1.180; chess 4x128 at 256 leaves 0.104 | 0.098 | 0.116 | 0.151; hex7 6x64 at 128 leaves
     * 0.083 | 0.082 | not covered | 0.061 (resident).  So 1.01 - 1.10x CATTUS_DTYPE_F16's step time, inside the 12 % that two boxes
     * differ by: no difference from F16 in speed, and 0.75 - 0.90x F16W's time.  Per leaf (profiles/f16r_numerics.txt) rms |dlogit|
     * against float64 0.53x / 0.45x / 0.51x F16's on the chess 4x128 / chess 20x256 / hex7 6x64 fixtures (emulation, profiles/
     * gate_f16r.json: 0.53 / 0.44 / 0.52).  Search level (256 searches of 800 simulations on chess 20x256 against the f32 search): 100.0 %
     * of the moves equal, visit L1 mean 0.00006; F16 on the same searches 99.2 %, 0.00039, F16W 99.6 %, 0.00037.  RECOMMENDED wherever
     * F16 or F16W is used today; where a 64-filter resident form runs, as CATTUS_DTYPE_F16R_RESIDENT (below: the same bits in one launch).  The estimate written
     * before the run (+3 - 10 % on F16 by batch size) was met at its upper end.  Not measured: stamps, counters,
     * other filter counts than 256 / 128 / 64, batches below 64 leaves, two evaluators on one device. */
    CATTUS_DTYPE_F16R = 6,
    /* CATTUS_DTYPE_F16R's arithmetic, BIT FOR BIT, as a demand for the ONE-LAUNCH LDS-RESIDENT form (K1hr resident,
     * tower64_stream_kernel): every logit, every value and cattus_stats.saturated equal what the same blob returns from
     * CATTUS_DTYPE_F16R, for every n, through every entry point (tests/test_f16r_resident_gpu.py).  Behaviour of CATTUS_DTYPE_F16R, of
     * every other dtype and of every tower_form is unchanged; it is a dtype value because CATTUS_DTYPE_F16R with RESIDENT stays refused
     * and this struct stays 32 bytes.  The launch is tower64_lds_kernel's f16 instantiation -- loader waves, weight ring, plane expansion,
     * LDS plan (buffer 0 the f16 operand copy A, buffer 1 the planes and then the middle activation M) -- except where the stream lives:
     * a consumer lane finishes the same output elements in every layer, so the f32 stream S of those elements stays in that lane's
     * registers across the layer loop (16 values per lane at one board per workgroup, 32 at 128 rows) and never touches LDS; the last
     * layer stores it as f32 rows and the two f32 head launches follow, as under CATTUS_DTYPE_F16 with RESIDENT.  Weights, [biases |
     * inverse scales], stream shifts and cattus_hip_create_calibrated's rule are CATTUS_DTYPE_F16R's.
     * Coverage: exactly the evaluators on which CATTUS_DTYPE_F16 accepts tower_form RESIDENT -- at most 64 (padded) filters, vhc + phc <=
     * 32, at most 64 planes, no CATTUS_TOWER64=0; any board up to 11x11, any block count including 0 -- anything else is
     * CATTUS_E_UNSUPPORTED (never other bits under this name).  A SimpleTwoHeadedModel blob runs in f32, as under every dtype.
     * tower_form: AUTO and RESIDENT both mean this form; DIRECT, WINOGRAD, WINOGRAD_F4 and DIRECT_SPLITK are ignored as under
     * CATTUS_DTYPE_F16R.  tail_leaves is ignored (cattus_hip_tail_leaves reports 0).  cattus_hip_time_tower reports 1 launch.
     * Observation (cattus_hip_tap, cattus_hip_trace) runs the per-layer CATTUS_DTYPE_F16R pass on the same buffers: the same bits.
     * MEASURED on one MI355X (scripts/f16r_resident_time.py -> profiles/f16r_resident.txt: one process, max_batch = n, five evaluators
     * alternating over three rounds, 300 steps through cattus_hip_eval_device, min; F16R_RESIDENT | F16R | F16 RESIDENT | F16X2 | BF16, ms
     * per step):
     *   hex7 6x64:  32 leaves 0.042 | 0.072 | 0.040 | 0.053 | 0.024,  128: 0.043 | 0.075 | 0.041 | 0.053 | 0.025,  512: 0.059 | 0.110 | 0.058 | 0.088 | 0.037
     *     (the tower: one launch of 25.8 / 26.3 / 42.7 us against 13 of 4.5 / 4.7 / 6.6 us);
     *   chess 7x16: 64 leaves 0.050 | 0.083 | 0.049 | 0.061 | 0.031,  256: 0.053 | 0.094 | 0.052 | 0.062 | 0.032  (one launch of 32.4 / 33.5 us against 15 of 4.5 / 4.9).
     * Against the 12 % by which two boxes differ on one binary: RECOMMENDED OVER CATTUS_DTYPE_F16R ON ALL FIVE SHAPES (40-47 % less time per
     * step, the same bits); no shape was measured on which it is not.  It runs at F16 RESIDENT's speed (1.02-1.04x its step: inside that
     * spread) at about half F16's per-leaf error, and takes 0.67-0.86x F16X2's step -- 14-33 % less, beyond the spread on every shape --
     * at 11-bit operands where F16X2 has 22 bits; 1.6-1.7x BF16's step.  The estimate it was built on (DESIGN.md section 3, K1hr resident:
     * about F16 RESIDENT's 0.041 ms at hex7 6x64 and 128 leaves, within 3 %) held for the step (0.0425) and was missed by a point on the
     * margin (+3.7 % there, +2 - 4 % over the five shapes).  Not measured: in-kernel stamps or counters of tower64_stream_kernel, filter
     * counts other than 64 and 16 (padded to 64), two evaluators sharing a device, self-play. */
    CATTUS_DTYPE_F16R_RESIDENT = 7,
    /* (8 is unassigned and stays CATTUS_E_INVALID.) */
    /* CATTUS_DTYPE_F32's arithmetic, BIT FOR BIT -- and so the CPU oracle's -- as a demand for the ONE-LAUNCH LDS-RESIDENT form (K1rf,
     * tower64_f32_kernel): every logit and every value equal what the same blob returns from CATTUS_DTYPE_F32, for every n, through every
     * entry point (tests/test_f32_resident_gpu.py); cattus_stats.saturated stays 0.  Behaviour of CATTUS_DTYPE_F32, of every other dtype
     * and of every tower_form is unchanged, and AUTO never picks this plan; it is a dtype value because CATTUS_DTYPE_F32 with RESIDENT
     * stays refused and this struct stays 32 bytes.  One launch runs plane expansion, stem and every residual block: 512 threads, four
     * MFMA consumer waves and four LDS-DMA loader waves, 64 rows per workgroup (one 64-slot board, while the batch has at most 256 padded
     * boards) or 128 (two 64-slot boards, or one 128-slot board); the per-layer kernel's 3-slab weight ring in front of two f32
     * activation buffers of two 32-channel chunks each (107,008 / 139,776 B of LDS).  Per output element the operations are
     * conv3x3_mfma_v2_kernel<float>'s in its order: one v_mfma_f32_32x32x2_f32 chain over (chunk) x (kernel row) x (3 taps x 4 k-slices), +
     * bias, + skip, ReLU; no rounding, no clamp, no stream shift.  A network of at most 32 filters walks chunk 0 of its hidden layers only
     * (half the MFMAs, the same bits: the dropped terms are fmaf(0, 0, acc); diagnostic switch CATTUS_T64F_NARROW=0 walks both).  The last
     * layer leaves as the f32 rows the per-layer tower writes and the two f32 head launches follow unchanged.  Weights, biases and head
     * matrices are CATTUS_DTYPE_F32's uploads.
     * Coverage: at most 64 (padded) filters, vhc + phc <= 32, at most 32 planes, no CATTUS_TOWER64=0; any board up to 11x11, any block
     * count including 0 -- anything else is CATTUS_E_UNSUPPORTED (never other bits under this name; CATTUS_DTYPE_F32 runs every shape per
     * layer).  A SimpleTwoHeadedModel blob runs in f32, as under every dtype.  tower_form: AUTO and RESIDENT both mean this form; DIRECT,
     * WINOGRAD, WINOGRAD_F4 and DIRECT_SPLITK are ignored as under CATTUS_DTYPE_F32.  tail_leaves is ignored.  cattus_hip_time_tower reports
     * 1 launch, cattus_hip_tower_kernel "tower64_f32_kernel".  Observation (cattus_hip_tap) runs the per-layer CATTUS_DTYPE_F32 pass on the
     * same buffers: the same bits.  cattus_hip_verify / cattus_hip_trace are CATTUS_E_UNSUPPORTED as for CATTUS_DTYPE_F32 (the shadow would
     * be itself; the shadow and the calibration evaluator of other dtypes keep the per-layer f32 tower), cattus_hip_stream_range stays
     * CATTUS_E_UNSUPPORTED (it measures on the per-layer tower), cattus_hip_create_calibrated has nothing to calibrate and is
     * cattus_hip_create, cattus_hip_head_chain applies as under CATTUS_DTYPE_F32.
     * MEASURED on one MI355X (scripts/f32_resident_time.py -> profiles/f32_resident.txt: one process, max_batch = n, the evaluators
     * alternating over three rounds, 300 steps through cattus_hip_eval_device, min; F32_RESIDENT | F32 | F16X2 | F16R_RESIDENT, ms per step):
     *   hex7 6x64:  32 leaves 0.142 | 0.168 | 0.053 | 0.041,  128: 0.143 | 0.171 | 0.053 | 0.042,  512: 0.250 | 0.309 | 0.089 | 0.059
     *     (the tower: one launch of 125.6 / 126.7 / 233.8 us against 13 of 11.3 / 11.5 / 22.0 us);
     *   chess 7x16 (the narrow walk): 64 leaves 0.100 | 0.195 | 0.060 | 0.050,  256: 0.102 | 0.206 | 0.062 | 0.053  (one launch of 81.5 /
     *     82.6 us against 15 of 11.4 / 12.1; with CATTUS_T64F_NARROW=0 146.1 / 147.2 us and 0.164 / 0.166 ms per step: the narrow walk
     *     takes 0.61x that step, the same bits).
     * The yardstick is CATTUS_DTYPE_F32 in the same process on the same binary; against the 12 % by which two boxes differ on one binary:
     * RECOMMENDED OVER CATTUS_DTYPE_F32 ON ALL FIVE SHAPES, narrowly on hex7 6x64 (16 / 17 / 19 % less time per step, the same bits) and
     * clearly on chess 7x16 (49 / 51 %); no shape was measured on which it is not.  It stays 1.6-2.8x F16X2's step and 1.9-4.3x
     * F16R_RESIDENT's: the exact tower for checks, not a throughput mode.  The estimate it was built on (hex7
     * 6x64 at 128 leaves 0.18 -> 0.115-0.125 ms, 30-35 % less; chess 7x16 0.07-0.08) WAS MISSED: 0.143 and 0.100.  A step of 48 MFMAs
     * costs 1.54 us in the launch (from the two walks of chess 7x16), 64 cycles per MFMA at about 2.0 GHz where the estimate took 2.4.
     * Not measured: in-kernel stamps or counters of tower64_f32_kernel, the clock under this load, filter counts other than 64 and 16
     * (padded to 64), two evaluators sharing a device, self-play. */
    CATTUS_DTYPE_F32_RESIDENT = 9,
} cattus_dtype;
/* Every dtype takes any network the blob format and the plane pack allow: up to 128 plane words per leaf (planes x plane_words),
 * e.g. AlphaZero's 119 chess planes. */

/* Form of the f16x2 conv tower on 8x8 boards with a multiple of 128 filters.  The two forms agree to < 2e-6 per logit but not
 * bit for bit, and a leaf's bits must not depend on the batch it came in: the form is fixed per evaluator, here. */
typedef enum cattus_tower_form {
    CATTUS_TOWER_AUTO = 0,     /* Winograd where the shape allows it and max_batch > 128, else direct */
    CATTUS_TOWER_DIRECT = 1,   /* direct 3x3 (conv3x3_splitw_kernel): the faster form up to 128 leaves per batch */
    CATTUS_TOWER_WINOGRAD = 2, /* Winograd F(2x2,3x3) whatever max_batch is; CATTUS_E_UNSUPPORTED where no such kernel exists */
    /* Winograd F(4x4,3x3) (conv3x3_winof4_kernel): 36 products per 4x4 outputs and input channel where F(2x2,3x3) needs 64.  Opt-in:
     * NEVER chosen by AUTO, always one launch per layer.  Coverage as for WINOGRAD (f16x2, 8x8 board, at least one residual block, a
     * multiple of 64 filters, at least 128), else CATTUS_E_UNSUPPORTED.  Its bits are its own; on a 20-block network its error against
     * a float64 run is 2.2-2.8x the direct form's and inside the reference's cross-runtime tolerance (profiles/winograd_gate_f4.json).
     * The error grows with depth (chess 40x384: 2.7x the direct form's): networks far deeper than 20 blocks may leave that tolerance --
     * check with cattus_hip_verify.
     * Range: activations are capped at 655 in stream units -- 25x tighter than the other Winograd form's 16376 -- and a stream is
     * never shifted DOWN: a network whose activations pass 655 counts in cattus_stats.saturated and belongs on another form. */
    CATTUS_TOWER_WINOGRAD_F4 = 3,
    /* Direct 3x3 with the K walk of every layer behind the stem divided over the waves of a workgroup (conv3x3_splitk_kernel), for
     * evaluators whose batches hold a few leaves: the reference's threading model (threads: 8, batch_size: 1) through the leaf server.
     * A workgroup takes one board x 32 output channels; its W waves (8 from 256 filters on, 4 below: a function of the filter count
     * alone) each walk a contiguous range of 32-channel input chunks and the W partial sums are added in f32 as a pairwise tree by
     * wave index.  Opt-in: NEVER chosen by AUTO, legal for any max_batch.  Coverage: f16x2, a board of edge <= 8, at least one residual
     * block, a multiple of 64 filters from 128 to 512, else CATTUS_E_UNSUPPORTED.  ITS BITS ARE ITS OWN -- another f32 summation order
     * than DIRECT's, of the same quality (tests/test_splitk_gpu.py holds its error against float64 to at most twice DIRECT's) -- and a
     * leaf's bits still do not depend on its batch.  tail_leaves is ignored.  cattus_hip_splitk_plan() (cattus_hip_diag.h) reports W and
     * the waves' ranges.
     * MEASURED on one MI355X (scripts/splitk_time.py -> profiles/splitk_latency.txt: one process, max_batch = n, the forms alternating, 5 windows
     * of 200 steps through cattus_hip_eval_device, median; DIRECT | DIRECT_SPLITK, ms per step (us per conv launch)), chess 20x256:
     *   1 leaf 0.522 (11.7) | 0.398 (8.6),  4: 0.523 (11.7) | 0.399 (8.6),  8: 0.526 (11.7) | 0.407 (8.9),  16: 0.528 (11.8) | 0.414 (9.0),
     *   32: 0.532 (11.8) | 0.461 (10.1),  64: 0.589 (13.3) | 0.800 (18.5),  128: 0.978 (23.0) | 1.472 (35.1);
     * chess 4x128:  0.083 (7.7) | 0.076 (6.1) at 1 leaf ... 0.089 (8.6) | 0.084 (8.3) at 64,  0.093 (7.7) | 0.107 (9.3) at 128.
     * (A second run on another box is in the same file; ranges below are over both.)
     * Against the 12 % by which two boxes differ on one binary: RECOMMENDED UP TO 16 LEAVES PER BATCH ON 256 FILTERS (21-24 % faster per
     * step); at 32 leaves it is 8-13 % faster, which that spread covers; FROM 64 LEAVES ON IT IS 1.4-1.5x SLOWER (one workgroup per board and 32
     * couts, each fetching the whole 288 KiB of its cout block's weights).  On 128 filters the 5-9 % it gains up to 64 leaves are inside
     * the spread: not recommended there, and slower at 128.  The estimate it was built on -- the K loop's half of a launch falling 4-8x --
     * WAS MISSED: a launch falls from 11.7 to 8.6 us, not to ~7.  Forced way counts (1 | 2 | 4 | 8 ways: 23.7 | 13.9 | 9.8 | 8.6 us): each
     * doubling saves half of what the one before did, and 4 -> 8 ways only 1.2 us: what binds is the ~7.4 us that no split divides --
     * dispatch, the first loads (a wave's image and its chunk's 36 KiB of weights), the exchange and the epilogue.  16 blocking threads with one leaf per call through the leaf server
     * (9-12 leaves per batch, Python threads around cattus_hip_apply): 17.3-19.2 k -> 21.1-27.0 k leaves/s on chess 20x256.  Not measured:
     * in-kernel stamps or counters of the new kernel, filter counts other than 128 and 256, two evaluators sharing a device. */
    CATTUS_TOWER_DIRECT_SPLITK = 4,
    /* The whole conv tower in ONE launch with the activations resident in LDS, for networks of at most 64 (padded) filters -- every
     * network the reference trains.  A demand, like WINOGRAD: CATTUS_E_UNSUPPORTED where no such kernel covers the evaluator.
     *   dtype f16: opt-in, NEVER chosen by AUTO (which runs 1 + 2 * blocks conv3x3_mfma_v2_kernel launches).  tower64_lds_kernel in its
     *     f16 instantiation, on the shapes dtype bf16 runs that kernel on: value + policy head channels <= 32 and at most 64 filters.  THE
     *     BITS DO NOT CHANGE: every logit and value equals, bit for bit, what the same blob returns from dtype f16 with AUTO, for every n,
     *     through every entry point, and cattus_stats.saturated counts the same elements (tests/test_resident_f16_gpu.py).  The last layer
     *     leaves the launch as f32 rows and the two f32 head launches follow: three launches per step where bf16 has two.
     *   dtype bf16, f16x2: accepted exactly where AUTO already runs tower64_lds_kernel / tower64_split_kernel, with that plan and its bits.
     *   dtype f32, f16w, f32w, more than 64 filters, CATTUS_TOWER64=0: CATTUS_E_UNSUPPORTED.  A SimpleTwoHeadedModel blob runs in f32 as
     *     under every form.  tail_leaves is ignored.
     * MEASURED on one MI355X (scripts/resident_f16_time.py -> profiles/resident_f16.txt: one process, max_batch = n, four evaluators
     * alternating over three rounds, 300 steps through cattus_hip_eval_device, min; f16 RESIDENT | f16 AUTO | bf16 | f16x2, ms per step):
     *   hex7 6x64:  32 leaves 0.040 | 0.072 | 0.024 | 0.053,  128: 0.041 | 0.075 | 0.025 | 0.053,  512: 0.057 | 0.104 | 0.038 | 0.090
     *     (the tower: one launch of 24.6 / 26.0 / 42.4 us against 13 of 4.7 / 4.7 / 6.3 us);
     *   chess 7x16: 64 leaves 0.049 | 0.083 | 0.031 | 0.061,  256: 0.052 | 0.091 | 0.032 | 0.062  (one launch of 30.6 / 32.8 us against 15 of 4.7 / 4.9).
     * Against the 12 % by which two boxes differ on one binary: RECOMMENDED FOR dtype f16 ON ALL FIVE SHAPES (41-45 % less time per step,
     * 1.7-1.8x); no shape was measured on which it is not.  It is also 16-36 % faster per step than f16x2 there, and takes 1.5-1.7x bf16's
     * time: the f16 epilogue, and the f32 head convs as a third launch (fusing them into the tower's tail is the follow-up).  The estimate
     * it was built on (~0.04 against ~0.11 ms at 128 leaves, 2.5x; 1.5x at 512) held for the resident step (0.041) and
     * MISSED THE RATIO at 128 leaves, where f16 AUTO is faster than estimated (0.075: its launches take 4.7 us, not bf16's 6.3 of round 1),
     * and was exceeded at 512 (1.8x).  Not measured: in-kernel stamps or counters of the f16 instantiations, filter counts other than 64
     * and 16 (padded to 64), two evaluators sharing a device. */
    CATTUS_TOWER_RESIDENT = 5,
} cattus_tower_form;

/* Replaces the reference's InferenceConfig + batch_size (engine/src/net/model.rs:17-25,
 * training/self-play/src/self_play_cmd.rs:41-44). */
typedef struct cattus_eval_config {
    /* sizeof(cattus_eval_config) = 32.  The earlier lengths are accepted too: 24 (the fields up to flush_us: tower_form = AUTO) and
     * 28 (up to tower_form); both mean tail_leaves = 0. */
    uint32_t struct_size;
    int32_t device;       /* HIP device ordinal */
    uint32_t max_batch;   /* model.batch_size: largest n accepted by eval / batch the server fills */
    uint32_t plane_words; /* u64 words per bitboard plane: chess 1, ttt 1, hex 2 (u128 as lo,hi) */
    uint32_t dtype;       /* cattus_dtype */
    uint32_t flush_us;    /* partial-batch deadline of the leaf server (reference: 20 ms, net/mod.rs:96) */
    uint32_t tower_form;  /* cattus_tower_form; the forms 1 to 4 are ignored by every dtype but f16x2 */
    /* Short batches of the Winograd F(2x2,3x3) tower (f16x2, AUTO with max_batch > 128 or WINOGRAD).  0, the default: nothing changes.
     * k > 0: a batch of n <= k leaves runs the layers behind the stem on conv3x3_wino4s_kernel, a kernel for the same arithmetic whose
     * workgroup takes 2 boards x 32 output channels where the tower's takes 4 x 64 -- four times as many workgroups for a batch that
     * leaves most of the chip idle.  THE BITS DO NOT CHANGE: every logit and value equals, bit for bit, what the evaluator returns with
     * tail_leaves = 0, for every n and every k, so a leaf's result still does not depend on the batch it came in
     * (tests/test_short_batches_gpu.py).  Ignored (cattus_hip_tail_leaves reports 0) on every other plan: the direct form, f32 / bf16 /
     * f16, WINOGRAD_F4, networks of <= 64 filters.  k > max_batch is CATTUS_E_INVALID.
     * Measured (whole step through cattus_hip_eval_device, default | tail_leaves = n, ms; scripts/short_batch_time.py ->
     * profiles/wino_short_batches.txt), chess 20x256:  1 leaf 0.894 | 0.760,  8: 0.896 | 0.768,  16: 0.893 | 0.779,  32: 0.892 | 0.786,
     * 64: 0.894 | 0.799,  96: 0.898 | 1.482,  128: 0.902 | 1.501;  chess 4x128: 0.145 | 0.108 at 1 leaf ... 0.145 | 0.118 at 128.
     * Against the 12 % by which two boxes differ on one binary that makes it RECOMMENDED UP TO 16 LEAVES ON 256 FILTERS (13-15 % faster;
     * at 32 and 64 it is 12 % and 11 % faster, inside that spread) and up to 128 on 128 filters (18-25 % faster).  From the batch whose
     * grid passes the device's 256 CUs on (more than 64 leaves on 256 filters) it is 1.65x SLOWER: never set it above
     * 64 * 256 / filters.  The default stays 0. */
    uint32_t tail_leaves;
} cattus_eval_config;

typedef struct cattus_stats {
    uint64_t batches;       /* == reference metric model.activation_count (net/mod.rs:68) */
    uint64_t positions;     /* real (non-padded) leaves evaluated */
    uint64_t full_batches;  /* batches that ran with n == max_batch */
    double run_seconds_ema; /* == reference metric model.run_duration (EMA 0.99, util/metric.rs:16-19) */
    double run_seconds_total;
    /* f16x2 / f16 towers: activation values that exceeded the f16 range (65504; in the Winograd form of the f16x2 tower a
     * quarter of it, 16376: its transformed inputs are sums of four; in the F(4x4,3x3) form 655) and were clamped, since the evaluator was created (sticky).  0 for every network inside the range; > 0 means outputs of this evaluator are NOT the network's:
     * use dtype f32 for that network (a BatchNorm scale of 1e5 does it; one of 200 does not). */
    uint64_t saturated;
} cattus_stats;

/* Network shape as stored in the weight blob header (cattus_amd/weights.py).  filters == 0 (with blocks = vhc = phc = 0) is
 * the reference's other model type, SimpleTwoHeadedModel (training/cattus_train/net_utils.py:92-121: two dense layers and two
 * dense heads on the flattened planes); it is evaluated in f32 whatever dtype is configured. */
typedef struct cattus_net_desc {
    uint32_t planes, board, moves, blocks, filters, vhc, phc, fc_hidden;
} cattus_net_desc;

/* Model::new (model.rs:61): parse the weight blob (copied), fold BatchNorm, upload.  Everything that selects a code path is in
 * `cfg`; the library reads two operational environment variables and no other: CATTUS_HIP_WAIT=block (the host thread sleeps
 * on an event instead of spinning while a batch runs) and CATTUS_ROCTX=1 (ROCTx ranges around every batch).  The A/B switches
 * of the tests and timing scripts go through cattus_hip_create_diag (cattus_hip_diag.h), never through the environment; the
 * same header declares cattus_hip_stream_shift() and cattus_hip_stream_shifts(), what an f16 / f16x2 evaluator chose for its
 * residual stream and for each channel of it, and cattus_hip_stem_input(), how the stem gets its input.  A network of more than 128 plane words per
 * leaf (planes x cfg->plane_words) is refused with CATTUS_E_UNSUPPORTED, whatever the dtype; up to there every dtype takes it. */
int cattus_hip_create(const void* weights, size_t nbytes, const cattus_eval_config* cfg, cattus_eval** out);
void cattus_hip_destroy(cattus_eval* e);
int cattus_hip_desc(const cattus_eval* e, cattus_net_desc* out);

/* Calibration of the f16 / f16x2 towers on sample positions.  Those towers carry channel k of the residual stream (the stem output
 * and every block's output) at 2^t_k times its size, so that a small channel keeps its 22 significant bits.  cattus_hip_create
 * takes t_k from an estimate of the channel's RMS, the BatchNorm gamma / beta that write the stream; that is exact only while
 * every BatchNorm input has unit variance under its running statistics.  A converted checkpoint whose scale sits elsewhere -- in
 * the conv rows and running means, say -- is estimated at O(1) whatever its stream does.  These two entry points measure instead.
 *
 * cattus_hip_stream_range: rms and largest |value| of every stream channel over the n leaves' S x S pixels and the 1 + blocks
 * stream tensors, measured on the exact f32 tower.  `e` must be a dtype f32 evaluator on the MFMA per-layer tower (value + policy
 * head channels <= 32), anything else is CATTUS_E_UNSUPPORTED; channels must be the network's filters and n >= 1, else
 * CATTUS_E_INVALID.  Any n: the call walks the leaves in chunks of max_batch.  Blocking; takes a lane as cattus_hip_eval does;
 * the same leaves give the same bytes on every call (no atomics in the reduction), and later evaluations are not changed by it. */
typedef struct cattus_channel_range { float rms, abs_max; } cattus_channel_range;
int cattus_hip_stream_range(cattus_eval* e, const uint64_t* planes, uint32_t n, cattus_channel_range* out, uint32_t channels);
/* cattus_hip_create with the shifts taken from measurement.  dtype f16x2 / f16: builds a temporary f32 evaluator of the same blob on
 * cfg->device (max_batch = min(n, 256)), measures the n leaves ([n][planes][plane_words], as cattus_hip_eval takes them), destroys
 * it, and creates the evaluator exactly as cattus_hip_create does except for the shifts: the same rule fed with the measured mean
 * squares, then a headroom guard -- t_k drops while abs_max 2^t_k > 4096, a quarter of the Winograd form's cap, never below 0.
 * dtype f32 / bf16 and SimpleTwoHeadedModel blobs have nothing to calibrate: planes and n are validated (non-NULL, n >= 1) and the
 * call is cattus_hip_create.  A few hundred positions of real play are plenty; cattus_hip_create_calibrated_diag() and the
 * read-back of what was chosen are in cattus_hip_diag.h. */
int cattus_hip_create_calibrated(const void* weights, size_t nbytes, const cattus_eval_config* cfg, const uint64_t* planes, uint32_t n,
                                 cattus_eval** out);

/* planes_to_tensor + run_net for n leaves, blocking (1 <= n <= max_batch, net/mod.rs:122-127).
 * planes: [n][planes][plane_words] u64 host memory; policy: [n][moves]; value: [n]. */
int cattus_hip_eval(cattus_eval* e, const uint64_t* planes, uint32_t n, float* policy, float* value);

/* cattus_hip_eval followed by calc_moves_probs (engine/src/net/mod.rs:100-119) on the device: the
 * logits stay in HBM and each leaf's softmax over its legal moves comes back instead.
 * legal_idx: [n][legal_stride] policy indices (Move::to_nn_idx) of the leaf's legal moves, in the
 * order the caller wants the probabilities; legal_count: [n], each <= legal_stride <= 1024;
 * probs: [n][legal_stride], entries past legal_count[i] are 0.  max = fold(f32::MIN, max), the sum
 * runs in move order, exp is the evaluator's own, so a host restatement
 * reproduces the result bit for bit. */
int cattus_hip_eval_legal(cattus_eval* e, const uint64_t* planes, uint32_t n, const uint16_t* legal_idx,
                          const uint16_t* legal_count, uint32_t legal_stride, float* probs, float* value);

/* Same with every buffer already resident in device memory (HBM) and asynchronous on `stream`, a
 * hipStream_t taken as HIP takes it: NULL is the legacy default stream.  All work of the call is enqueued
 * on that stream and nowhere else, so the caller orders it (and reads d_policy / d_value) with the
 * stream's own means: later work on the same stream, an event, or hipStreamSynchronize.  The evaluator's
 * intermediate buffers belong to a lane (below): two calls on one lane must not overlap on the device.
 * Used by bench.py so that the timed region excludes PCIe. */
int cattus_hip_eval_device(cattus_eval* e, const uint64_t* d_planes, uint32_t n, float* d_policy,
                           float* d_value, void* stream);

/* The evaluator keeps CATTUS_HIP_LANES independent sets of activation buffers.  cattus_hip_eval and the
 * leaf server pick a free one per call, so that many host threads can each have a batch in flight;
 * cattus_hip_eval_device uses lane 0.  This variant names the lane: work enqueued on different lanes
 * and different streams may overlap on the device (the tail of one batch's kernels with the head of
 * the other's).  Two calls on the same lane must be ordered by the caller (same stream or events). */
#ifndef CATTUS_HIP_LANES
#define CATTUS_HIP_LANES 2
#endif
int cattus_hip_eval_device_lane(cattus_eval* e, uint32_t lane, const uint64_t* d_planes, uint32_t n,
                                float* d_policy, float* d_value, void* stream);
/* The lane's own non-blocking stream (the one cattus_hip_eval uses for that lane), for callers of the
 * device entry points that have no stream of their own. */
int cattus_hip_lane_stream(cattus_eval* e, uint32_t lane, void** stream);

/* Leaf-batching server, the replacement of Batcher::apply (engine/src/util/batch.rs:49-177):
 * submit copies one leaf's planes and returns a ticket; wait blocks until that leaf's batch ran
 * and copies its logits/value out.  A batch runs when max_batch leaves are queued, when the oldest
 * queued leaf is flush_us old, or on cattus_hip_flush. */
int cattus_hip_submit(cattus_eval* e, const uint64_t* planes_one, uint64_t* ticket);
int cattus_hip_wait(cattus_eval* e, uint64_t ticket, float* policy, float* value);
int cattus_hip_flush(cattus_eval* e);
/* Batcher::apply as the reference's worker threads call it (engine/src/util/batch.rs:49-177,
 * net/mod.rs:94-98): a blocking call with the signature of cattus_hip_eval that goes through the leaf
 * server, i.e. the n leaves (n = 1 from a search thread) share batches with whatever the other calling
 * threads submit meanwhile; a batch runs when max_batch leaves are queued or flush_us have passed. */
int cattus_hip_apply(cattus_eval* e, const uint64_t* planes, uint32_t n, float* policy, float* value);

/* The leaf server with calc_moves_probs (engine/src/net/mod.rs:100-119) on the device: what a search thread of the reference does per
 * leaf -- Batcher::apply (engine/src/util/batch.rs:49-177), then the softmax over the leaf's legal moves on the host -- as one call.  The
 * logits stay in HBM; the leaf's probabilities come back in place of its M logits.
 *
 * Batcher::apply + calc_moves_probs per leaf.  legal_idx: legal_count policy indices (Move::to_nn_idx) in the order the caller wants the
 * probabilities back; 0 <= legal_count <= 1024, every index < moves: anything else is CATTUS_E_INVALID, checked on the host at submit, and
 * nothing is queued.  legal_count == 0 is valid: the value comes back and no probability is written (legal_idx and probs may be NULL).
 *
 * Leaves of cattus_hip_submit and cattus_hip_submit_legal share batches, their sealing (max_batch leaves, flush_us, cattus_hip_flush) and
 * the lanes.  Inside a batch the lists lie back to back with one offset per leaf (a ragged layout: no stride to agree on); a batch whose
 * leaves all carry a list copies no logits to the host, only its probabilities and values; a mixed batch copies the logits as well, for its
 * plain leaves.  The arithmetic is cattus_hip_eval_legal's -- max = fold(f32::MIN, max), the evaluator's own exp, the sum in move order
 *  -- so a leaf and its list give that call's bits, whatever batch they came in, and a host restatement reproduces them.
 *
 * A ticket is claimed by the call that matches its submit: cattus_hip_wait on a legal ticket and cattus_hip_wait_legal on a plain one are
 * CATTUS_E_INVALID and leave the ticket claimable by the right call.  SimpleTwoHeadedModel evaluators are supported, as by cattus_hip_eval_legal.
 * The first cattus_hip_submit_legal of an evaluator allocates the staging for max_batch lists of 1024 per lane (it waits for the batches in
 * flight); an evaluator that never calls these entry points allocates nothing for them. */
int cattus_hip_submit_legal(cattus_eval* e, const uint64_t* planes_one, const uint16_t* legal_idx, uint32_t legal_count, uint64_t* ticket);
int cattus_hip_wait_legal(cattus_eval* e, uint64_t ticket, float* probs /* [legal_count of that submit] */, float* value);
/* submit_legal + wait_legal for n leaves, blocking, through the server like cattus_hip_apply:
 * legal_off [n + 1] ascending with legal_off[0] == 0; legal_idx and probs hold legal_off[n] entries back to back.  Offsets that do not start
 * at 0 or descend, a list above 1024 and an index >= moves are CATTUS_E_INVALID, checked before the first leaf is queued. */
int cattus_hip_apply_legal(cattus_eval* e, const uint64_t* planes, uint32_t n, const uint16_t* legal_idx, const uint32_t* legal_off,
                           float* probs, float* value);

/* Page-locked host memory.  cattus_hip_eval transfers directly from / into buffers allocated here
 * (no staging copy); any other host memory works too, through the evaluator's own staging buffers. */
void* cattus_hip_host_alloc(size_t bytes);
void cattus_hip_host_free(void* p);

int cattus_hip_stats(cattus_eval* e, cattus_stats* out);

/* Live verification against a shadow f32 tower.  `saturated` above fires only when the f16 range is left; this tells how far a bf16 /
 * f16 / f16x2 evaluator is from the exact network on the positions it is actually given.  With every >= 1, every `every`-th batch of
 * the blocking entry points (cattus_hip_eval, cattus_hip_eval_legal, and the leaf server behind submit / wait / apply) is, behind its
 * own forward pass and on the same device-resident leaves, also run through a dtype f32 evaluator of the same blob that this evaluator
 * builds on first use and owns; the two outputs are compared on the device, and a small sticky record is kept.  Batches take a ticket
 * each while verification is on, counted from 0, and ticket % every == 0 is verified: with verification on from the start an
 * evaluator's first batch is always checked.  every == 0 turns it off again: the record and the shadow stay, and turning it on once
 * more goes on counting.  What the caller gets back for a verified batch is bit for bit what it gets without verification;
 * cattus_stats counts what it counted before (the shadow pass is no batch), except that run_seconds_ema leaves verified batches out
 * (run_seconds_total has them: the caller did wait).  The asynchronous device entry points, cattus_hip_eval_device and
 * cattus_hip_eval_device_lane, do NOT verify.
 *
 * The bar is the reference's own cross-runtime tolerance (training/tests/test_net_output.py:28-33), with the f32 shadow as the
 * reference side: a logit is inside when |a - b| <= 1e-6 + 1e-3 |b|, a value when |a - b| <= max(1e-5 max(|a|, |b|), 1e-6), both in
 * double; a non-finite operand is outside; two scrubbed logits (both f32::MIN) differ by 0 and are inside.  A leaf is outside when its
 * value or any of its logits is.
 *
 * Cost.  The shadow is a second copy of the weights, in f32, plus two lanes of f32 activations in HBM (CATTUS_E_NOMEM where that does
 * not fit).  A verified batch costs one f32 tower pass on top of its own -- several times its own length -- and the f32 pass
 * displaces the Winograd tower's working set in the Infinity Cache, which the batch behind it pays for;
 * profiles/verify_cost.txt has what every = 1, 8 and 64 were measured to cost on chess 20x256.
 *
 * leaves_outside > 0 means what saturated > 0 means: outputs of this evaluator are not the network's by the reference's own bar -- use
 * dtype f32 for that network, or calibrate (cattus_hip_create_calibrated).
 *
 * `weights` is the blob the evaluator was created from, passed again because the evaluator keeps no host copy of it: another blob
 * (by size or by a 64-bit hash taken at create) is CATTUS_E_INVALID.  A dtype f32 evaluator (the shadow would be itself) and a
 * SimpleTwoHeadedModel (f32 whatever the dtype) are CATTUS_E_UNSUPPORTED.  The call waits for the batches in flight. */
typedef struct cattus_verify_stats {
    uint32_t struct_size;   /* in: sizeof(cattus_verify_stats) */
    uint32_t every;         /* 0 = off */
    uint64_t batches, leaves, leaves_outside;
    float max_dlogit, logit, logit_ref; uint32_t move;   /* the largest |dlogit| seen and where: this evaluator's logit, the shadow's, the move index */
    float max_dvalue, value, value_ref; uint32_t reserved;
} cattus_verify_stats;
int cattus_hip_verify(cattus_eval* e, const void* weights, size_t nbytes, uint32_t every);
/* The sticky record since the evaluator was created.  Of several leaves with the same largest difference the first one verified is kept. */
int cattus_hip_verify_stats(cattus_eval* e, cattus_verify_stats* out);
/* The planes of the leaf that holds max_dlogit, as it was given to the evaluator.  CATTUS_E_STATE before any leaf was verified.
 * (cattus_hip_compare_outputs() in cattus_hip_diag.h runs the comparison kernel alone, on host arrays.) */
int cattus_hip_verify_worst_planes(cattus_eval* e, uint64_t* planes /* [planes][plane_words] */);

/* The same verification in the quantities a PUCT search consumes.  The logit bar above is the reference's cross-runtime tolerance: a bf16 or
 * f16 evaluator (8 and 11 significant bits) is outside it on practically every leaf by construction, so leaves_outside == leaves tells
 * nothing about them.  A search consumes the softmax over the leaf's legal moves (calc_moves_probs, engine/src/net/mod.rs:100-119) and the
 * value; this record compares those, per leaf, on the device.
 *
 * What feeds it.  A verified batch (ticket % every == 0, as above) of cattus_hip_eval_legal: behind the logit comparison the shadow's logits
 * go through the same legal-move softmax with the same legal_idx / legal_count, and the two probs rows -- pa, what the call returns, and
 * pb, what the exact network would have returned -- are compared per leaf over k < c = min(legal_count, legal_stride):
 *   tv      = float(0.5 sum_k |pa[k] - pb[k]|), the total-variation distance, summed in double in a fixed order (prior_rule.h: the bytes
 *             can be restated on a CPU)
 *   regret  = pb[top_ref] - pb[top]: the prior mass the exact network's favourite loses; top / top_ref are the positions in the legal
 *             list of the largest pa / pb, the lowest on ties; exactly 0 when they agree, >= 0 otherwise
 * A leaf with a non-finite probability on either side is counted in `nonfinite`, one with legal_count == 0 in `empty`; neither enters a
 * sum, a maximum or the histogram, so tv_mean = sum_tv / (leaves - nonfinite - empty).  Verified batches of cattus_hip_eval carry no legal
 * moves: they count in batches_without_legal and feed the value part alone.  A verified batch of the leaf server feeds it the same way as
 * cattus_hip_eval_legal when at least one of its leaves came through cattus_hip_submit_legal / cattus_hip_apply_legal: those leaves are compared
 * in slot order, each over its own list (c = its legal_count), and the batch's plain leaves (cattus_hip_submit / apply) feed the value part
 * alone; a server batch of plain leaves only counts in batches_without_legal.  The value
 * part runs over every verified leaf of all paths whose two values are finite: sum_dvalue = sum |value - value_ref|.
 * The asynchronous device entry points, cattus_hip_eval_device and cattus_hip_eval_device_lane, still do NOT verify and feed nothing.
 *
 * Cost: two HBM-trivial launches and 32 bytes per leaf of device-to-host copy behind a batch that already pays for an f32 pass; nothing
 * for a batch that is not verified.  What the caller gets back is bit for bit what it gets without verification, and cattus_verify_stats
 * and cattus_stats hold what they held.
 *
 * A dtype f32 evaluator and a SimpleTwoHeadedModel are CATTUS_E_UNSUPPORTED, as for cattus_hip_verify. */
typedef struct cattus_prior_stats {
    uint32_t struct_size; /* in: sizeof(cattus_prior_stats) */
    uint32_t reserved;
    uint64_t batches;               /* verified batches that came with legal moves */
    uint64_t batches_without_legal; /* verified batches that did not: value part only */
    uint64_t leaves;                /* leaves of `batches`, nonfinite and empty ones included */
    uint64_t top1_flips;            /* leaves whose favourite move differs from the exact network's */
    uint64_t nonfinite, empty;
    double sum_tv, sum_regret;
    float max_tv, max_regret;
    uint64_t tv_hist[8];            /* upper edges 1e-7, 1e-6, .., 1e-1, +inf: a leaf is in the first bucket whose edge exceeds its tv */
    uint64_t value_leaves;          /* verified leaves of both paths with two finite values */
    double sum_dvalue;
} cattus_prior_stats;
int cattus_hip_verify_prior_stats(cattus_eval* e, cattus_prior_stats* out);
/* The leaf that holds max_tv -- the first one compared, then every strictly larger one -- as it was given to the evaluator: its planes
 * [planes][plane_words], its *legal_count = min(legal_count, legal_stride) legal moves into legal_idx[cap], and both favourites as positions in
 * that list (*top this evaluator's, *top_ref the exact network's).  CATTUS_E_STATE before any leaf was compared, CATTUS_E_INVALID when
 * cap is smaller than the leaf's legal count.  (cattus_hip_compare_priors() in cattus_hip_diag.h runs the comparison kernel alone.) */
int cattus_hip_verify_worst_prior(cattus_eval* e, uint64_t* planes, uint16_t* legal_idx, uint32_t cap, uint32_t* legal_count, uint32_t* top,
                                  uint32_t* top_ref);

/* Layer-level observation.  leaves_outside > 0 or saturated > 0 says that this evaluator left the exact network somewhere; these two calls
 * say where.  A ConvNetV1 evaluator has P = 1 + 2 * blocks + 1 points:
 *   point 0        the stem ConvBlock's output (the residual stream), `filters` channels
 *   point 2i + 1   block i behind conv1 + bn1 + ReLU, `filters` channels
 *   point 2i + 2   block i's output (the residual stream), `filters` channels
 *   point P - 1    the two head ConvBlocks' outputs, the value head's channels first, then the policy head's: vhc + phc channels
 *
 * cattus_hip_tap returns point `point` of n leaves (1 <= n <= max_batch) as the reference module holds it: f32 [n][C][S][S], in network
 * units.  Whatever the evaluator stores there -- f32, bf16 or f16 rows, (hi, lo) f16 pairs, the heads' fragment order; a stream channel
 * carried at 2^t (the f16 towers) -- is decoded exactly (hi + lo in f32, the widening of a bf16 / f16) and multiplied by the exact inverse
 * of that power of two: a tap is a deterministic bit pattern, not an approximation.  Pixel slots, boards and channels of the evaluator's
 * padding never reach a result.  policy / value (both may be NULL) receive the logits and values of that pass.
 *
 * Every tower plan is observed on the per-layer form of its own arithmetic -- the resident one-launch towers and the one-launch Winograd
 * tower on the per-layer launches that the equality tests hold them to, bit for bit -- so the outputs are cattus_hip_eval's.  An evaluator
 * that never calls tap or trace runs what it ran before, on the buffers it had before.
 *
 * cattus_hip_trace runs the n leaves through this evaluator's per-layer pass and through the f32 shadow's (cattus_hip_verify's: built on
 * first use by whichever of the two calls comes first, from `weights`, the blob the evaluator was created from) in lockstep, and compares
 * the two on the device behind every point: out[point * n + leaf] is one record, `points` the P that the caller sized it for.  Nothing but
 * the P * n records grows with the number of points.  The same leaves give the same bytes on every run.
 *
 * Both calls block, and take a lane as cattus_hip_eval does.  Neither is a batch: batches, positions, full_batches and run_seconds_* do
 * not count them and no verify ticket is taken; `saturated` does count what their passes clamp (it is the kernels' own counter).
 *
 * CATTUS_E_UNSUPPORTED: a SimpleTwoHeadedModel (all three calls); trace on a dtype f32 evaluator (its shadow would be itself).
 * CATTUS_E_INVALID: another blob than the evaluator's own, point >= P, points != P, n outside 1..=max_batch. */
int cattus_hip_points(const cattus_eval* e, uint32_t* points);
int cattus_hip_tap(cattus_eval* e, const uint64_t* planes, uint32_t n, uint32_t point, float* out /* [n][C_point][S][S] */, float* policy,
                   float* value);
typedef struct cattus_trace_record {
    float max_diff; uint32_t at;   /* largest float(|double(x) - double(ref)|) over the leaf's live elements (NaN differences take no part; 0 at
                                      index 0 where none is positive); at = channel * S * S + pixel, the lowest index on ties */
    float x, ref;                  /* this evaluator's value and the shadow's there */
    float rms_diff, rms_ref;       /* sqrt(mean (x - ref)^2), sqrt(mean ref^2) over all live elements, sums in double; a NaN is 0x7fc00000 */
    uint32_t flags, reserved;      /* bit 0: a non-finite value on either side */
} cattus_trace_record;
int cattus_hip_trace(cattus_eval* e, const void* weights, size_t nbytes, const uint64_t* planes, uint32_t n,
                     cattus_trace_record* out /* [P][n] */, uint32_t points, float* policy, float* value);

/* Average device time in microseconds of one 3x3-conv tower launch over `reps` forwards of n
 * leaves.  Every launch carries its own start/stop HIP event pair stamped by the kernel dispatch
 * itself (hipExtLaunchKernelGGL) on the evaluator's stream.  Also returns the number of such
 * launches per forward. */
int cattus_hip_time_tower(cattus_eval* e, uint32_t n, uint32_t reps, float* avg_launch_us, uint32_t* launches);

/* Diagnostic: the rate (TFLOP/s) the matrix pipe of the evaluator's device sustains on nothing but back-to-back MFMAs of
 * the evaluator's tower kind (f16x2: v_mfma_f32_32x32x16_f16, bf16: ..._bf16, f32: v_mfma_f32_32x32x2_f32) -- one wave per
 * SIMD on every CU, operands in registers, launches of ~50 us repeated for `seconds` (0 < seconds <= 30), the last group's
 * rate.  The nominal peaks are 2.4 GHz figures; under MFMA load the device's power management sets the clock. */
int cattus_hip_mfma_sustained(cattus_eval* e, double seconds, double* tflops);

/* Stand-alone planes_to_tensor (engine/src/net/mod.rs:121-156): host planes [n][C][plane_words]
 * -> host f32 tensor [batch][C][S][S], rows n..batch zero. */
int cattus_hip_planes_to_tensor(int device, const uint64_t* planes, uint32_t n, uint32_t C, uint32_t plane_words,
                                uint32_t S, uint32_t batch, float* out);
/* Device-resident variant, asynchronous on `stream`. */
int cattus_hip_planes_to_tensor_device(const uint64_t* d_planes, uint32_t n, uint32_t C, uint32_t plane_words,
                                       uint32_t S, uint32_t batch, float* d_out, void* stream);

/* Name of the kernel that runs this evaluator's tower (the dominant kernel of a forward pass): "conv3x3_splitw_kernel",
 * "tower_wino4_kernel" (f16x2 on 8x8 boards with max_batch > 128: the Winograd tower, every layer behind the stem in one launch),
 * "tower64_split_kernel", "conv3x3_mfma_v2_kernel", ... */
const char* cattus_hip_tower_kernel(const cattus_eval* e);

/* cattus_eval_config.tail_leaves as it holds for this evaluator: the configured value on a Winograd F(2x2,3x3) plan, 0 on every other
 * (the field is ignored there).  cattus_hip_tower_kernel keeps naming the plan's kernel. */
int cattus_hip_tail_leaves(const cattus_eval* e, uint32_t* effective);
/* Batches that took the short path (n <= tail_leaves, not observed by tap / trace) since the evaluator was created, through any entry
 * point; a timing pass of cattus_hip_time_tower is not a batch. */
int cattus_hip_tail_batches(cattus_eval* e, uint64_t* batches);

/* The f32 heads' FC pair as short chains.  0 (the default): nothing changes.  k >= 1: a batch of n <= k leaves runs FC1 + FC2 and the policy FC on
 * head_fc_chain_kernel instead of head_fc_pair_kernel<float>: one output element per lane, its dot product a v_fma_f32 chain in the MFMA's k order
 * (4 cycles per k where the pair's single v_mfma_f32_32x32x2_f32 chain pays 32) on the operands the heads already have -- no second upload, no new
 * layout; the head convs are untouched.  THE BITS DO NOT CHANGE: every logit, value and prior equals what the evaluator returns with 0, for every n
 * and k, through every entry point (tests/test_head_chain_gpu.py).  k > max_batch: CATTUS_E_INVALID.  Accepted and ignored
 * (cattus_hip_head_chain_leaves reports 0) where the heads are not the f32 MFMA heads: dtype bf16, value + policy head channels > 32 (generic
 * path), SimpleTwoHeadedModel.  Waits for the batches in flight.  Observed passes (tap, trace), cattus_hip_time_tower, the verification shadow and
 * the calibration's temporary evaluator keep the MFMA pair.
 * Measured (whole step through cattus_hip_eval_device, ms, 0 | k = n, one evaluator alternating, min of 3 rounds x 300 steps; scripts/head_chain_time.py ->
 * profiles/head_chain.txt): hex7 6x64 f16x2  32 leaves 0.0612 | 0.0595, 128: 0.0616 | 0.0599, 512: 0.0969 | 0.0978;  f16r_resident  32: 0.0499 | 0.0484,
 * 128: 0.0506 | 0.0496, 512: 0.0678 | 0.0708;  f32  128: 0.1796 | 0.1786.  chess 7x16 f16x2  1: 0.0586 | 0.0551, 8: 0.0590 | 0.0557, 64: 0.0603 | 0.0597,
 * 256: 0.0618 | 0.0754;  f16r_resident  1: 0.0472 | 0.0437, 8: 0.0488 | 0.0455, 64: 0.0500 | 0.0496, 256: 0.0530 | 0.0661.  chess 20x256 f16x2: within
 * 1.2 % either way at 1 .. 256.  The estimate this was built on (the FC launch 12-18 -> 4-7 us on K = 784, the hex7 step -15 to -20 %) WAS MISSED: the
 * step falls by 2-3 % on hex7 6x64 and by 6-7 % on chess 7x16 up to 8 leaves, and from the batch whose grid passes one workgroup per CU on it RISES
 * (chess, 1880 moves: +22-25 % at 256 leaves).  No shape reaches the 12 % by which two boxes differ on one binary, so the chain form is RECOMMENDED
 * NOWHERE; where it is tried, never set k above 64 on a chess head (1880 moves) or 128 on a hex7 head (49 moves).  The default stays 0.  Not measured:
 * the FC launch alone (no kernel trace of the new build), self-play throughput, boards other than 7x7 and 8x8, more than 512 leaves. */
int cattus_hip_head_chain(cattus_eval* e, uint32_t leaves);
int cattus_hip_head_chain_leaves(const cattus_eval* e, uint32_t* effective);
/* Batches whose FC pair took the chain form since the evaluator was created, through any entry point (as cattus_hip_tail_batches). */
int cattus_hip_head_chain_batches(cattus_eval* e, uint64_t* batches);

/* The two 1x1 head convs in the tail of the resident f16 and f16r towers.  0 (the default): nothing changes.  on != 0: an unobserved pass launches
 * the HEADS instance of the plan's resident kernel (tower64_lds_tower<..., HEADS>): the last layer's f32 rows stay in LDS,
 * the consumer waves run head_conv_tile<float>'s chain on them (head weights and biases brought into dead ring bytes under the last layer) and write hv;
 * the tower's output rows are not written to memory and head_conv_kernel<float> is not launched -- two launches per pass instead of three.  THE BITS DO
 * NOT CHANGE: every logit, value, prior and the saturation count equal what the evaluator returns with 0, through every entry point
 * (tests/test_fused_heads_gpu.py).  Effective (cattus_hip_fused_heads_effective reports 1) on CATTUS_DTYPE_F16 under CATTUS_TOWER_RESIDENT and
 * CATTUS_DTYPE_F16R_RESIDENT (cattus_hip_tower_kernel, which this setting does not change); accepted and ignored (0) everywhere else: the bf16 and
 * f16x2 resident towers, which run the head convs in their tails always, and CATTUS_DTYPE_F32_RESIDENT, whose kernel has no such instance.  Waits
 * for the batches in flight.  Composes with cattus_hip_head_chain.  Observed passes (tap, trace), cattus_hip_time_tower, the verification shadow and the
 * calibration's temporary evaluator keep the head conv launch.  UNMEASURED (scripts/fused_heads_time.py is the method, DESIGN.md
 * section 3, K3r, has the estimate): recommended nowhere until it is.  The default stays 0. */
int cattus_hip_fused_heads(cattus_eval* e, uint32_t on);
int cattus_hip_fused_heads_effective(const cattus_eval* e, uint32_t* effective);
/* Passes that ran the head convs in the tower's tail since the evaluator was created, through any entry point (as cattus_hip_tail_batches). */
int cattus_hip_fused_heads_batches(cattus_eval* e, uint64_t* batches);

const char* cattus_hip_last_error(void);
const char* cattus_hip_version(void);
/* What the last cattus_hip_create found for HIP_FORCE_DEV_KERNARG (the host process exports it before HIP initialises:
 * kernel arguments in device memory, -8 % per batch; the library never changes the environment itself). */
const char* cattus_hip_runtime_note(void);

#ifdef __cplusplus
}
#endif
#endif /* CATTUS_HIP_H */
