// Internal launch interface between evaluator.hip (host logic) and kernels.hip (gfx950 kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frag_index.h"  // split_frag_index, wino_frag_index, WINO_RING_STAGES
#include "verify_rule.h"  // VerifyRecord and the rule behind it
#include "prior_rule.h"   // PriorRecord and the rule behind it
#include "legal_span.h"   // the ragged layout of the leaf server's legal-move lists
#include "tap_layout.h"   // TapSource, TraceRecord: where a point's activations live, the rule of a trace record
#include "winof4_rule.h"  // the Winograd F(4x4, 3x3) form: matrices, transforms, geometry, cap, U index
#include "splitk_rule.h"  // the split-K direct form: ways, ranges, reduction order, grid map, LDS plan
#include "f16r_rule.h"    // dtype f16r: the epilogue with an f32 residual stream, the lane buffers' roles, the tap layout per point
#include "head_chain_rule.h"  // the short-chain form of the f32 FC pair: grid map, operand offsets, walk order, epilogues
#include "t64r_rule.h"    // dtype f16r_resident: that tower in one LDS-resident launch -- who owns an element, the LDS buffers, the layer table
#include "t64f_rule.h"    // dtype f32_resident: the exact f32 tower in one LDS-resident launch -- LDS plan, step table, ownership map, layer table
#include "head_fuse_rule.h"  // cattus_hip_fused_heads: the f32 head convs in the tail of the resident f16 and f16r towers -- LDS plan, ownership, chain, hv index

namespace cattus {

// Tower layout: a board owns 64 pixel slots (board edge <= 8) or 128 (edge 9..11); rows = board * slots + slot.
inline uint32_t tower_slots(uint32_t S) { return S <= 8 ? 64u : 128u; }
constexpr int ROWS_PER_WG = 256; // tower rows per workgroup of the conv kernel: 4 boards of 64 slots, 2 of 128
constexpr int COUT_PER_WG = 64;  // output channels per workgroup of the tower conv kernel

// Activation element of the tuned tower: 2-byte bf16, 4-byte f32, a pair of f16 values (hi, lo) of 2 + 2 bytes
// (the split-precision tower: 128 bytes of a row are [hi of 32 channels | lo of the same 32]), or a single 2-byte f16
// (the single-term f16 tower: the bf16 kernel's layout and MFMA count with 11 significant bits instead of 8).
enum class Act : int { F32 = 0, BF16 = 1, F16S = 2, F16 = 3 };

inline bool act_two_bytes(Act a) { return a == Act::BF16 || a == Act::F16; }
inline int act_bytes(Act a) { return act_two_bytes(a) ? 2 : 4; }  // bytes of one activation in HBM
// Input channels consumed per pipeline stage: one 128-byte LDS row.
inline int act_kc(Act a) { return act_two_bytes(a) ? 64 : 32; }
// Element type of the head kernels (K3-K5) for a tower of type `a`: the f16 towers' heads run in exact f32 (their last
// layer writes plain f32 rows).
inline Act head_act(Act a) { return a == Act::BF16 ? Act::BF16 : Act::F32; }
// The f16 towers: weights pre-scaled per output channel by a power of two, the bias buffer carries the inverse scales,
// activations saturate at 65504 (counted), the last layer writes f32 rows.
inline bool act_f16_family(Act a) { return a == Act::F16S || a == Act::F16; }

// Sets the > 64 KiB dynamic-LDS attribute of every tower kernel variant on the current device; called once per device
// from cattus_hip_create before the first launch.
hipError_t prepare_device();

// ---- K0: bitboard planes -> tensors -------------------------------------------------------
// NHWC tower input [bpad][slots][cpad] in the activation layout of `act` -- f32, bf16 or f16 rows, or the F16S pairs (4 bytes per
// channel, [hi of 32 channels | lo of the same 32] per 128 bytes; hi = f16(bit), lo = 0); rows >= n, slots >= S*S and channels >= C
// are zero.  C * w64 <= 128 plane words, cpad >= C a multiple of one 128-byte row of the layout.
void launch_pack_planes_nhwc(Act act, const uint64_t* planes, uint32_t n, uint32_t bpad, uint32_t C,
                             uint32_t w64, uint32_t S, uint32_t cpad, void* out, hipStream_t st);
// Reference layout: f32 NCHW [batch][C][S*S], rows >= n zero (engine/src/net/mod.rs:121-156).
void launch_planes_to_tensor_nchw(const uint64_t* planes, uint32_t n, uint32_t C, uint32_t w64, uint32_t S,
                                  uint32_t batch, float* out, hipStream_t st);

// ---- K1/K2: 3x3 conv + folded BN (+ residual) + ReLU, MFMA, NHWC -------------------------
// in [bpad][slots][cin], w [9][cout][cin], bias [cout] f32, res/out [bpad][slots][cout], slots = tower_slots(S).
// Requires bpad * slots % 256 == 0, cin % kc == 0, cout % 64 == 0, S <= 11.
// ev_start / ev_stop (optional): events stamped with the kernel's own begin / end time.
// stem (optional): the layer reads the leaves' bitboard planes instead of `in` (K0 fused into the stem conv: the
// loader waves expand the planes straight into LDS).  Requires C <= 32 planes and cin == one 128-byte row; more planes go
// through launch_pack_planes_nhwc and the layer without `stem` (F16S: cin a multiple of 64 then, see CONV_W_FRAG below).
struct StemInput {
    const uint64_t* planes;  // [n][C][w64]
    uint32_t n, C, w64;
};
// Act::F16S (split precision): rows of in / res / out and of w are f16 pairs interleaved in groups of 32 channels,
// [hi of channels 32g .. 32g+31 | lo of the same 32] per 128 bytes; w is pre-scaled per output channel by a power of
// two, bias is [cout biases | cout inverse scales]; cin counts channels (pairs).
// Act::F16 (single-term f16): rows of f16 values in the bf16 tower's layout, w [9][cout][cin] f16 pre-scaled as above, bias
// [cout biases | cout inverse scales].
// flags & CONV_OUT_F32 (F16S / F16 only): out is written as plain f32 [row][cout] (last tower layer, read by the f32 head kernels).
// flags & CONV_W_FRAG (F16S only): w is in MFMA fragment order, [cout / 32][stage][hi | lo][lane][8 f16] with
// stage = ((chunk * 3 + dy) * 3 + dx) * 2 + k-half (split_frag_index): the kernel that keeps the weights in a register
// ring instead of LDS.  Non-stem layers then need cin >= 64.
// flags & CONV_WINO_IN (with CONV_OUT_F32): the rows feed a Winograd tower (K1w): values are capped at WINO_ACT_MAX and counted in
// `sat` beyond it -- a transformed input B^T d B is a signed sum of four activations, so no |V| can leave the f16 range then and the
// Winograd kernel's transform needs neither a clamp nor a range check of its own.
// flags & CONV_WINOF4_IN (with CONV_OUT_F32, instead of CONV_WINO_IN): the rows feed a Winograd F(4x4, 3x3) tower (K1f4): the same cap
// and count at WINOF4_ACT_MAX (winof4_rule.h).
constexpr int CONV_OUT_F32 = 1, CONV_W_FRAG = 2, CONV_WINO_IN = 4, CONV_WINOF4_IN = 8;
constexpr float WINO_ACT_MAX = 16376.0f;  // 65504 / 4, exactly
// Per-evaluator launch options (they used to be process-wide switches: a second evaluator must not re-tile the first).
struct ConvOpts {
    int cb = 0;   // forces the conv kernel's tile: 1 = 256 rows x 32 couts, 2 = 256 rows x 64 couts; 0 = chosen by grid size
    int pbw = 0;  // 2: never / 1: whenever the tile is 32 couts -- the 128-row workgroup; 0 = chosen by grid size
    // F16S / F16: device counter of activation values that were clamped to 65504 (atomic add on the clamp path only);
    // must be non-null for those towers
    unsigned* saturated = nullptr;
};
void launch_conv3x3_mfma(Act act, const void* in, const void* w, const float* bias, const void* res, void* out,
                         uint32_t bpad, uint32_t cin, uint32_t cout, uint32_t S, hipStream_t st,
                         hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr, const StemInput* stem = nullptr,
                         int flags = 0, const ConvOpts& opts = ConvOpts());

// ---- K1hr: the single-term f16 layer with the residual stream in f32 (dtype f16r; conv3x3_f16r_kernel in kernels.hip; f16r_rule.h has
// the epilogue, the buffer plan and the tap layouts) ----
// The Act::F16 layer of launch_conv3x3_mfma -- in, w, bias = [cout biases | cout inverse scales], the tiles, ConvOpts -- except for what
// leaves it: `stream` [bpad][slots][cout] plain f32 rows, not clamped, is the layer's output and, with `skip`, also its skip rows, updated
// in place (the lane that reads an element writes it; `in` must be another buffer); `copy` [bpad][slots][cout] f16 rows receives
// f16(min(y, 65504)), counted in ConvOpts::saturated beyond it, unless `last` (the tower's last layer writes the stream alone; copy may be
// NULL then).  stem as there; a stem layer has no skip.  Same MFMA sequence per accumulator as the Act::F16 layer.
void launch_conv3x3_f16r(const void* in, const void* w, const float* bias, float* stream, bool skip, void* copy, uint32_t bpad, uint32_t cin,
                         uint32_t cout, uint32_t S, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop, const StemInput* stem, bool last,
                         const ConvOpts& opts);

// ---- K1w: the split-precision conv in Winograd F(2x2, 3x3) form (kernels_wino.hip) ----
// 8x8 boards only; in / res / out are PLAIN F32 rows [row][channel] (what CONV_OUT_F32 writes: a tower in this form keeps f32
// activations between its layers); wu = G g G^T as (hi, lo) f16 pairs pre-scaled per output channel, in fragment order
// [cout / 32][(cin / 16) k-steps x 16 frequencies][hi | lo][lane][8 f16] (wino_frag_index); bias = [cout biases | cout inverse
// scales] of THAT scaling; res may be out (a block's output over its skip rows); outputs are capped at WINO_ACT_MAX and sat counts
// the threads that wrote the cap.  The kernel's weight ring reads WINO_RING_STAGES stages past a cout block's end (frag_index.h).
bool wino_supported(uint32_t bpad, uint32_t cin, uint32_t cout, uint32_t S);
void launch_conv3x3_wino(const float* in, const void* wu, const float* bias, const float* res, float* out, uint32_t bpad, uint32_t cin,
                         uint32_t cout, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop, unsigned* sat);
hipError_t prepare_wino();  // its dynamic-LDS opt-in; called by prepare_device()

// ---- K1w4: the same layer with 4 frequencies x (2 tile blocks x 2 cout blocks) per wave (kernels_wino4.hip) ----
// Same arguments, same U buffer, same bits as launch_conv3x3_wino; workgroup = 4 boards x 64 couts (bpad % 4 == 0, cout % 64 == 0):
// half of K1w's U bytes per CU, the transformed input made in registers.  The evaluator prefers it wherever it is supported.
bool wino4_supported(uint32_t bpad, uint32_t cin, uint32_t cout, uint32_t S);
void launch_conv3x3_wino4(const float* in, const void* wu, const float* bias, const float* res, float* out, uint32_t bpad, uint32_t cin,
                          uint32_t cout, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop, unsigned* sat);
hipError_t prepare_wino4();
// The whole Winograd tower in one launch (tower_wino4_kernel): a table of its layers in device memory (an even number: residual blocks,
// the first layer of a block without skip rows, the second with; res may equal out), `ready` = nlayers x (bpad / 4) zeroed counters, `err` a zeroed word the launch sets when a hand-off wait ran out of
// `spin_budget` polls (the outputs are then invalid: run the batch on the per-layer launches).  Only while wino4_tower_fits: every
// workgroup resident at once (one per CU), and never two such launches on one device at a time.
struct Wino4TowerLayer {
    const float* in;
    const void* wu;
    const float* bias;
    const float* res;
    float* out;
};
bool wino4_tower_fits(uint32_t bpad, uint32_t filters, uint32_t cus);
void launch_tower_wino4(const Wino4TowerLayer* d_layers, uint32_t nlayers, unsigned* ready, unsigned* err, unsigned* sat, uint32_t bpad, uint32_t filters,
                        uint32_t spin_budget, uint32_t cus, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop);

// ---- K1w4s: the same layer on a small tile, for short batches (kernels_wino4s.hip; wino4s_rule.h has its geometry and LDS plan) ----
// Same arguments, same U buffer, same bits as launch_conv3x3_wino4 wherever wino4_supported holds; workgroup = 2 boards x 32 couts, grid
// (bpad / 2) x (cout / 32), one launch per layer, no cross-workgroup synchronisation.  Nothing is read past U's last stage or the rows.
void launch_conv3x3_wino4s(const float* in, const void* wu, const float* bias, const float* res, float* out, uint32_t bpad, uint32_t cin,
                           uint32_t cout, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop, unsigned* sat);
hipError_t prepare_wino4s();

// ---- K1wh: the SINGLE-TERM f16 conv in Winograd F(2x2, 3x3) form (dtype f16w; kernels_wino_f16.hip; wino_f16_rule.h has its geometry) ----
// The arguments of launch_conv3x3_wino4s: in / res / out plain f32 rows on 8x8 boards, res may be out; wu = f16(U 2^s) alone in the order
// of wino_f16_frag_index (weight_layout.h: wino_u_f16; nothing is read past it); bias = [cout biases | cout inverse scales] of that
// scaling.  V = B^T d B in f32, rounded once to f16; one MFMA term per product, f32 accumulation, k ascending; outputs capped at
// WINO_ACT_MAX, sat counts the threads that wrote the cap.  Workgroup = 2 boards x 32 or 64 couts (wf16_ncb; the same bits either way),
// one launch per layer, no cross-workgroup synchronisation.  bpad % 2 == 0, cin and cout multiples of 64 >= 128.
bool wino_f16_supported(uint32_t bpad, uint32_t cin, uint32_t cout, uint32_t S);
void launch_conv3x3_wino_f16(const float* in, const void* wu, const float* bias, const float* res, float* out, uint32_t bpad, uint32_t cin,
                             uint32_t cout, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop, unsigned* sat);
hipError_t prepare_wino_f16();

// ---- K1wf: the F32-OPERAND conv in Winograd F(2x2, 3x3) form (dtype f32w; kernels_wino_f32.hip; wino_f32_rule.h has its geometry and its
// arithmetic order) ----
// The arguments of launch_conv3x3_wino_f16: in / res / out plain f32 rows on 8x8 boards (the f32 tower's rows), res may be out; wu =
// f32(G g G^T) without a scale in the order of wino_f32_frag_index (weight_layout.h: wino_u_f32; nothing is read past it); bias = cout
// biases.  V = B^T d B in f32; one f32 MFMA chain per product (Mfma<float>::mac, 8-channel groups ascending); Y + bias, + skip, ReLU; no
// cap: the last argument is not read.  Workgroup = 2 boards x 32 or 64 couts (wf32_ncb; the same bits either way), one launch per layer,
// no cross-workgroup synchronisation.  bpad % 2 == 0, cin and cout multiples of 64 >= 128.
bool wino_f32_supported(uint32_t bpad, uint32_t cin, uint32_t cout, uint32_t S);
void launch_conv3x3_wino_f32(const float* in, const void* wu, const float* bias, const float* res, float* out, uint32_t bpad, uint32_t cin,
                             uint32_t cout, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop, unsigned* unused);
hipError_t prepare_wino_f32();

// ---- K1sk: the direct split-precision layer with the K walk divided over the waves of a workgroup (kernels_splitk.hip; splitk_rule.h has the
// split, the reduction order, the grid map and the LDS plan) ----
// The arguments of launch_conv3x3_mfma's Act::F16S layer with CONV_W_FRAG: in / res / out rows of (hi, lo) pairs on 64-slot boards (S <= 8), wf
// the fragment-ordered weights, bias = [cout biases | cout inverse scales]; flags & CONV_OUT_F32 as there.  Workgroup = one board x 32 couts,
// grid boards x (cout / 32), W = splitk_ways(cin / 32, forced_ways) waves; its bits are those of the direct kernels only for W = 1.
// splitk_supported: cin and cout multiples of 64, 128 .. SK_MAX_FILTERS; anything else aborts.
bool splitk_supported(uint32_t cin, uint32_t cout, uint32_t S);
void launch_conv3x3_splitk(const void* in, const void* wf, const float* bias, const void* res, void* out, uint32_t boards, uint32_t cin, uint32_t cout,
                           uint32_t S, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop, int flags, int forced_ways, unsigned* sat);
hipError_t prepare_splitk();  // its dynamic-LDS opt-in; called by prepare_device()

// ---- K1f4: the split-precision conv in Winograd F(4x4, 3x3) form (kernels_winof4.hip; winof4_rule.h has the rule) ----
// The arguments of launch_conv3x3_wino4: in / res / out plain f32 rows on 64-slot boards, res may be out; wu = G g G^T as (hi, lo) f16
// pairs pre-scaled per output channel in the order of winof4_frag_index (weight_layout.h: winof4_u; nothing is read past it); bias =
// [cout biases | cout inverse scales] of that scaling; outputs are capped at WINOF4_ACT_MAX and sat counts the threads that wrote the cap.
// bpad % 4 == 0: a workgroup takes 8 boards, the last one 4 when bpad is no multiple of 8.
bool winof4_supported(uint32_t bpad, uint32_t cin, uint32_t cout, uint32_t S);
void launch_conv3x3_winof4(const float* in, const void* wu, const float* bias, const float* res, float* out, uint32_t bpad, uint32_t cin,
                           uint32_t cout, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop, unsigned* sat);
hipError_t prepare_winof4();

// ---- calibration: the range of one stream tensor of the f32 per-layer tower (cattus_hip_stream_range) ----
// rows: plain f32 [nb * slots][FP] (nb * slots % 256 == 0, FP % 64 == 0), of which board < n and pixel slot < S * S are live.  Adds,
// per channel, the live values' sum of squares to acc_sq [FP] (double) and folds their largest |value| into acc_max [FP] -- the
// caller zeroes both once and they collect tensor after tensor, ordered by `st`.  part_sq / part_max: scratch of
// stream_range_parts(bpad, S) * FP entries (bpad >= nb), the workgroups' partials, folded in index order by a second launch: the
// same bits on every run, no floating-point atomics.
size_t stream_range_parts(uint32_t bpad, uint32_t S);
void launch_stream_range(const float* rows, uint32_t nb, uint32_t n, uint32_t S, uint32_t FP, double* part_sq, float* part_max, double* acc_sq,
                         float* acc_max, hipStream_t st);

// ---- verification: an evaluator's outputs against its f32 shadow's (cattus_hip_verify, cattus_hip_compare_outputs) ----
// policy_a / policy_b: [n][M] logits, value_a / value_b: [n], b the shadow's; records: [n], 16-byte aligned, one verify_rule.h verdict per
// leaf; detail: NULL, or [n][4] floats, 16-byte aligned: logit_a, logit_b at the record's move, value_a, value_b.  The same inputs give the
// same bytes on every run (no atomics).
void launch_verify_outputs(const float* policy_a, const float* policy_b, const float* value_a, const float* value_b, uint32_t n, uint32_t M,
                           VerifyRecord* records, float* detail, hipStream_t st);

// probs_a / probs_b: [n][L] legal-move softmax rows of the evaluator and of its shadow (launch_legal_softmax on either's logits), cnt: [n]
// legal counts, value_a / value_b: [n]; records: [n], one prior_rule.h record per leaf.  The same inputs give the same bytes on every run.
// row_off: NULL, or the offset table [n + 1] of a ragged batch (legal_span.h): leaf i's two rows then start at row_off[i] and are as long as
// its list, and cnt / L are not read.
void launch_verify_priors(const float* probs_a, const float* probs_b, const uint16_t* cnt, const float* value_a, const float* value_b, uint32_t n,
                          uint32_t L, PriorRecord* records, hipStream_t st, const uint32_t* row_off = nullptr);

// ---- observation: one point of the network (cattus_hip_tap, cattus_hip_trace; tap_layout.h has the layouts and the record) ----
// src: the tensor as the evaluator holds it (TapSource), shifts: NULL, or per live channel the exponent t the tensor carries it at (device,
// s.C ints); out: f32 [n][s.C][s.hw], 16-byte aligned, in network units.  Rows layouts of the tuned towers' padding (pitch % 64 == 0) go
// through the transposing kernel, everything else through a gather.  Only leaves < n, pixels < hw and channels < C are read into a result.
void launch_tap(const void* src, const TapSource& s, const int* shifts, uint32_t n, float* out, hipStream_t st);
// x (layout sx, shifts as above) against ref (layout sref, the f32 shadow's: nothing to divide out), the same C and hw: records [n],
// 32-byte aligned, one per leaf.  The same inputs give the same bytes on every run (no atomics).
void launch_trace_compare(const void* x, const TapSource& sx, const int* shifts, const void* ref, const TapSource& sref, uint32_t n, TraceRecord* records,
                          hipStream_t st);

// Diagnostic: one launch of nothing but back-to-back MFMAs of the tower's kind (F16S: f16, BF16, F32: 32x32x2 f32), four
// waves on each of `cus` workgroups, iters x 4 MFMAs per wave; `out` holds cus * 256 floats.  Returns the launch's FLOPs.
double launch_mfma_sustain(Act act, int cus, int iters, float* out, hipStream_t st);

// ---- K1 resident: whole tower of a network with <= 64 (padded) filters in one launch, bf16 or single-term f16 (see kernels.hip) ----
struct Tower64Layer {
    const void* w;      // [9][64][64] bf16 / f16 (stem: input channels padded to 64); f16: pre-scaled per output channel
    const float* bias;  // [64]; f16: [64 biases | 64 inverse scales]
    int res;            // 1: add the block input (second conv of a residual block)
    int pad_;
};
struct Tower64Args {
    const uint64_t* planes;      // [n][C][w64] bitboards
    const Tower64Layer* layers;  // device array [nlayers]: stem, then (conv1, conv2) per block
    void* out;                   // bf16, optional: [rows][64] bf16 tower output, rows = boards * tower_slots(S); f16: the same in f32, required unless the heads are fused
    unsigned* sat;               // f16: the evaluator's saturation counter (ConvOpts::saturated); bf16: not read
    uint32_t n, C, w64, S, nlayers;
    // optional, fused K3: the two 1x1 head convs (+ folded BN + ReLU) on the resident tower output, written in the
    // layout the head FC kernels read (HeadsMfma::hv).  f16 (cattus_hip_fused_heads; head_fuse_rule.h): in f32, instead of `out`
    const void* head_w;   // [32][64] bf16 (f16: f32), value rows first, rows >= ocn zero
    const float* head_b;  // [32]: entries >= ocn are not used
    void* hv;             // head activations in the fragment-packed layout of HeadsMfma::hv, bf16 (f16: f32)
    uint32_t hv_pol, kvp, kpp, vhc, ocn;  // hv_pol: element offset of the policy part
};
// rows % 256 == 0; ch = 2: 128 rows per workgroup, ch = 4: one 64-slot board per workgroup (small batches; 128-slot
// boards run as ch = 2).  layer_steps: with ch = 4 and boards of <= 63 pixels, one barrier per layer instead of three
// (two layers of weights in LDS); same results.  act: Act::BF16, or Act::F16 with sat set and exactly one of out (the f32 head kernels read
// it) and head_w + head_b + hv (the HEADS instances: the head convs in the tail, nothing written to out); anything else aborts.
void launch_tower64(Act act, const Tower64Args& args, uint32_t rows, int ch, bool layer_steps, hipStream_t st,
                    hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// K1hr resident (dtype f16r_resident; tower64_stream_kernel; t64r_rule.h has the ownership map, the LDS buffers and the layer table): the
// Act::F16 launch above -- its arguments, layers (dtype f16r's = dtype f16's weights and [biases | inverse scales]; Tower64Layer::res as
// t64r_layer().skip), workgroup shapes and LDS plan -- with the residual stream kept in f32 in the owning lanes' registers: the bits of
// the per-layer f16r tower (launch_conv3x3_f16r and dtype f16's conv1).  args.sat required, and exactly one of args.out and the fused heads'
// head_w + head_b + hv, as for Act::F16 above; anything else aborts.
void launch_tower64_stream(const Tower64Args& args, uint32_t rows, int ch, bool layer_steps, hipStream_t st, hipEvent_t ev_start = nullptr,
                           hipEvent_t ev_stop = nullptr);

// ---- K1rf resident, exact f32 (dtype f32_resident; tower64_f32_kernel in kernels_t64f.hip; t64f_rule.h has the LDS plan, the step table, the
// ownership map and the layer table): the per-layer f32 tower of a <= 64-filter network in one launch, its bits ----
struct Tower64F32Args {
    const uint64_t* planes;      // [n][C][w64] bitboards, C <= 32
    const Tower64Layer* layers;  // device array [nlayers]: stem ([9][64][32] f32), then (conv1, conv2) per block ([9][64][64] f32); bias [64]; res as t64f_layer().skip
    float* out;                  // required: [rows][64] f32, the tower output, rows = boards * tower_slots(S)
    uint32_t n, C, w64, S, nlayers;
    uint32_t nch;                // 32-channel chunks a hidden layer walks: t64f_hidden_chunks (1 only where channels 32..63 are all zero)
};
// rows % 256 == 0; ch = 4: one 64-slot board per workgroup, ch = 2: 128 rows (128-slot boards always); t64f_ch has the rule.  Anything the
// arguments' comments exclude aborts.
void launch_tower64_f32(const Tower64F32Args& args, uint32_t rows, int ch, hipStream_t st, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
hipError_t prepare_tower64_f32();  // its dynamic-LDS opt-in; called by prepare_device()

// ---- K1rs resident, split precision: the whole tower of a <= 64-filter f16x2 network in one launch (see kernels.hip) ----
struct Tower64SplitLayer {
    const void* wf;     // fragment-ordered (hi, lo) weights (CONV_W_FRAG layout, cout padded to 64)
    const float* bias;  // [64 biases | 64 inverse scales]
    int res;            // 1: add the block input (second conv of a residual block)
    int nch;            // 32-channel chunks of the layer's input: 1 for the stem (planes), 2 otherwise
};
struct Tower64SplitArgs {
    const uint64_t* planes;            // [n][C][w64] bitboards, C <= 32
    const Tower64SplitLayer* layers;   // device array [nlayers]: stem, then (conv1, conv2) per block
    const float* bias_all;             // [nlayers][64 biases | 64 inverse scales]: every layer's `bias`, contiguous
    float* out;                        // optional: [rows][64] f32, the tower output, rows = boards * tower_slots(S)
    unsigned* sat;                     // the evaluator's saturation counter (ConvOpts::saturated)
    uint32_t n, C, w64, S, nlayers;
    // optional, fused K3: the two 1x1 head convs (+ folded BN + ReLU) in f32 on the resident output, written in the layout the
    // head FC kernels read (HeadsMfma::hv); head_w [32][64] f32 (value rows first, rows >= ocn zero), head_b [32]
    const float* head_w;
    const float* head_b;
    float* hv;
    uint32_t hv_pol, kvp, kpp, vhc, ocn;  // hv_pol: element offset of the policy part
};
constexpr int T64S_MAX_LAYERS = 81;  // the bias table of all layers lives in LDS (512 B per layer)
// rows % 256 == 0 (whole boards); one workgroup per board
// shape (64-slot boards): 1 = one board per workgroup (four one-tile waves), 2 = two boards per workgroup (a wave holds a
// board's 64 pixels x 32 couts); anything else = by grid size
void launch_tower64_split(const Tower64SplitArgs& args, uint32_t rows, int shape, hipStream_t st, hipEvent_t ev_start = nullptr,
                          hipEvent_t ev_stop = nullptr);
hipError_t prepare_tower64_split();  // its dynamic-LDS opt-in; called by prepare_device()

// Generic f32 NCHW direct conv for shapes the MFMA kernel does not cover (any S <= 11, any C).
// in [b][cin][hw], w [9][cout][cin], out [b][cout][hw]; same summation order as the MFMA f32 kernel.
void launch_conv3x3_generic(const float* in, const float* w, const float* bias, const float* res, float* out,
                            uint32_t b, uint32_t cin, uint32_t cout, uint32_t S, hipStream_t st,
                            hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);

// ---- K3-K5: heads on MFMA (tuned tower layout) ----------------------------------------------
// All matrices are in the tower element type `act` with K contiguous and zero-padded:
//   conv_w [32][F] (value rows, then policy rows, rest zero), conv_b [32] f32 (entries >= vhc+phc zero),
//   hv: value part [leaf][kvp] at element 0, policy part [leaf][kpp] at element hv_leaves * kvp, both stored in MFMA
//   fragment order (below; pad columns stay zero), w1 [128][kvp] and wp [round32(M)][kpp] in the same order,
//   b1 [128] f32, bp [M] f32, policy [nb][M] f32;
//   fragment order of a [rows][K] matrix (rows padded to 32): element (row, k) lives at
//     ((((row / 32) * (K / KSTEP) + k / KSTEP) * 2 + (k % KSTEP) / HALF) * 32 + row % 32) * HALF + k % HALF,
//   KSTEP = 32 bytes of k, HALF = 16 bytes: the 64 lanes' 16-byte operand pieces of one 32-row tile and one MFMA k-step
//   are one contiguous KiB, so a wave's fragment load is one fully coalesced instruction (no LDS staging, no barrier);
//   h1 [nb][128] f32 is scratch of the stand-alone FC1 (the fused FC launch keeps the hidden units in LDS).
//   kvp, kpp and F are multiples of 16 elements (the k walk reads whole 16-byte pieces).
struct HeadsMfma {
    const void* conv_w;
    const float* conv_b;
    void* hv;
    const void* w1;
    const float* b1;
    float* h1;
    const void* wp;
    const float* bp;
    float* policy;
    const float *w2, *b2;  // value FC2 [128], [1]
    float* value;          // [nb], tanh applied
    uint32_t hw, vhc, phc, kvp, kpp, M;
    uint32_t hv_leaves;    // leaf capacity of hv, a multiple of 32
    uint32_t slots;  // pixel slots per board of the tower (tower_slots)
};
void launch_heads_mfma(Act act, const void* tower, uint32_t nb, uint32_t F, const HeadsMfma& hd, hipStream_t st);
// K4c + K5c (kernels_head_chain.hip; head_chain_rule.h has the rule): launch_heads_mfma for Act::F32 with the FC pair on head_fc_chain_kernel -- one
// lane per output element (two of two leaves beyond HC_SINGLE_MAX leaves), a v_fma_f32 chain in the MFMA's k order instead of the MFMA chain: THE SAME
// BITS in policy and value.  Same operands, same hv (written by the same head conv launch, or by a resident tower when tower == nullptr), nothing
// uploaded twice.  Act::BF16 aborts: the bf16 pair has no such chain.
void launch_heads_chain(Act act, const void* tower, uint32_t nb, uint32_t F, const HeadsMfma& hd, hipStream_t st);
// the head conv launch of launch_heads_mfma alone (K3; kernels.hip)
void launch_heads_conv(Act act, const void* tower, uint32_t nb, uint32_t F, const HeadsMfma& hd, hipStream_t st);

// ---- K3-K5: heads, SIMT f32 (generic tower layout), same term order as the MFMA path ------
// Tower output addressing: element (b, k, p) at  x[b*sb + k*sk + p*sp]  (elements of type `act`).
struct TowerView {
    const void* x;
    Act act;
    uint32_t sb, sk, sp;
};
// hv[b][(oc)*hw + p] = relu(sum_k w[oc][k]*x(b,k,p) + bias[oc]) for oc < ocn (value rows first, then policy)
void launch_head_conv1x1(TowerView x, const float* w, const float* bias, uint32_t b, uint32_t F, uint32_t ocn,
                         uint32_t hw, float* hv, hipStream_t st);
// h1[b][j] = relu(sum_k w1t[k][j]*hv[b*hv_stride + k] + b1[j]), j < 128
void launch_value_fc1(const float* hv, uint32_t hv_stride, const float* w1t, const float* b1, uint32_t b, uint32_t K,
                      float* h1, hipStream_t st);
// value[b] = tanh(sum_j w2[j]*h1[b][j] + b2)
void launch_value_fc2_tanh(const float* h1, const float* w2, const float* b2, uint32_t b, float* value,
                           hipStream_t st);
// policy[b][m] = scrub(sum_k wpt[k][m]*hv[b*hv_stride + off + k] + bp[m])
// Softmax over each leaf's legal moves (net/mod.rs:100-119): idx [b][L] policy indices, cnt [b] <= L, probs [b][L].
int launch_legal_softmax(const float* policy, uint32_t M, const uint16_t* idx, const uint16_t* cnt, uint32_t L, uint32_t b,
                         float* probs, hipStream_t st);
// The same softmax on a ragged batch (legal_span.h): idx / probs [total] back to back, off [n + 1], total == off[n]; every list <= 1024
// entries (the host checks).  The same leaf and list give launch_legal_softmax's bits.  total == 0 launches nothing.
void launch_legal_softmax_ragged(const float* policy, uint32_t M, const uint16_t* idx, const uint32_t* off, uint32_t n, uint32_t total, float* probs,
                                 hipStream_t st);
void launch_policy_fc(const float* hv, uint32_t hv_stride, uint32_t off, const float* wpt, const float* bp, uint32_t b,
                      uint32_t K, uint32_t M, float* policy, hipStream_t st);
// One dense layer of SimpleTwoHeadedModel (training/cattus_train/net_utils.py:92-121), f32, the term order of every
// other dot product here: y[b][n] = epi(sum_k wt[k][n] * x[b * x_stride + k] + bias[n]); epi 0: non-finite -> f32::MIN
// (policy logits), 1: ReLU, 2: tanh.  K * 32 bytes of LDS (K <= 2048).
void launch_dense(const float* x, uint32_t x_stride, const float* wt, const float* bias, uint32_t b, uint32_t K, uint32_t N,
                  float* y, int epi, hipStream_t st);

}  // namespace cattus
