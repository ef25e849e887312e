// The two 1x1 head convs in the tail of the resident f16 and f16r towers (cattus_hip_fused_heads: tower64_lds_tower<..., HEADS> in
// kernels.hip), as far as they can be wrong without a GPU: where the head weights, the
// biases and the tower's f32 output rows live in a workgroup's LDS, which wave and lane owns which (row, head channel) element, the k order of
// an element's chain, where the element goes in hv, and which tower plans take the setting.  Plain C++: host and device, no HIP call; the
// kernels and the evaluator are written with these functions and tests/test_head_fuse_rule.py runs them on the CPU.
//
// The arithmetic is head_conv_tile<float>'s (kernels.hip), operation for operation: per element one Mfma<float>::mac chain over the 64
// (padded) filters, k in 8-groups ascending and 0,4,1,5,2,6,3,7 inside a group, then + bias, ReLU.  Only where the operands come from
// differs: the stand-alone launch stages 256-byte row chunks from memory in LDS at a pitch of 272 bytes; here the rows never leave LDS.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "t64r_rule.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HF_HD __host__ __device__ inline
#else
#define HF_HD inline
#endif

namespace cattus {

// ---- 1. the LDS plan ----
// Head weights [32][64] f32 and staged tower rows [rows][64] f32 at a pitch of 272 bytes = 68 words: lane r of a ds_read_b128 down 32 rows
// starts at word 4 r + const (mod 64), so every group of 8 lanes covers the banks once (HG_PITCH's reasoning).  The 32 biases behind the weights.
constexpr int HF_K = 64;                       // filters (padded) = terms of a chain
constexpr int HF_CHANNELS = 32;                // head channels (padded): value rows first, rows >= ocn zero
constexpr int HF_PITCH = HF_K * 4 + 16;        // 272
constexpr int HF_W_BYTES = HF_CHANNELS * HF_PITCH;  // 8,704
constexpr int HF_B_BYTES = HF_CHANNELS * 4;         // 128
constexpr int HF_SLAB = 3 * 64 * 128;          // one weight slab of the resident towers' ring (V2_SLAB)
struct HfLds {
    int w, b;        // first byte of the head weights, of the biases
    int rows;        // first byte of the tower's output rows
    int rows_bytes;  // their extent: f32 rows at HF_PITCH, written by the last layer's epilogue
};
// The f16 family (dtype f16 under tower_form resident, f16r_resident): tower64_lds_bytes(ch, ls) is [ring | two activation buffers].
//   !ls: the ring is 3 slabs, step t in slot t % 3, and every layer has 3 steps: the last step reads slot 2.  Whoever has passed the last
//        step's barrier finds slots 0 and 1 dead (their readers waited for their ds_reads ahead of that barrier, the loaders issue nothing
//        more): 48 KiB for 8,832 + 128 rows x 272 = 43,648 bytes.
//    ls: the ring is two halves of 3 slabs, layer l in half l & 1.  A tower has 1 + 2 blocks layers, so the last layer reads half 0, and
//        behind its barrier half 1 is dead: 72 KiB for 8,832 + 64 rows x 272 = 26,240 bytes.
HF_HD constexpr HfLds hf_lds_t64(int ch, bool ls) {
    const int base = ls ? 3 * HF_SLAB : 0;
    return HfLds{base, base + HF_W_BYTES, base + HF_W_BYTES + HF_B_BYTES, (256 / ch) * HF_PITCH};
}
// byte offsets inside the regions: element (head channel i, filter k) of the weights, (row, channel) of the staged rows
HF_HD constexpr int hf_w_offset(int i, int k) { return i * HF_PITCH + k * 4; }
HF_HD constexpr int hf_row_offset(int row, int channel) { return row * HF_PITCH + channel * 4; }
// what a fragment read of Mfma<float> takes for stage u (0..7) in lane half h: 16 bytes = k 8 u + 4 h + j in element j
HF_HD constexpr int hf_w_frag(int i, int u, int h) { return hf_w_offset(i, u * 8 + h * 4); }
HF_HD constexpr int hf_row_frag(int row, int u, int h) { return hf_row_offset(row, u * 8 + h * 4); }
// the operands' way into LDS: thread t (0..255: the four loader waves) copies 16-byte pieces t and t + 256 of the [32][64] f32 weights --
// piece q is row q >> 4, filters 4 (q & 15) .. + 3 -- and, t < 32, bias t
constexpr int HF_STAGE_THREADS = 256;
HF_HD constexpr int hf_piece_dst(int q) { return hf_w_offset(q >> 4, (q & 15) * 4); }

// ---- 2. the ownership map ----
// A 32-row tile of the workgroup's 256 / ch rows belongs to one consumer wave: ch = 2, wave w has tile w (the towers' row block w >> 1,
// pixel block w & 1); ch = 4, the wave of each pixel block that holds cout block 0 (waves 0 and 2).  Element e (0..15) of lane `lane` is
// (row, head channel) -- the accumulator layout of a 32x32 MFMA with the head weights as operand A.
HF_HD constexpr int hf_tiles(int ch) { return 256 / ch / 32; }
HF_HD constexpr int hf_tile_of_wave(int ch, int wave) {  // -1: the wave has none
    return wave < 0 || wave >= 4 ? -1 : ch == 2 ? wave : (wave & 1) ? -1 : wave >> 1;
}
struct HfOwn {
    int row;      // 0 .. 256 / ch - 1
    int channel;  // 0 .. 31
};
HF_HD constexpr HfOwn hf_own(int ch, int wave, int lane, int e) {
    return HfOwn{hf_tile_of_wave(ch, wave) * 32 + (lane & 31), (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)};
}

// ---- 3. the chain ----
// term t (0..63) of an element's chain multiplies the operands at k = hf_term_k(t): stage t >> 3, MFMA (t & 7) >> 1 of the stage, lane half t & 1
HF_HD constexpr uint32_t hf_term_k(uint32_t t) { return (t & ~7u) + ((t & 1u) << 2) + ((t & 7u) >> 1); }

// ---- 4. where an element goes ----
// hv (kernels.h, HeadsMfma): the value part [leaf][kvp] at element 0, the policy part [leaf][kpp] at hv_pol, both in f32 MFMA fragment order
struct HfHead {
    uint32_t hw, vhc, ocn, kvp, kpp, hv_pol, slots;  // pixels of a board; value channels; value + policy channels; ...; pixel slots per board
};
HF_HD constexpr size_t hf_packed_f32(uint32_t row, uint32_t k, uint32_t K) {  // frag_packed_index<float>
    return ((((size_t)(row >> 5) * (K / 8) + k / 8) * 2 + (k % 8) / 4) * 32 + (row & 31)) * 4 + k % 4;
}
// tower row `grow` (board grow / slots, pixel slot grow % slots) of a pass of n leaves, head channel i: written at all?  (head_conv_tile:
// rows of the n leaves only, p < hw, i < ocn)
HF_HD constexpr bool hf_writes(const HfHead& H, uint32_t n, uint32_t grow, uint32_t i) { return grow / H.slots < n && grow % H.slots < H.hw && i < H.ocn; }
HF_HD constexpr size_t hf_hv_index(const HfHead& H, uint32_t grow, uint32_t i) {
    const uint32_t bb = grow / H.slots, p = grow % H.slots;
    return i < H.vhc ? hf_packed_f32(bb, i * H.hw + p, H.kvp) : H.hv_pol + hf_packed_f32(bb, (i - H.vhc) * H.hw + p, H.kpp);
}

// ---- 5. who takes the setting ----
// The resident f16 towers, whose last layer leaves f32 rows for a head conv launch of its own.  The bf16 and f16x2 resident towers run the
// head convs in their tails already, unconditionally.  The resident f32 tower (tower64_f32_kernel) does not take it: its body is the
// __global__ function itself, and moving it into a function that a HEADS instance could share changes the code the compiler makes of the
// instances that exist (measured on the build: 1,308 against 1,340 instructions at CH = 4 from wrapping alone) -- the default path must not
// move, so that tower keeps its head conv launch.  Every other plan has no resident output.
enum class HfPlan { Other, Resident64Bf16, Resident64F16, Resident64Split, Resident64Stream, Resident64F32 };
HF_HD constexpr bool hf_takes(HfPlan p) { return p == HfPlan::Resident64F16 || p == HfPlan::Resident64Stream; }

}  // namespace cattus
