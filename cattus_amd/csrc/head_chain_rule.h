// The short-chain form of the f32 FC pair (value FC1 + FC2 + tanh and the policy FC on head_fc_chain_kernel, kernels_head_chain.hip), as
// far as it can be wrong without a GPU: which (leaf, output unit) a thread produces, where its operands live, the order of its fmaf
// chain and what it does to the sum.  Plain C++: host and device, no HIP call; the kernel and the evaluator are written with these
// functions and tests/test_head_chain_rule.py runs them on the CPU.
//
// Why a second kernel: head_fc_pair_kernel<float> gives a wave one 32 x 32 tile and ONE accumulator, so its K walk is a single dependent
// chain of v_mfma_f32_32x32x2_f32 -- 64 cycles for 2 k.  A dependent v_fma_f32 chain costs 4 cycles per k, and an f32 MFMA is, per output
// element, an fmaf chain.  So a lane that walks one output element's chain in the MFMA's order gives the same bits eight times faster per
// k; what it gives up is the matrix pipe, which a head of a small net does not fill anyway.
//
// The contract (kernels.hip, kperm): a dot product runs over the PADDED K (a multiple of 16; pad terms are 0 * 0, and fmaf(0, 0, acc)
// is acc for every acc this chain can hold: it starts at +0 and a sum that is -0 needs a -0 product behind a -0 sum) in 8-groups
// ascending, k = 0,4,1,5,2,6,3,7 inside a group, accumulator +0.0f at the start, one fmaf per term, nothing split, nothing reassociated.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "tap_layout.h"  // tap_frag_index: the fragment-packed layout hv, w1t and wpt already have

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HC_HD __host__ __device__ inline
#else
#define HC_HD inline
#endif

namespace cattus {

// ---- 1. the grid map ----
// A workgroup is HC_THREADS lanes = HC_UNITS output units of `nl` leaves: thread t owns unit strip * 128 + t of each of its nl leaves
// (nl independent chains that share the thread's weight loads; a chain is never split).  blockIdx.x = 0 is the value FC1 (its 128
// hidden units are exactly one workgroup, which therefore also finishes FC2 + tanh through LDS), blockIdx.x = 1 + strip the policy FC;
// blockIdx.y counts groups of nl leaves.
constexpr uint32_t HC_THREADS = 128, HC_UNITS = 128, HC_HIDDEN = 128;
// Leaves per lane.  One up to HC_SINGLE_MAX leaves: the grid of the one-output form is n * (1 + strips) workgroups, and for the widest
// head the project runs (chess, 1880 moves: 1 + 15 strips) 16 leaves are 256 workgroups -- one per CU, so a second chain per lane would
// only make every lane's walk twice as long.  Two beyond: half the weight bytes through the vector memory path per fmaf.
constexpr uint32_t HC_SINGLE_MAX = 16;
HC_HD uint32_t hc_leaves_per_lane(uint32_t n) { return n <= HC_SINGLE_MAX ? 1u : 2u; }
HC_HD uint32_t hc_strips(uint32_t M) { return (M + HC_UNITS - 1) / HC_UNITS; }
HC_HD uint32_t hc_grid_x(uint32_t M) { return 1 + hc_strips(M); }
HC_HD uint32_t hc_grid_y(uint32_t n, uint32_t nl) { return (n + nl - 1) / nl; }

enum : uint32_t { HC_FC1 = 0, HC_POLICY = 1 };
struct HcOut {
    uint32_t part;  // HC_FC1 / HC_POLICY
    uint32_t leaf, unit;
    bool live;      // leaf < n and unit < J: the thread stores this output (a dead one is computed on clamped operands and dropped)
};
HC_HD uint32_t hc_part_units(uint32_t part, uint32_t M) { return part == HC_FC1 ? HC_HIDDEN : M; }
HC_HD HcOut hc_map(uint32_t bx, uint32_t by, uint32_t tid, uint32_t slot, uint32_t nl, uint32_t n, uint32_t M) {
    HcOut o;
    o.part = bx == 0 ? HC_FC1 : HC_POLICY;
    o.leaf = by * nl + slot;
    o.unit = (bx == 0 ? 0 : (bx - 1) * HC_UNITS) + tid;
    o.live = o.leaf < n && o.unit < hc_part_units(o.part, M);
    return o;
}
// what a dead output loads instead (every load is unconditional: a load under a branch serialises the look-ahead)
HC_HD uint32_t hc_load_leaf(uint32_t leaf, uint32_t n) { return leaf < n ? leaf : n - 1; }
HC_HD uint32_t hc_load_row(uint32_t unit, uint32_t J) { return unit < J ? unit : J - 1; }

// ---- 2. operand offsets ----
// A step is one 8-group of k; its two 16-byte pieces (h = 0: k = 8u .. 8u + 3, h = 1: k = 8u + 4 .. 8u + 7) of row `row` of a [rows][K]
// matrix in fragment order.  Consecutive rows of a 32-row tile are consecutive 16 bytes; a step is 1 KiB per tile, a half 512 bytes.
constexpr uint32_t HC_STEP_K = 8;
HC_HD uint32_t hc_steps(uint32_t K) { return K / HC_STEP_K; }
HC_HD size_t hc_piece_index(uint32_t row, uint32_t u, uint32_t h, uint32_t K) { return tap_frag_index(row, HC_STEP_K * u + 4 * h, K, 4); }
constexpr size_t HC_STEP_STRIDE = 256, HC_HALF_STRIDE = 128;  // elements between a row's pieces of steps u, u + 1 / of halves 0, 1
// the policy part of hv behind the value part (kernels.h, HeadsMfma)
HC_HD size_t hc_hv_policy_at(uint32_t hv_leaves, uint32_t kvp) { return (size_t)hv_leaves * kvp; }

// ---- 3. the walk ----
// term t of the chain, 0 <= t < K, multiplies the operands at k = hc_term_k(t)
HC_HD constexpr uint32_t hc_term_k(uint32_t t) { return (t & ~7u) + ((t & 1u) << 2) + ((t & 7u) >> 1); }
// one step on the four pieces (a: the leaf's, b: the weight row's; anything indexable by 0..3): terms 8u .. 8u + 7
template <class V>
HC_HD float hc_step(float acc, const V& a0, const V& a1, const V& b0, const V& b1) {
    acc = __builtin_fmaf(a0[0], b0[0], acc);
    acc = __builtin_fmaf(a1[0], b1[0], acc);
    acc = __builtin_fmaf(a0[1], b0[1], acc);
    acc = __builtin_fmaf(a1[1], b1[1], acc);
    acc = __builtin_fmaf(a0[2], b0[2], acc);
    acc = __builtin_fmaf(a1[2], b1[2], acc);
    acc = __builtin_fmaf(a0[3], b0[3], acc);
    acc = __builtin_fmaf(a1[3], b1[3], acc);
    return acc;
}
// the whole chain of (row_a of a) . (row_b of b), both fragment-packed [rows][K]: what a lane computes, piece by piece
HC_HD float hc_dot(const float* a, uint32_t row_a, const float* b, uint32_t row_b, uint32_t K) {
    float acc = 0.0f;
    for (uint32_t u = 0; u < hc_steps(K); u++) {
        const float* a0 = a + hc_piece_index(row_a, u, 0, K);
        const float* b0 = b + hc_piece_index(row_b, u, 0, K);
        acc = hc_step(acc, a0, a0 + HC_HALF_STRIDE, b0, b0 + HC_HALF_STRIDE);
    }
    return acc;
}

// ---- 4. the epilogues, of one element ----
HC_HD float hc_fc1_epilogue(float acc, float bias) {
    const float y = acc + bias;
    return y > 0.0f ? y : 0.0f;
}
// non-finite logits -> f32::MIN (reference: engine/src/net/mod.rs:56-61)
HC_HD float hc_policy_epilogue(float acc, float bias) {
    const float y = acc + bias;
    return !(__builtin_fabsf(y) <= 3.40282347e+38f) ? -3.40282347e+38f : y;
}
// value FC2: the 128-term chain over a leaf's hidden units (plain order in memory), then + b2; the caller applies tanh_exact
HC_HD float hc_fc2_sum(const float* w2, const float* hidden, float b2) {
    float acc = 0.0f;
    for (uint32_t t = 0; t < HC_HIDDEN; t++) {
        const uint32_t k = hc_term_k(t);
        acc = __builtin_fmaf(w2[k], hidden[k], acc);
    }
    return acc + b2;
}

// ---- 5. LDS ----
// A workgroup keeps its nl leaves' activations (the part it walks, in plain k order: [slot][K]) and, for FC1, their hidden units
// ([slot][128]) in LDS.  K <= 32 channels x 121 pixels, so this never passes 64 KiB.
HC_HD uint32_t hc_lds_hidden_at(uint32_t nl, uint32_t kvp, uint32_t kpp) { return nl * (kvp > kpp ? kvp : kpp); }  // in floats
HC_HD uint32_t hc_lds_bytes(uint32_t nl, uint32_t kvp, uint32_t kpp) { return (hc_lds_hidden_at(nl, kvp, kpp) + nl * HC_HIDDEN) * 4; }
constexpr uint32_t HC_LDS_MAX = 65536;

}  // namespace cattus
