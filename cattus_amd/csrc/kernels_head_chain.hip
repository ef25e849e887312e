// K4c + K5c: the f32 FC pair of the heads -- value FC1 + FC2 + tanh and the policy FC -- as v_fma_f32 chains, one output element per lane
// (head_chain_rule.h has the grid map, the operand offsets, the walk order and the epilogues; this file is written with them).
//
// head_fc_pair_kernel<float> (kernels.hip) walks K as ONE dependent chain of v_mfma_f32_32x32x2_f32 per wave: 64 cycles for 2 k, 25 k
// cycles for the K = 784 of hex7 with 16 head channels, while nearly every CU idles.  An f32 MFMA is, per output element, an fmaf chain
// in a fixed order (Mfma<float>::mac: k = 0,4,1,5,2,6,3,7 of an 8-group); a lane that walks that chain with v_fma_f32 pays 4 cycles per k
// and produces the same bits.  The work is small (128 leaves x 177 outputs x 784 k = 18 M fma), so the vector ALUs of the CUs the grid
// reaches are enough.  cattus_hip_head_chain (include/cattus_hip.h) turns it on per evaluator; profiles/head_chain.txt has the numbers.
//
// A workgroup = 128 lanes = 128 output units (the hidden units of FC1, or a strip of moves) of NL leaves:
//   * the leaves' activations (NL x K floats of hv) go to LDS once, in plain k order, and every lane reads them from there with
//     same-address (broadcast) ds_read_b128 -- the loop's only global loads are the lane's own weight row;
//   * the weight row is read as the 16-byte pieces the fragment-packed layout already has -- lanes of consecutive rows read consecutive
//     16 bytes at one k-group -- straight from L2 into a register ring HC_AHEAD steps ahead;
//   * the walk is unrolled in straight-line groups of HC_GROUP steps with unconditional loads (a step beyond K re-reads the last one
//     and its fmafs are skipped), as in head_fc_tile_packed and for its reason: with loads in flight around a loop's back edge, or under
//     a branch, the compiler waits for all of them.  The empty asm statement at a group's head is a compiler fence that pins this: no
//     load of a group may be hoisted above it, over the back edge; it emits no instruction.
//   * NL = 2: the two leaves' chains are independent and share the weight pieces; a chain is never split.
// The FC1 workgroup holds all 128 hidden units of its leaves: it stages them in LDS and finishes FC2 + tanh, as block column 0 of
// head_fc_pair_kernel does.
#include "kernels.h"
#include "device_common.h"

#include <cstdio>
#include <cstdlib>

namespace cattus {

constexpr int HC_AHEAD = 16;  // steps in flight per lane: 2 x 4 VGPRs each; 16 steps are 512 (NL = 1) or 1024 cycles of fmaf
constexpr int HC_GROUP = 64;  // steps per straight-line group (512 k): K = 784 is two groups

struct HeadChainArgs {
    const float* hv;  // fragment-packed: the value part [hv_leaves][kvp] at element 0, the policy part [hv_leaves][kpp] at hv_pol
    const float *w1, *wp;  // fragment-packed [128][kvp], [round32(M)][kpp]
    const float *b1, *bp, *w2, *b2;
    float *policy, *value;
    uint32_t n, M, kvp, kpp, hv_pol, hidden_at;
};

template <int NL>
__global__ void __launch_bounds__(HC_THREADS) head_fc_chain_kernel(HeadChainArgs A) {
    extern __shared__ __attribute__((aligned(16))) float hc_lds[];
    const uint32_t tid = threadIdx.x, bx = blockIdx.x, by = blockIdx.y;
    const bool fc1 = bx == 0;
    const uint32_t K = fc1 ? A.kvp : A.kpp, J = hc_part_units(fc1 ? HC_FC1 : HC_POLICY, A.M);
    const float* __restrict__ P = A.hv + (fc1 ? 0 : A.hv_pol);
    const float* __restrict__ Q = fc1 ? A.w1 : A.wp;
    HcOut out[NL];
#pragma unroll
    for (int s = 0; s < NL; s++) out[s] = hc_map(bx, by, tid, s, NL, A.n, A.M);
    const uint32_t row = hc_load_row(out[0].unit, J), nsteps = hc_steps(K);
    const float bias_j = (fc1 ? A.b1 : A.bp)[row];  // requested now: its round trip is not paid after the last fmaf
    // the leaves' activations to LDS, [slot][K] in plain k order: piece q of a leaf is step q / 2, half q % 2
    const uint32_t ppl = K / 4;  // 16-byte pieces per leaf
    f32x4* const lds4 = reinterpret_cast<f32x4*>(hc_lds);
    for (uint32_t q = tid; q < NL * ppl; q += HC_THREADS) {
        const uint32_t s = q / ppl, pq = q - s * ppl;
        const uint32_t leaf = hc_load_leaf(by * NL + s, A.n);
        lds4[s * ppl + pq] = *reinterpret_cast<const f32x4*>(P + hc_piece_index(leaf, pq >> 1, pq & 1, K));
    }
    __syncthreads();

    const float* wq = Q + hc_piece_index(row, 0, 0, K);
    f32x4 ring[HC_AHEAD][2];
    auto fetch = [&](int slot, uint32_t u) {
        const float* at = wq + (size_t)min(u, nsteps - 1) * HC_STEP_STRIDE;
        ring[slot][0] = *reinterpret_cast<const f32x4*>(at);
        ring[slot][1] = *reinterpret_cast<const f32x4*>(at + HC_HALF_STRIDE);
    };
    float acc[NL];
#pragma unroll
    for (int s = 0; s < NL; s++) acc[s] = 0.0f;
    for (uint32_t u0 = 0; u0 < nsteps; u0 += HC_GROUP) {
        asm volatile("" ::: "memory");  // compiler fence: a group's loads stay inside the group (see above)
        const uint32_t left = nsteps - u0;  // > 0
#pragma unroll
        for (int s = 0; s < HC_AHEAD; s++) fetch(s, u0 + s);
#pragma unroll
        for (int q = 0; q < HC_GROUP; q++) {
            const uint32_t uc = min(u0 + q, nsteps - 1);
            f32x4 a[NL][2];
#pragma unroll
            for (int s = 0; s < NL; s++) {
                a[s][0] = lds4[s * ppl + 2 * uc];
                a[s][1] = lds4[s * ppl + 2 * uc + 1];
            }
            if ((uint32_t)q < left) {
#pragma unroll
                for (int s = 0; s < NL; s++) acc[s] = hc_step(acc[s], a[s][0], a[s][1], ring[q % HC_AHEAD][0], ring[q % HC_AHEAD][1]);
            }
            if (q + HC_AHEAD < HC_GROUP) fetch(q % HC_AHEAD, u0 + q + HC_AHEAD);
        }
    }

    if (fc1) {
        // every lane is a hidden unit (unit = tid < 128): [slot][128] to LDS, then one lane per leaf finishes the value head
        float* hidden = hc_lds + A.hidden_at;
#pragma unroll
        for (int s = 0; s < NL; s++) hidden[s * HC_HIDDEN + tid] = hc_fc1_epilogue(acc[s], bias_j);
        __syncthreads();
        const uint32_t leaf = by * NL + tid;
        if (tid < NL && leaf < A.n) A.value[leaf] = tanh_exact(hc_fc2_sum(A.w2, hidden + tid * HC_HIDDEN, A.b2[0]));
    } else {
#pragma unroll
        for (int s = 0; s < NL; s++)
            if (out[s].live) A.policy[(size_t)out[s].leaf * A.M + out[s].unit] = hc_policy_epilogue(acc[s], bias_j);
    }
}

void launch_heads_chain(Act act, const void* tower, uint32_t nb, uint32_t F, const HeadsMfma& hd, hipStream_t st) {
    const uint32_t nl = hc_leaves_per_lane(nb), lds = hc_lds_bytes(nl, hd.kvp, hd.kpp);
    if (act != Act::F32 || lds > HC_LDS_MAX) {
        fprintf(stderr, "launch_heads_chain: f32 heads of at most %u bytes of LDS only (act %d, %u bytes)\n", HC_LDS_MAX, (int)act, lds);
        abort();
    }
    launch_heads_conv(act, tower, nb, F, hd, st);  // K3 as it is: writes hv
    if (!nb) return;
    HeadChainArgs a{};
    a.hv = static_cast<const float*>(hd.hv), a.w1 = static_cast<const float*>(hd.w1), a.wp = static_cast<const float*>(hd.wp);
    a.b1 = hd.b1, a.bp = hd.bp, a.w2 = hd.w2, a.b2 = hd.b2, a.policy = hd.policy, a.value = hd.value;
    a.n = nb, a.M = hd.M, a.kvp = hd.kvp, a.kpp = hd.kpp;
    a.hv_pol = (uint32_t)hc_hv_policy_at(hd.hv_leaves, hd.kvp), a.hidden_at = hc_lds_hidden_at(nl, hd.kvp, hd.kpp);
    const dim3 grid(hc_grid_x(hd.M), hc_grid_y(nb, nl)), block(HC_THREADS);
    if (nl == 1)
        hipLaunchKernelGGL(head_fc_chain_kernel<1>, grid, block, lds, st, a);
    else
        hipLaunchKernelGGL(head_fc_chain_kernel<2>, grid, block, lds, st, a);
}

}  // namespace cattus
