// gfx950 kernels of the Cattus leaf evaluator: the resident exact-f32 tower (K1rf, dtype f32_resident).  See kernels.hip for the per-layer
// kernel it is bit-identical to (conv3x3_mfma_v2_kernel<float>) and for the bf16 / f16 resident tower it is modelled on.
#include "kernels.h"
#include "device_common.h"

#include <hip/hip_ext.h>

#include <cstdio>
#include <cstdlib>

namespace cattus {

// ------------------------------------------------------------------------------------------
// K1rf resident: the whole f32 tower of a <= 64-filter network in ONE launch, activations stay in LDS
// ------------------------------------------------------------------------------------------
//
// The f32 counterpart of tower64_lds_kernel.  A 64-channel f32 row is two 128-byte chunks, so a 256-row workgroup's two activation
// buffers would not fit beside the weight ring; at 64 or 128 rows they do (t64f_rule.h, the LDS plan: 107,008 / 139,776 B).  The workgroup
// expands its boards' bitboard planes into chunk 0 of buffer 1, then runs the stem and two convs per residual block with the stream X in
// buffer 0 and a block's middle M in buffer 1, streaming only the weights: waves 4-7 run conv3x3_mfma_v2_kernel's LDS-DMA ring (3 slabs of
// [3 taps][64 cout][128 B]) two steps ahead across layer boundaries, waves 0-3 are MFMA consumers.  A step is one slab, (layer, 32-channel
// chunk, kernel row); one s_barrier per step orders the ring and, at a layer boundary, a wave's LDS writes against its neighbours' reads.
// Per output element the operations are the per-layer f32 kernel's in its order -- one Mfma<float>::mac chain over chunk -> dy -> dx ->
// k-slice, + bias, + skip, ReLU, zero off the board -- so the results are its bits (tests/test_f32_resident_gpu.py).  No rounding, no
// clamp, no counter.  The epilogue writes the accumulator layout straight into the other buffer: a lane's four consecutive couts are one
// 16-byte slot of the row (t64f_lds_offset), which is what the next layer's fragment read takes.
// nch (a kernel argument): chunks a hidden layer walks -- 2, or 1 on a network of at most 32 filters (t64f_rule.h, the step table).
// CH = 4: 64 rows = one 64-slot board, wave w owns the 32 pixels of half w>>1 and the 32 couts of half w&1 (one tile).
// CH = 2: 128 rows, wave w owns row block w>>1 and the 32 couts of half w&1 (1x2 tiles); BIG: the 128 rows are one 128-slot board.
template <int CH, bool BIG>
__global__ void __launch_bounds__(512) tower64_f32_kernel(Tower64F32Args A) {
    static_assert(CH == 2 || CH == 4, "128 or 64 rows per workgroup");
    static_assert(!(BIG && CH == 4), "a 128-slot board needs 128 rows in one workgroup");
    typedef Mfma<float>::frag frag;
    constexpr int ROWS = t64f_rows(CH), NPB = t64f_npb(CH);
    constexpr T64fLds LDS = t64f_lds(CH);
    static_assert(LDS.total <= T64F_LDS_MAX && LDS.buf[0] % 256 == 0 && LDS.buf[1] % 256 == 0 && LDS.zero_off % 256 == 0,
                  "off-board reads keep their row's banks only if the zero areas are 256-B aligned");
    constexpr int SLOTS_PER_BOARD = BIG ? 128 : 64;
    constexpr int WPL = T64F_PIECES / 4;  // weight pieces per loader wave and step
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const bool is_loader = wave >= 4;
    const int S = (int)A.S;
    const int row0 = blockIdx.x * ROWS;
    const int nlayers = (int)A.nlayers, nch = (int)A.nch;
    const int T_total = t64f_steps(nlayers, nch);
    // The layer table through a constant-address-space pointer: a row's fetch is then a scalar load.  As a vector load it would count in
    // vmcnt, and the loaders' wait for it would drain the slab they keep in flight across the barrier.
    typedef const __attribute__((address_space(4))) Tower64Layer* layer_table;
    const layer_table layers = (layer_table)A.layers;

    if (tid < 32) reinterpret_cast<f32x4*>(smem + LDS.buf[tid >> 4] + LDS.zero_off)[tid & 15] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the loader waves put the first two weight slabs on their way before they help with the plane expansion
    const int lw = wave - 4;
    auto issue_w = [&](int s) {  // weight slab of step s -> ring slot s % 3
        const T64fStep st = t64f_step(s, nch);
        const int rb = t64f_row_bytes(st.layer);
        const char* src = reinterpret_cast<const char*>(layers[st.layer].w) + t64f_slab_src(st);
        char* dst = smem + LDS.ring + t64f_ring_slot(s) * T64F_SLAB;
#pragma unroll
        for (int i = 0; i < WPL; i++) glds16(src + t64f_piece_src(lw * WPL + i, lane, rb), dst + t64f_piece_dst(lw * WPL + i));
    };
    if (is_loader) {
        issue_w(0);
        if (T_total > 1) issue_w(1);
    }

    // ---- stem input: bitboard planes -> chunk 0 of buffer 1, [row][32 ch] f32, 1.0 where the plane has the pixel's bit ----
    {
        const int hw = S * S;
        const uint32_t cslots = (A.C + 3) / 4;  // 16-byte channel groups that hold a real plane
        constexpr int ITEMS = ROWS * 8 / 512;   // (row, channel group) pairs per thread
        typedef const __attribute__((address_space(1))) uint64_t* gu64p;
        // all plane words first (one round trip to memory for the whole expansion), then the rows
        uint64_t words[ITEMS][4];
#pragma unroll
        for (int it = 0; it < ITEMS; it++) {
            const int v = tid + it * 512;
            const int row = v >> 3, sl = v & 7;
            const uint32_t grow = (uint32_t)(row0 + row);
            const uint32_t board = grow / SLOTS_PER_BOARD, px = grow % SLOTS_PER_BOARD;
            const bool live = (uint32_t)sl < cslots && board < A.n && (int)px < hw;
            const gu64p pl = (gu64p)(A.planes + (size_t)(live ? board : 0) * A.C * A.w64 + (live ? (px >> 6) : 0));
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t c = sl * 4 + i;
                words[it][i] = (live && c < A.C) ? pl[(size_t)c * A.w64] : 0ull;
            }
        }
#pragma unroll
        for (int it = 0; it < ITEMS; it++) {
            const int v = tid + it * 512;
            const int row = v >> 3, sl = v & 7;
            const uint32_t px = (uint32_t)(row0 + row) % SLOTS_PER_BOARD;
            f32x4 vals;
#pragma unroll
            for (int i = 0; i < 4; i++) vals[i] = ((words[it][i] >> (px & 63)) & 1ull) ? 1.0f : 0.0f;
            *reinterpret_cast<f32x4*>(smem + LDS.buf[T64F_LDS_M] + t64f_lds_offset(CH, row, sl * 4)) = vals;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // written before this wave's first barrier
    }

    if (is_loader) {
        // ================================ loader waves: the weight stream ================================
        for (int s = 0; s < T_total; s++) {
            // step s's slab was issued two steps ago; only the slab of step s+1 may still be in flight
            if (s + 1 < T_total) wait_vm_barrier<WPL>();
            else wait_vm_barrier<0>();
            if (s + T64F_AHEAD < T_total) issue_w(s + T64F_AHEAD);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    }

    // ================================ consumer waves ================================
    const int r = lane & 31, h = lane >> 5;
    const int rb = CH == 2 ? wave >> 1 : 0;   // 64-row block of this wave
    const int pb0 = CH == 4 ? wave >> 1 : 0;  // first 32-pixel block of this wave inside its row block
    const int coutb = (wave & 1) * 32;        // first output channel of this wave
    const int pslot0 = BIG ? (rb & 1) * 64 : 0;
    const int board_row = BIG ? 0 : rb * 64;  // first workgroup row of this wave's board
    // Activation fragment addresses, relative to the input buffer (t64f_tap): per (kernel row, tap column, pixel block) the byte offset of the
    // shifted pixel's row in chunk 0 (the buffer's zero area off the board) and the row's swizzle term; `onb` has a bit per on-board tap, which
    // alone moves on to chunk 1.  They depend on nothing but the lane, so they are made once; a step adds buffer and chunk.
    bool pvalid[NPB];
    int rel[3][3][NPB], swz[3][3][NPB];
    unsigned onb = 0;
#pragma unroll
    for (int pb = 0; pb < NPB; pb++) {
        const int p = pslot0 + (pb0 + pb) * 32 + r;
        pvalid[pb] = p < S * S;
#pragma unroll
        for (int g = 0; g < 3; g++)
#pragma unroll
            for (int dxi = 0; dxi < 3; dxi++) {
                const T64fTap tap = t64f_tap(CH, S, board_row, p, g, dxi);
                rel[g][dxi][pb] = tap.rel;
                swz[g][dxi][pb] = (h ^ tap.swz) << 4;
                onb |= tap.ok ? 1u << ((g * 3 + dxi) * NPB + pb) : 0u;
            }
    }
    int aaddr[4];  // weight fragment address per k-slice: ring slot and tap are immediates
#pragma unroll
    for (int ks = 0; ks < 4; ks++) aaddr[ks] = LDS.ring + t64f_wfrag_offset(0, coutb + r, ks, h);

    // fragments are read AHEAD stages before the MFMAs that use them; a stage is NPB x 4 MFMAs
    constexpr int AHEAD = 3, RING = AHEAD + 1;
    int opaque = 0;
    const uint32_t blocks = t64f_blocks((uint32_t)nlayers);
    for (int layer = 0; layer < nlayers; layer++) {
        const float* const lbias = layers[layer].bias;
        const T64fLayer rl = t64f_layer((uint32_t)layer, blocks);
        const int ibase = LDS.buf[0] + rl.reads * (LDS.buf[1] - LDS.buf[0]);
        const int obase = LDS.buf[0] + rl.writes * (LDS.buf[1] - LDS.buf[0]);
        // through a global pointer: as FLAT loads these would count in lgkmcnt and every wait for an LDS fragment would have to be lgkmcnt(0)
        typedef const __attribute__((address_space(1))) f32x4* gf32x4p;
        const gf32x4p gbias = (gf32x4p)(lbias + coutb + h * 4);
        f32x4 biasv[4];
#pragma unroll
        for (int g = 0; g < 4; g++) biasv[g] = gbias[g * 2];
        f32x16 acc[NPB];
#pragma unroll
        for (int j = 0; j < NPB; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[j][e] = 0.0f;

        const int lch = t64f_layer_chunks(layer, nch);
        for (int chunk = 0; chunk < lch; chunk++) {
            const int cadd = chunk * LDS.chunk_stride;
#pragma unroll
            for (int g = 0; g < 3; g++) {
                // fragment reads of the previous step and (at a layer boundary) the previous layer's output writes are done before anybody
                // passes: the loaders may reuse the slab, the neighbours may read the rows
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                asm volatile("" : "+v"(opaque));  // keeps the per-step addresses from being hoisted out of the loops
                const int wslab = g * T64F_SLAB;  // every layer has a multiple of 3 steps: the ring slot of (layer, chunk, g) is g
                int baddr[3][NPB][4];
#pragma unroll
                for (int dxi = 0; dxi < 3; dxi++)
#pragma unroll
                    for (int pb = 0; pb < NPB; pb++) {
                        const bool on = (onb >> ((g * 3 + dxi) * NPB + pb)) & 1u;
                        const int rowa = ibase + rel[g][dxi][pb] + (on ? cadd : 0) + opaque;
#pragma unroll
                        for (int ks = 0; ks < 4; ks++) baddr[dxi][pb][ks] = rowa + (swz[g][dxi][pb] ^ (ks << 5));
                    }
                frag fa[RING], fb[RING][NPB];
                auto load_stage = [&](int i, frag& a, frag (&b)[NPB]) {
                    const int dxi = i >> 2, ks = i & 3;
                    a = *reinterpret_cast<const frag*>(smem + aaddr[ks] + (wslab + dxi * T64F_TAP_BYTES));
#pragma unroll
                    for (int pb = 0; pb < NPB; pb++) b[pb] = *reinterpret_cast<const frag*>(smem + baddr[dxi][pb][ks]);
                };
#pragma unroll
                for (int i = 0; i < AHEAD; i++) load_stage(i, fa[i % RING], fb[i % RING]);
                __builtin_amdgcn_sched_group_barrier(0x100, (1 + NPB) * AHEAD, 0);
#pragma unroll
                for (int i = 0; i < 12; i++) {
                    if (i + AHEAD < 12) load_stage(i + AHEAD, fa[(i + AHEAD) % RING], fb[(i + AHEAD) % RING]);
#pragma unroll
                    for (int pb = 0; pb < NPB; pb++) Mfma<float>::mac(fa[i % RING], fb[i % RING][pb], acc[pb]);
                    // pin the issue order: this stage's look-ahead reads, then its MFMAs
                    if (i + AHEAD < 12) __builtin_amdgcn_sched_group_barrier(0x100, 1 + NPB, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, NPB * 4, 0);
                }
            }
        }

        // ---- layer epilogue: + bias (+ block input), ReLU, zero off the board; into the other buffer, or (last layer) f32 rows to memory ----
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int lane_now = lane + opaque;  // (0: keeps the addresses below out of the layer loop's live registers)
        f32x4 rv[NPB][4];
        if (rl.skip) {  // the block input lives in the buffer being overwritten: the lane's own elements, all read first
#pragma unroll
            for (int pb = 0; pb < NPB; pb++)
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const T64fOwn own = t64f_own(CH, wave, lane_now, pb, g * 4);
                    rv[pb][g] = *reinterpret_cast<const f32x4*>(smem + obase + t64f_lds_offset(CH, own.row, own.channel));
                }
        }
#pragma unroll
        for (int pb = 0; pb < NPB; pb++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const T64fOwn own = t64f_own(CH, wave, lane_now, pb, g * 4);  // elements 4g .. 4g + 3: four consecutive channels
                f32x4 yv;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    float v = acc[pb][g * 4 + q] + biasv[g][q];
                    if (rl.skip) v = v + rv[pb][g][q];
                    float y = v > 0.0f ? v : 0.0f;
                    if (!pvalid[pb]) y = 0.0f;
                    yv[q] = y;
                }
                if (rl.last) *reinterpret_cast<f32x4*>(A.out + t64f_out_index((size_t)row0, own)) = yv;
                else *reinterpret_cast<f32x4*>(smem + obase + t64f_lds_offset(CH, own.row, own.channel)) = yv;
            }
    }
}

// Every instance that exists, f(kernel, LDS bytes, CH, BIG): one board per workgroup (CH = 4) on 64-slot boards only.
template <class F>
static void for_each_tower64_f32(F&& f) {
    each_int<2, 4>([&](auto ch) { each_bool([&](auto big) {
        constexpr int CH = decltype(ch)::value;
        constexpr bool BIG = decltype(big)::value;
        if constexpr (!(CH == 4 && BIG)) f(&tower64_f32_kernel<CH, BIG>, t64f_lds(CH).total, ch, big);
    }); });
}

void launch_tower64_f32(const Tower64F32Args& args, uint32_t rows, int ch, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop) {
    const bool want_big = tower_slots(args.S) == 128;
    const int want_ch = ch == 4 && !want_big ? 4 : 2;
    if (!args.out || (args.nch != 1 && args.nch != 2) || args.C > 32 || rows % 256 != 0) {
        fprintf(stderr, "cattus: launch_tower64_f32: needs Tower64F32Args::out, nch 1 or 2, at most 32 planes and whole 256-row groups\n");
        abort();
    }
    for_each_tower64_f32([&](auto kernel, int lds, auto c, auto big) {
        if (c == want_ch && big == want_big) hipExtLaunchKernelGGL(kernel, dim3(rows / t64f_rows(c)), dim3(512), lds, st, ev_start, ev_stop, 0, args);
    });
}

hipError_t prepare_tower64_f32() {
    hipError_t err = hipSuccess;
    for_each_tower64_f32([&](auto kernel, int lds, auto...) { lds_opt_in(err, kernel, lds); });
    return err;
}

}  // namespace cattus
