// gfx950 kernels of the Cattus leaf evaluator, part 8: the direct 3x3 split-precision conv with the K walk DIVIDED over the waves of a
// workgroup (K1sk), for batches of a few leaves.
//
// conv3x3_splitw_kernel (kernels.hip, K1s') gives every consumer wave all of K for its 32 x 32 tile: at 256 filters 8 chunks x 18 stages
// x 3 terms = 432 dependent MFMAs, while a batch of 8 leaves puts 32 workgroups on 256 CUs.  This kernel computes the same layer on a
// tile of one board x 32 couts, with the chunks of the K walk dealt out to W waves (splitk_rule.h: W and the ranges follow from the
// input-channel count alone), and adds the W partial accumulators in f32, in one fixed order, through LDS.
//   workgroup = W waves = 1 board (64 pixel rows) x 32 couts.  Grid = boards x (cout / 32) behind xcd_remap's map.
//   weights: K1s''s buffer and fragment order ([cout / 32][stage][hi | lo][lane][8 f16]); a chunk's 18 stages are 36 KiB of contiguous
//       global memory, loaded into registers a whole chunk ahead with ordinary loads.
//   activations: the wave copies the 64 x 128 B of each chunk of its range global -> registers -> LDS into that chunk's own image (K1s's
//       144-byte rows and zero area); only the wave itself reads it: no barrier inside the K walk.
//   per chunk 18 stages of (4 ds_read_b128, 6 MFMAs) in K1s's order: taps in row order, two k-halves per tap, per stage w_lo a_hi,
//       w_hi a_lo, w_hi a_hi.
//   reduction: barrier, every wave writes its two accumulators into the exchange (over the images), barrier; thread (pixel, cg) then
//       reads the W partials of its 8 couts and adds them as a pairwise tree by wave index, and runs K1s's epilogue (finish_f16x2_sums)
//       on the sum.  With one way the sum is the one partial: conv3x3_splitw_kernel's bits.
// No cross-workgroup synchronisation, no atomics on floating-point data.  A FIRST BUILD: plain loads, no hand-placed waits beside the two barriers.
#include "kernels.h"
#include "device_common.h"
#include "splitk_rule.h"

#include <hip/hip_ext.h>

namespace cattus {

static_assert(SK_PP == SP, "the image's pixel pitch is the split tower's LDS row pitch");
static_assert(SK_STAGES * 2 * 1024 == 18 * SW_STAGE, "a chunk's weight stages");

// the pairwise tree over the partials of waves FIRST .. FIRST + COUNT - 1 (splitk_rule.h: sum(first, count), the order that the walk of
// splitk_tree_dst / _src spells out), one 16-byte unit of a pixel's row
template <int FIRST, int COUNT>
__device__ __forceinline__ f32x4 splitk_tree(const char* smem, int pixel, int unit) {
    if constexpr (COUNT == 1) {
        return *reinterpret_cast<const f32x4*>(smem + splitk_x(FIRST, pixel, unit));
    } else {
        const f32x4 a = splitk_tree<FIRST, COUNT / 2>(smem, pixel, unit);
        const f32x4 b = splitk_tree<FIRST + COUNT / 2, COUNT / 2>(smem, pixel, unit);
        return a + b;
    }
}
template <int N>
__device__ __forceinline__ void splitk_tree_sum(float (&v)[8], const char* smem, int pixel, int cg) {
    const f32x4 lo = splitk_tree<0, N>(smem, pixel, 2 * cg), hi = splitk_tree<0, N>(smem, pixel, 2 * cg + 1);
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = lo[j], v[4 + j] = hi[j];
}

template <bool HAS_RES>
__global__ void __launch_bounds__(SK_MAX_WAYS * 64, 1)
    conv3x3_splitk_kernel(const _Float16* __restrict__ in, const _Float16* __restrict__ wf, const float* __restrict__ bias,
                          const _Float16* __restrict__ res, _Float16* __restrict__ out, unsigned* __restrict__ sat, int cin, int cout, int S,
                          int flags) {
    typedef _Float16 T;
    typedef Mfma<T>::frag frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ways = __builtin_amdgcn_readfirstlane(nthreads >> 6);
    const int lane = tid & 63;

    const int ncb = cout >> 5;
    const int logical = splitk_logical((int)blockIdx.x, (int)gridDim.x);
    const int cout0 = splitk_cout_block(logical, ncb) * SK_COUTS;  // the workgroup's 32 output channels
    const size_t row0 = (size_t)splitk_board(logical, ncb) * SK_ROWS;  // first tower row of its board

    const int nch = cin >> 5;  // 32-channel chunks
    const int c0 = splitk_bound(nch, ways, wave), c1 = splitk_bound(nch, ways, wave + 1);  // this wave's range
    const uint32_t row_bytes = (uint32_t)cin * 4;

    // ---- the epilogue's operands of this thread's first item, requested ahead of everything else ----
    const int item0 = tid;
    f32x4 bias8[2], ds8[2];
    T resv0[16] = {};
    {
        const int cg = splitk_item_cg(item0 & (SK_ITEMS - 1));
#pragma unroll
        for (int q = 0; q < 2; q++) {
            bias8[q] = *reinterpret_cast<const f32x4*>(bias + cout0 + cg * 8 + q * 4);
            ds8[q] = *reinterpret_cast<const f32x4*>(bias + cout + cout0 + cg * 8 + q * 4);
        }
        if (HAS_RES && item0 < SK_ITEMS) {
            const size_t off = (row0 + splitk_item_pixel(item0)) * ((size_t)cout * 2) + sp_col(cout0 + cg * 8);
            reinterpret_cast<f32x4*>(resv0)[0] = *reinterpret_cast<const f32x4*>(res + off);
            reinterpret_cast<f32x4*>(resv0)[1] = *reinterpret_cast<const f32x4*>(res + off + 32);
        }
    }

    // ---- the images of this wave's chunks: global -> registers -> LDS, and their zero areas ----
    const char* abase = reinterpret_cast<const char*>(in) + row0 * row_bytes;
    uint32_t asrc[8];
    int adst[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        asrc[i] = (uint32_t)splitk_piece_row(lane, i) * row_bytes + (lane & 7) * 16;
        adst[i] = splitk_piece_dst(lane, i);
    }
    auto fetch_image = [&](u32x4(&a)[8], int ch) {
#pragma unroll
        for (int i = 0; i < 8; i++) a[i] = *reinterpret_cast<const u32x4*>(abase + (size_t)ch * 128 + asrc[i]);
    };
    auto store_image = [&](const u32x4(&a)[8], int ch) {
        char* img = smem + splitk_image(ch);
#pragma unroll
        for (int i = 0; i < 8; i++) *reinterpret_cast<u32x4*>(img + adst[i]) = a[i];
        if (lane < SK_ZAREA / 16) *reinterpret_cast<u32x4*>(img + SK_DZERO + lane * 16) = u32x4{0u, 0u, 0u, 0u};
    };

    // ---- weights: a chunk's 18 stages x (hi, lo) fragments in registers ----
    const char* wblk = reinterpret_cast<const char*>(wf) + (size_t)(cout0 >> 5) * nch * SK_STAGES * SW_STAGE + lane * 16;
    u32x4 wr[SK_STAGES][2];
    auto fetch_stage = [&](int ch, int j) {
        const char* p = wblk + ((size_t)ch * SK_STAGES + j) * SW_STAGE;
        wr[j][0] = *reinterpret_cast<const u32x4*>(p);
        wr[j][1] = *reinterpret_cast<const u32x4*>(p + 1024);
    };

    {
        // the first two images and the first chunk's weights travel together
        u32x4 a0[8], a1[8];
        fetch_image(a0, c0);
        const bool two = c0 + 1 < c1;
        if (two) fetch_image(a1, c0 + 1);
#pragma unroll
        for (int j = 0; j < SK_STAGES; j++) fetch_stage(c0, j);
        store_image(a0, c0);
        if (two) store_image(a1, c0 + 1);
    }
    for (int ch = c0 + 2; ch < c1; ch++) {  // longer ranges: only under a forced way count
        u32x4 a[8];
        fetch_image(a, ch);
        store_image(a, ch);
    }

    const int r = lane & 31, h = lane >> 5;
    int rowa[9][2];
#pragma unroll
    for (int pb = 0; pb < 2; pb++)
#pragma unroll
        for (int t9 = 0; t9 < 9; t9++) rowa[t9][pb] = splitk_tap_read(S, pb * 32 + r, t9, h);

    f32x16 acc[2];
#pragma unroll
    for (int pb = 0; pb < 2; pb++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[pb][e] = 0.0f;

    // one chunk = 18 stages; LAST: the range's final chunk (nothing to fetch behind it)
    auto chunk = [&](int ch, auto last_tag) {
        constexpr bool LAST = decltype(last_tag)::value;
        const char* img = smem + splitk_image(ch);
#pragma unroll
        for (int j = 0; j < SK_STAGES; j++) {
            const int t9 = j >> 1, k = j & 1;
            frag ph[2], pl[2];
#pragma unroll
            for (int pb = 0; pb < 2; pb++) {
                ph[pb] = *reinterpret_cast<const frag*>(img + rowa[t9][pb] + splitk_frag_offset(k, 0));
                pl[pb] = *reinterpret_cast<const frag*>(img + rowa[t9][pb] + splitk_frag_offset(k, 1));
            }
            const frag wh = __builtin_bit_cast(frag, wr[j][0]);
            const frag wl = __builtin_bit_cast(frag, wr[j][1]);
#pragma unroll
            for (int pb = 0; pb < 2; pb++) {
                Mfma<T>::mac(wl, ph[pb], acc[pb]);
                Mfma<T>::mac(wh, pl[pb], acc[pb]);
                Mfma<T>::mac(wh, ph[pb], acc[pb]);
            }
            if (!LAST) fetch_stage(ch + 1, j);  // the next chunk's stage j, a chunk ahead
        }
    };
    for (int ch = c0; ch + 1 < c1; ch++) chunk(ch, std::false_type{});
    chunk(c1 - 1, std::true_type{});

    // ---- reduction and epilogue ----
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // every wave is out of the images: the exchange lies over them
#pragma unroll
    for (int pb = 0; pb < 2; pb++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = acc[pb][g * 4 + i];
            *reinterpret_cast<f32x4*>(smem + splitk_x(wave, pb * 32 + r, g * 2 + h)) = v;
        }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // every wave's partial tile is written
    for (int item = item0; item < SK_ITEMS; item += nthreads) {
        const int px = splitk_item_pixel(item), cg = splitk_item_cg(item);  // cg is the same for all of a thread's items (threads % 4 == 0)
        float v[8];
        switch (ways) {
            case 1: splitk_tree_sum<1>(v, smem, px, cg); break;
            case 2: splitk_tree_sum<2>(v, smem, px, cg); break;
            case 4: splitk_tree_sum<4>(v, smem, px, cg); break;
            default: splitk_tree_sum<8>(v, smem, px, cg); break;
        }
        T resv[16];
#pragma unroll
        for (int j = 0; j < 16; j++) resv[j] = resv0[j];
        if (HAS_RES && item != item0) {
            const size_t off = (row0 + px) * ((size_t)cout * 2) + sp_col(cout0 + cg * 8);
            reinterpret_cast<f32x4*>(resv)[0] = *reinterpret_cast<const f32x4*>(res + off);
            reinterpret_cast<f32x4*>(resv)[1] = *reinterpret_cast<const f32x4*>(res + off + 32);
        }
        finish_f16x2_sums<1, HAS_RES>(v, ds8, bias8, resv, px < S * S, flags, sat, out, row0 + px, cout, cout0 + cg * 8);
    }
}

// Both instances, f(kernel, HAS_RES).
template <class F>
static void for_each_splitk(F&& f) {
    each_bool([&](auto r) { f(&conv3x3_splitk_kernel<decltype(r)::value>, r); });
}

bool splitk_supported(uint32_t cin, uint32_t cout, uint32_t S) {
    return S <= 8 && cin % 64 == 0 && cout % 64 == 0 && cin >= 128 && cout >= 128 && cin <= (uint32_t)SK_MAX_FILTERS && cout <= (uint32_t)SK_MAX_FILTERS;
}

void launch_conv3x3_splitk(const void* in, const void* wf, const float* bias, const void* res, void* out, uint32_t boards, uint32_t cin, uint32_t cout,
                           uint32_t S, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop, int flags, int forced_ways, unsigned* sat) {
    typedef _Float16 H;
    if (!splitk_supported(cin, cout, S) || !sat) {
        fprintf(stderr, "cattus: launch_conv3x3_splitk: unsupported layer (cin %u, cout %u, board %u)\n", cin, cout, S);
        abort();
    }
    const int chunks = (int)cin / 32, ways = splitk_ways(chunks, forced_ways);
    const dim3 grid(splitk_grid(boards, cout));
    for_each_splitk([&](auto kernel, auto r) {
        if (r == (res != nullptr))
            hipExtLaunchKernelGGL(kernel, grid, dim3(ways * 64), splitk_lds_bytes(chunks), st, ev_start, ev_stop, 0, (const H*)in, (const H*)wf, bias,
                                  (const H*)res, (H*)out, sat, (int)cin, (int)cout, (int)S, flags);
    });
}

hipError_t prepare_splitk() {
    hipError_t err = hipSuccess;
    for_each_splitk([&](auto kernel, auto) { lds_opt_in(err, kernel, splitk_lds_bytes(SK_MAX_CHUNKS)); });
    return err;
}

}  // namespace cattus
