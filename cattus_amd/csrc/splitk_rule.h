// The split-K direct layer kernel (kernels_splitk.hip, K1sk), as far as it can be wrong without a GPU: how the K walk of an output tile
// is divided over the waves of a workgroup, in which order their partial sums are added, which tile a workgroup takes, and where
// everything lives in LDS.  Plain C++: host and device, no HIP call; the kernel is written with these functions and
// tests/test_splitk_rule.py runs them on the CPU.
//
//   workgroup = W waves = 1 board (64 pixel rows) x 32 couts; wave w walks the 32-channel input chunks [bound(w), bound(w + 1)), all 9
//       taps and both k-halves of each, into two 32 x 32 accumulators (pixel blocks 0 and 1)
//   W = splitk_ways(chunks): a function of the layer's input-channel count and of NOTHING else -- not of n, max_batch, the grid or the
//       device -- so the f32 summation order of an output element, and with it a leaf's bits, cannot follow the batch
//   LDS:  [ image of chunk 0 | image of chunk 1 | ... ]: the board's whole input, each chunk written by the wave that walks it; the
//       partial-sum exchange lies over the images, behind a barrier
//     image (one chunk of the board): 64 pixel rows of 144 B (K1s's row: [32 ch hi | 32 ch lo | 16 B pad]) and a zero area behind them
//       that taps off the board (and pixel slots past it) are read from, at the read's own address mod 256 (the same banks)
//     exchange: [wave][pixel 64][8 units of 4 couts, f32], the unit XORed with splitk_x_swizzle(pixel)
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SK_HD __host__ __device__ inline
#else
#define SK_HD inline
#endif

namespace cattus {

constexpr int SK_ROWS = 64, SK_COUTS = 32;  // a workgroup's tile: one board of 64 pixel slots x 32 couts
constexpr int SK_MAX_WAYS = 8;              // waves of a workgroup at most
constexpr int SK_STAGES = 18;               // weight stages of a chunk: 9 taps x 2 k-halves; stage = chunk * 18 + tap * 2 + k-half

constexpr int SK_PP = 144;                       // pixel pitch of an image: 128 B of data + 16
constexpr int SK_DZERO = SK_ROWS * SK_PP;        // behind the 64 rows: the zero area (9,216 = 36 x 256)
constexpr int SK_ZAREA = 512;                    // a redirected read keeps its address's low 8 bits: 240 + 32 (k-half) + 64 (lo) + 16 bytes, to 256
constexpr int SK_IMG = SK_DZERO + SK_ZAREA;      // 9,728 B per chunk
constexpr int SK_XROW = 128;                     // a pixel's row of the exchange: 32 couts f32
constexpr int SK_XWAVE = SK_ROWS * SK_XROW;      // a wave's partial tile: 8,192 B
constexpr int SK_LDS_MAX = 160 * 1024;
constexpr int SK_MAX_CHUNKS = SK_LDS_MAX / SK_IMG;    // 16: the whole input of a board must fit
constexpr int SK_MIN_CHUNKS = 4;
constexpr int SK_MAX_FILTERS = SK_MAX_CHUNKS * 32;    // 512: the largest (padded) filter count the LDS plan holds
static_assert(SK_DZERO % 256 == 0 && SK_IMG % 256 == 0, "the zero area keeps a read's banks only if it is 256-B aligned");
static_assert(SK_ZAREA >= 240 + 32 + 64 + 16, "a read redirected into the zero area stays inside it");
static_assert(SK_MAX_CHUNKS * SK_IMG <= SK_LDS_MAX && SK_XWAVE <= SK_IMG, "LDS sizes: a wave's exchange tile fits the image of a chunk it walked");

// ---- the K split ----
// W: 8 ways from 8 chunks (256 filters) on, 4 below; never more ways than chunks.  `forced` (CATTUS_SPLITK_WAYS, tests and A/B only):
// 1, 2, 4 or 8 replaces the rule, anything else is ignored.
SK_HD int splitk_ways(int chunks, int forced = 0) {
    int w = chunks >= 8 ? 8 : 4;
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8) w = forced;
    while (w > chunks) w >>= 1;
    return w;
}
// first chunk of wave w's range (w = ways: the chunk count): contiguous ranges, the first chunks % ways of them one chunk longer
SK_HD int splitk_bound(int chunks, int ways, int w) { return w * (chunks / ways) + (w < chunks % ways ? w : chunks % ways); }

// ---- the reduction: a pairwise tree by wave index ----
// sum(first, count) = sum(first, count / 2) + sum(first + count / 2, count / 2), sum(w, 1) = wave w's partial: for 8 ways
// ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)).  Written as a walk over `ways` slots: step s = 0 .. ways - 2 adds slot
// splitk_tree_src(ways, s) into slot splitk_tree_dst(ways, s); the result is in slot 0.
SK_HD int splitk_tree_span(int ways, int s) {  // distance between the two slots of step s: 1 for the first ways / 2 steps, then 2, ...
    int span = 1, left = ways >> 1;
    while (s >= left) s -= left, left >>= 1, span <<= 1;
    return span;
}
SK_HD int splitk_tree_dst(int ways, int s) {
    int span = 1, left = ways >> 1;
    while (s >= left) s -= left, left >>= 1, span <<= 1;
    return s * 2 * span;
}
SK_HD int splitk_tree_src(int ways, int s) { return splitk_tree_dst(ways, s) + splitk_tree_span(ways, s); }

// ---- the grid ----
// (board, cout block) with the cout block fastest, behind the XCD map of the tiled kernels (device_common.h: xcd_remap): workgroup ids go
// round the 8 XCDs, so on a grid that is a multiple of 8 every XCD gets one contiguous range of logical indices and the cout blocks of a
// board, which read the same rows, share an L2.
SK_HD uint32_t splitk_grid(uint32_t boards, uint32_t cout) { return boards * (cout / SK_COUTS); }
SK_HD int splitk_logical(int wg, int nblk) { return (nblk & 7) == 0 ? (wg & 7) * (nblk >> 3) + (wg >> 3) : wg; }
SK_HD int splitk_board(int logical, int ncb) { return logical / ncb; }  // ncb = cout / 32
SK_HD int splitk_cout_block(int logical, int ncb) { return logical % ncb; }

// ---- images (offsets from the start of LDS) ----
SK_HD int splitk_image(int chunk) { return chunk * SK_IMG; }
SK_HD int splitk_lds_bytes(int chunks) { return chunks * SK_IMG; }
// filling an image: a chunk of the board is 64 rows x 8 sixteen-byte pieces; lane l of the wave moves piece (l & 7) of row 8 i + (l >> 3),
// i = 0..7 -- eight lanes read a row's 128 contiguous bytes and write them as one ds_write_b128 group
SK_HD int splitk_piece_row(int lane, int i) { return 8 * i + (lane >> 3); }
SK_HD int splitk_piece_dst(int lane, int i) { return splitk_piece_row(lane, i) * SK_PP + (lane & 7) * 16; }
// inside an image: the row that tap (dy, dx) reads for pixel slot p of a board of edge S, plus the lane half's 16 bytes (h: channels 8 h .. 8 h
// + 7 of the k-half); a tap off the board, or a slot past it, reads the zero area at the same address mod 256.  The k-half (32 B) and the
// lo half (64 B) are added behind the redirection.
SK_HD int splitk_tap_read(int S, int p, int tap, int h) {
    const int py = p / S, px = p - py * S;
    const int hh = py + tap / 3 - 1, ww = px + tap % 3 - 1;
    const bool ok = p < S * S && hh >= 0 && hh < S && ww >= 0 && ww < S;
    const int at = (hh * S + ww) * SK_PP + h * 16;  // off the board: only its low 8 bits are used
    return ok ? at : SK_DZERO + (at & 255);
}
SK_HD int splitk_frag_offset(int khalf, int lo) { return khalf * 32 + lo * 64; }

// ---- the partial-sum exchange (offsets from the start of LDS; over the images, behind a barrier) ----
// X[wave][pixel][unit]: unit u = couts 4 u .. 4 u + 3 of the workgroup's 32 (16 bytes).  Wave w writes, per lane (pixel r = lane & 31 of
// pixel block pb, half h = lane >> 5), units 2 g + h, g = 0..3: the accumulator's elements 4 g .. 4 g + 3 are couts 8 g + 4 h .. + 3.  The
// thread that finishes item (pixel, cg) reads units 2 cg and 2 cg + 1 of every wave's tile: couts 8 cg .. 8 cg + 7.
SK_HD int splitk_x_swizzle(int pixel) { return (pixel & 7) ^ ((pixel >> 2) & 1); }
SK_HD int splitk_x(int wave, int pixel, int unit) { return wave * SK_XWAVE + pixel * SK_XROW + ((unit ^ splitk_x_swizzle(pixel)) << 4); }
// the epilogue's items: 256 of them, item = pixel * 4 + cg; thread tid takes items tid, tid + threads, ... (a wave: 16 pixels x 4 cg)
constexpr int SK_ITEMS = SK_ROWS * 4;
SK_HD int splitk_item_pixel(int item) { return item >> 2; }
SK_HD int splitk_item_cg(int item) { return item & 3; }

}  // namespace cattus
