// The f32-operand Winograd F(2x2, 3x3) layer kernel (kernels_wino_f32.hip, K1wf, dtype f32w), as far as it can be wrong without a GPU:
// which tile a workgroup takes, which items of the input transform a thread takes, where everything lives in LDS, where a stage of U
// lives in its buffer, the two transforms in the kernel's operation order, the order of an accumulator's chain and the epilogue.
// Plain C++: host and device, no HIP call; the kernel is written with these functions, tests/test_wino_f32_rule.py runs them on the
// CPU and tests/wino_f32_layer_ref.cpp restates a whole layer with them, bit for bit.
//
//   workgroup = 4 waves = 2 boards (32 tiles of 2x2 outputs, 128 pixel rows) x NCB blocks of 32 couts (NCB = 1 or 2: wf32_ncb);
//       wave q owns frequency row q (f = 4 q + l) of every cout block: 4 NCB accumulators of 32 x 32
//   a STEP is 16 channels = two 8-channel groups = half a 32-channel chunk: 32 NCB v_mfma_f32_32x32x2_f32 per wave between two barriers
//   LDS:  [ V image 0 | V image 1 | chunk buffer 0 | chunk buffer 1 ]; the epilogue's exchange lies over V image 0
//     V image (one step): [f 16][tile 32][8 ch of group 0 | 8 ch of group 1 | 16 B pad], f32 -- K1wh's image byte for byte (pitch 80 B)
//     chunk buffer (32 channels of the 128 pixel rows, f32): K1w's image -- pixel pitch 144 B, board rows of 8 pixels + 64 B, a zero
//       area behind the 16 board rows that patch pixels off the board are read from, at the read's own address mod 256 (the same banks)
//     exchange (one cout block at a time): [frequency row q][c' 2][tile 32][8 units of 4 couts, f32], the unit XORed with bits 1..3
//       of the tile
//   U: f32(G g G^T), no scale, [cout / 32][8-channel group x 16 + f][lane][4 f32] -- 1 KiB per stage (frag_index.h: wino_f32_frag_index)
//
// The arithmetic, which tests/wino_f32_layer_ref.cpp restates with std::fmaf:
//   V = B^T d B in f32: wf32_bt down the patch's columns, then along its rows
//   M[f][cout][tile] starts at 0 and takes acc = fmaf(U, V, acc) over the input channels in the order wf32_chain_channel gives: chunks
//       ascending, in a chunk the 8-channel groups ascending, in a group the four MFMAs of Mfma<float>::mac, MFMA i multiplying channels
//       8 g + i and 8 g + 4 + i, in that order (the instruction chains its two k in issue order, as the exact f32 tower relies on)
//   Z = M A along a frequency row (wf32_at, left to right), Y = A^T Z down the rows (wf32_at), then wf32_finish: Y + bias, + skip, ReLU
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "frag_index.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WF32_HD __host__ __device__ inline
#else
#define WF32_HD inline
#endif

namespace cattus {

constexpr int WF32_BOARDS = 2, WF32_TILES = 32, WF32_ROWS = 128;  // a workgroup's boards; its couts are 32 NCB
constexpr int WF32_THREADS = 256;
constexpr int WF32_CUS = 256;  // the grid size from which a workgroup takes two cout blocks (wf32_ncb)
constexpr int WF32_UD = 2;     // steps of U in registers: the one being multiplied and the next (a step is 2,048 NCB MFMA cycles long)

constexpr int WF32_STEP = 16;                 // input channels of a step: two 8-channel groups
constexpr int WF32_STAGE = 1024;              // one (8-channel group, frequency) of a cout block: 64 lanes x 4 f32
constexpr int WF32_VP = 80;                   // a tile's row of a V image: 8 ch of group 0 (32 B) | 8 ch of group 1 (32 B) | 16 B pad
constexpr int WF32_VGROUP = 32;               // from a tile's group 0 to its group 1
constexpr int WF32_VF = WF32_TILES * WF32_VP; // one frequency
constexpr int WF32_VIMG = 16 * WF32_VF;       // one step's V: 40,960 B
constexpr int WF32_PP = 144;                  // pixel pitch of a chunk image: 128 B of data + 16
constexpr int WF32_DHALF = 64;                // from a pixel's channels 0..15 (the chunk's first step) to its channels 16..31 (its second)
constexpr int WF32_RP = 8 * WF32_PP + 64;     // pitch of a board row
constexpr int WF32_DZERO = 16 * WF32_RP;      // behind the 16 board rows: the zero area
constexpr int WF32_ZAREA = 512;               // a redirected read keeps its address's low 8 bits: 255 + a half's 64 + 8 bytes, to 256
constexpr int WF32_DBUF = WF32_DZERO + WF32_ZAREA;  // 19,968 B
constexpr int WF32_LDS_V = 0;                       // the two V images
constexpr int WF32_LDS_D = 2 * WF32_VIMG;           // the two chunk buffers
constexpr int WF32_LDS_TOTAL = WF32_LDS_D + 2 * WF32_DBUF;  // 121,856 B
constexpr int WF32_ZROW = 128;                              // a tile's row of the exchange: 32 couts f32
constexpr int WF32_LDS_Z = 4 * 2 * WF32_TILES * WF32_ZROW;  // the exchange: 32,768 B, over V image 0
static_assert(WF32_DZERO % 256 == 0 && WF32_DBUF % 256 == 0 && WF32_LDS_D % 256 == 0, "the zero area keeps a read's banks only if it is 256-B aligned");
static_assert(WF32_ZAREA >= 255 + 64 + 8, "a read redirected into the zero area stays inside it");
static_assert(WF32_LDS_Z <= WF32_VIMG && WF32_LDS_TOTAL <= 160 * 1024, "LDS sizes");

// ---- the grid ----
// Cout blocks per workgroup: two (64 couts: one input transform serves twice the MFMAs) once that grid still gives each of the 256 CUs a
// workgroup, one below.  A function of the padded batch and the layer's width alone; the choice does not enter an element's value (an
// accumulator is the same chain of MFMAs either way).
WF32_HD int wf32_ncb(uint32_t bpad, uint32_t cout) { return (bpad / WF32_BOARDS) * (cout / 64) >= (uint32_t)WF32_CUS ? 2 : 1; }
// (board pair, cout group) with the cout group fastest, behind the XCD map of the tiled kernels (device_common.h: xcd_remap): workgroup
// ids go round the 8 XCDs, so on a grid that is a multiple of 8 every XCD gets one contiguous range of logical indices and the cout
// groups of a board pair, which read the same rows, share an L2.
WF32_HD uint32_t wf32_grid(uint32_t bpad, uint32_t cout, int ncb) { return (bpad / WF32_BOARDS) * (cout / (32 * (uint32_t)ncb)); }
WF32_HD int wf32_logical(int wg, int nblk) { return (nblk & 7) == 0 ? (wg & 7) * (nblk >> 3) + (wg >> 3) : wg; }
WF32_HD int wf32_pair(int logical, int ngroups) { return logical / ngroups; }        // ngroups = cout / (32 NCB)
WF32_HD int wf32_cout_group(int logical, int ngroups) { return logical % ngroups; }

// ---- U: byte offset of the stage (8-channel group g, frequency f) of 32-cout block cb32; ngr = cin / 8 groups; lane l's fragment
// (the four channels 8 g + 4 (l >> 5) .. + 3 of cout 32 cb32 + (l & 31)) at + 16 l ----
WF32_HD size_t wf32_u_stage(int cb32, int ngr, int g, int f) { return (((size_t)cb32 * ngr + g) * 16 + f) * WF32_STAGE; }

// ---- the order of an accumulator's chain: the n-th fmaf of a layer of cin channels multiplies this input channel ----
// chunks ascending, 8-channel groups ascending, and in a group Mfma<float>::mac's k order 0, 4, 1, 5, 2, 6, 3, 7
WF32_HD int wf32_chain_channel(int n) { return (n & ~7) + ((n & 1) << 2) + ((n >> 1) & 3); }

// ---- the input transform's items: thread -> (tile, channel pair chp of the step's 8); one item per thread and step ----
// A 32-lane half of a wave takes 16 (tile, 16-byte slot) combinations x the slot's two channel pairs, chosen so that BOTH its patch
// reads (8 B each, out of a chunk buffer) and its V writes (8 B each) fall on 32 different pairs of banks:
//   * a patch pixel of tile (ty, tx) lies at 128 (ty & 1) + 32 tx (mod 256) whatever the board: eight tiles u = 4 ty + tx that differ
//     mod 8 fill the even or the odd 16-byte slots of a 256-byte bank row, so half of the lanes read slot 2 sp and half slot 2 sp + 1;
//   * tile t's V row starts at slot 5 t (mod 16): the eight tiles u that read slot 2 sp and the eight that read slot 2 sp + 1 are
//     picked (u = j or j + 8) so that {5 u} and {5 u + 1} together are all sixteen slots.
// half wave hw = tid >> 5: board hw >> 2, slot pair sp = (hw >> 1) & 1, and the complementary tile choice for odd hw.
// Tile tt = board tt >> 4, tile row (tt >> 2) & 3, tile column tt & 3.
WF32_HD int wf32_item_tile(int tid) {
    const int hw = tid >> 5, j = (tid >> 1) & 7, sel = (tid >> 4) & 1, compl_ = hw & 1;
    const int high = sel ? ((j >= 3 ? 1 : 0) ^ compl_) : compl_;
    return (hw >> 2) * 16 + high * 8 + j;
}
WF32_HD int wf32_item_chp(int tid) { return ((((tid >> 6) & 1) * 2 + ((tid >> 4) & 1)) << 1) + (tid & 1); }

// ---- V images (offsets from the start of LDS) ----
WF32_HD int wf32_v_image(int img) { return WF32_LDS_V + img * WF32_VIMG; }
// inside an image: where item (tile, chp) puts frequency f's pair of f32 values (8 bytes)
WF32_HD int wf32_v_write(int f, int tile, int chp) { return f * WF32_VF + tile * WF32_VP + chp * 8; }
// inside an image: the MFMA B fragment of a lane for group g -- tile lane & 31, channels 8 g + 4 (lane >> 5) .. + 3 (16 bytes)
WF32_HD int wf32_v_read(int f, int lane, int g) { return f * WF32_VF + (lane & 31) * WF32_VP + g * WF32_VGROUP + (lane >> 5) * 16; }

// ---- chunk buffers ----
WF32_HD int wf32_chunk_buffer(int buf) { return WF32_LDS_D + buf * WF32_DBUF; }
// a chunk = 128 pixel rows x 8 sixteen-byte pieces; thread tid moves piece (tid & 7) of pixel row 32 i + (tid >> 3), i = 0..3: a wave
// instruction reads eight whole 128-byte rows
WF32_HD int wf32_piece_row(int tid, int i) { return 32 * i + (tid >> 3); }
WF32_HD int wf32_pixel_offset(int row) { return (row >> 3) * WF32_RP + (row & 7) * WF32_PP; }  // row = board * 64 + y * 8 + x
WF32_HD int wf32_piece_dst(int tid, int i) { return wf32_pixel_offset(wf32_piece_row(tid, i)) + (tid & 7) * 16; }
// inside a buffer: patch pixel (i, j) of the item's tile, its channel pair of the chunk's half `half` (8 bytes); a pixel off the board
// is read from the zero area at the same address mod 256 (the half's 64 bytes are added behind the redirection: the kernel keeps the
// sixteen offsets of half 0 and adds the half)
WF32_HD int wf32_patch_read(int tile, int chp, int i, int j, int half) {
    const int board = tile >> 4, ty = (tile >> 2) & 3, tx = tile & 3;
    const int y = 2 * ty - 1 + i, x = 2 * tx - 1 + j;
    const int at = (board * 8 + y) * WF32_RP + x * WF32_PP + chp * 8;  // off the board: only its low 8 bits are used
    return (y >= 0 && y < 8 && x >= 0 && x < 8 ? at : WF32_DZERO + (at & 255)) + half * WF32_DHALF;
}

// ---- the epilogue's exchange (offsets from the start of LDS) ----
// Z[q][c'][tile][unit]: unit u = couts 4 u .. 4 u + 3 of the cout block's 32 (16 bytes).  Wave q writes the rows of its 32 tiles (lane =
// tile lane & 31, units 2 g + (lane >> 5)); the wave that finishes tile row r reads, per lane, unit (lane & 7) of the tile its pixel
// belongs to, out of three frequency rows.
WF32_HD int wf32_z(int q, int c, int tile, int unit) { return ((q * 2 + c) * WF32_TILES + tile) * WF32_ZROW + ((unit ^ ((tile >> 1) & 7)) << 4); }
// the finishing wave r's output rows: lane = (pixel k * 8 + (lane >> 3) of its 32, unit lane & 7), k = 0..3; pixel p = board p >> 4,
// output row 2 r + ((p >> 3) & 1), column p & 7 -- eight lanes cover a row's 128 bytes
WF32_HD int wf32_out_pixel(int lane, int k) { return k * 8 + (lane >> 3); }
WF32_HD int wf32_out_row(int r, int p) { return (p >> 4) * 64 + (2 * r + ((p >> 3) & 1)) * 8 + (p & 7); }  // row inside the workgroup's 128
WF32_HD int wf32_out_tile(int r, int p) { return (p >> 4) * 16 + r * 4 + ((p & 7) >> 1); }

// ---- the transforms, in the kernel's operation order (T: float, or a vector of floats) ----
// B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1], applied down the patch's columns, then along its rows: V = B^T d B
template <class T>
WF32_HD void wf32_bt(const T d0, const T d1, const T d2, const T d3, T& o0, T& o1, T& o2, T& o3) {
    o0 = d0 - d2, o1 = d1 + d2, o2 = d2 - d1, o3 = d1 - d3;
}
// A^T = [1 1 1 0; 0 1 -1 -1]: Z = M A along a frequency row, Y = A^T Z down the rows; left to right
template <class T>
WF32_HD void wf32_at(const T m0, const T m1, const T m2, const T m3, T& y0, T& y1) {
    y0 = m0 + m1 + m2, y1 = m1 - m2 - m3;
}
// G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1]: U = G g G^T (the host's float64 transform, weight_layout.h: wino_transform)
template <class T>
WF32_HD void wf32_g(const T g0, const T g1, const T g2, T& u0, T& u1, T& u2, T& u3) {
    u0 = g0, u1 = 0.5 * g0 + 0.5 * g1 + 0.5 * g2, u2 = 0.5 * g0 - 0.5 * g1 + 0.5 * g2, u3 = g2;
}
// ---- the epilogue behind Y: + bias, then + skip, then ReLU as the f32 tower writes it (x > 0 ? x : 0: -0 and NaN become +0) ----
WF32_HD float wf32_finish(float y, float bias, bool has_skip, float skip) {
    float x = y + bias;
    if (has_skip) x = x + skip;
    return x > 0.0f ? x : 0.0f;
}

}  // namespace cattus
