// The single-term f16 Winograd F(2x2, 3x3) layer kernel (kernels_wino_f16.hip, K1wh), as far as it can be wrong without a GPU: which
// tile a workgroup takes, which items of the input transform a thread takes, where everything lives in LDS, where a stage of U lives in
// its buffer, and the two transforms in the kernel's operation order.  Plain C++: host and device, no HIP call; the kernel is written
// with these functions and tests/test_wino_f16_rule.py runs them on the CPU.
//
//   workgroup = 4 waves = 2 boards (32 tiles of 2x2 outputs, 128 pixel rows) x NCB blocks of 32 couts (NCB = 1 or 2: wf16_ncb);
//       wave q owns frequency row q (f = 4 q + l) of every cout block: 4 NCB accumulators of 32 x 32
//   a STEP is one 32-channel chunk = two k-steps of 16 channels: 8 NCB MFMAs per wave between two barriers
//   LDS:  [ V image 0 | V image 1 | chunk buffer 0 | chunk buffer 1 ]; the epilogue's exchange lies over V image 0
//     V image (one step): [f 16][tile 32][16 ch of k-half 0 | 16 ch of k-half 1 | 16 B pad], f16 -- the pitch (80 B) of K1w's image
//     chunk buffer (32 channels of the 128 pixel rows, f32): K1w's image -- pixel pitch 144 B, board rows of 8 pixels + 64 B, a zero
//       area behind the 16 board rows that patch pixels off the board are read from, at the read's own address mod 256 (the same banks)
//     exchange (one cout block at a time): [frequency row q][c' 2][tile 32][8 units of 4 couts, f32], the unit XORed with bits 1..3
//       of the tile
//   U: f16(U 2^s) alone, [cout / 32][k-step x 16 + f][lane][8 f16] -- 1 KiB per stage (frag_index.h: wino_f16_frag_index)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "frag_index.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WF16_HD __host__ __device__ inline
#else
#define WF16_HD inline
#endif

namespace cattus {

constexpr int WF16_BOARDS = 2, WF16_TILES = 32, WF16_ROWS = 128;  // a workgroup's boards; its couts are 32 NCB
constexpr int WF16_THREADS = 256;
constexpr int WF16_CUS = 256;  // the grid size from which a workgroup takes two cout blocks (wf16_ncb)
constexpr int WF16_UD = 3;     // steps of U in registers: the one being multiplied and two on their way

constexpr int WF16_STAGE = 1024;              // one (k-step, frequency) of a cout block: 64 lanes x 8 f16
constexpr int WF16_VP = 80;                   // a tile's row of a V image: 16 ch of k-half 0 (32 B) | 16 ch of k-half 1 (32 B) | 16 B pad
constexpr int WF16_VHALF = 32;                // from a tile's k-half 0 to its k-half 1
constexpr int WF16_VF = WF16_TILES * WF16_VP; // one frequency
constexpr int WF16_VIMG = 16 * WF16_VF;       // one step's V: 40,960 B
constexpr int WF16_PP = 144;                  // pixel pitch of a chunk image: 128 B of data + 16
constexpr int WF16_DHALF = 64;                // from a pixel's channels 0..15 to its channels 16..31
constexpr int WF16_RP = 8 * WF16_PP + 64;     // pitch of a board row
constexpr int WF16_DZERO = 16 * WF16_RP;      // behind the 16 board rows: the zero area
constexpr int WF16_ZAREA = 512;               // a redirected read keeps its address's low 8 bits: 255 + a half's 64 + 8 bytes, to 256
constexpr int WF16_DBUF = WF16_DZERO + WF16_ZAREA;  // 19,968 B
constexpr int WF16_LDS_V = 0;                       // the two V images
constexpr int WF16_LDS_D = 2 * WF16_VIMG;           // the two chunk buffers
constexpr int WF16_LDS_TOTAL = WF16_LDS_D + 2 * WF16_DBUF;  // 121,856 B
constexpr int WF16_ZROW = 128;                              // a tile's row of the exchange: 32 couts f32
constexpr int WF16_LDS_Z = 4 * 2 * WF16_TILES * WF16_ZROW;  // the exchange: 32,768 B, over V image 0
static_assert(WF16_DZERO % 256 == 0 && WF16_DBUF % 256 == 0 && WF16_LDS_D % 256 == 0, "the zero area keeps a read's banks only if it is 256-B aligned");
static_assert(WF16_ZAREA >= 255 + 64 + 8, "a read redirected into the zero area stays inside it");
static_assert(WF16_LDS_Z <= WF16_VIMG && WF16_LDS_TOTAL <= 160 * 1024, "LDS sizes");

// ---- the grid ----
// Cout blocks per workgroup: two (64 couts: one input transform serves twice the MFMAs) once that grid still gives each of the 256 CUs a
// workgroup, one below.  A function of the padded batch and the layer's width alone; the choice does not enter an element's value (an
// accumulator is the same chain of MFMAs either way).
WF16_HD int wf16_ncb(uint32_t bpad, uint32_t cout) { return (bpad / WF16_BOARDS) * (cout / 64) >= (uint32_t)WF16_CUS ? 2 : 1; }
// (board pair, cout group) with the cout group fastest, behind the XCD map of the tiled kernels (device_common.h: xcd_remap): workgroup
// ids go round the 8 XCDs, so on a grid that is a multiple of 8 every XCD gets one contiguous range of logical indices and the cout
// groups of a board pair, which read the same rows, share an L2.
WF16_HD uint32_t wf16_grid(uint32_t bpad, uint32_t cout, int ncb) { return (bpad / WF16_BOARDS) * (cout / (32 * (uint32_t)ncb)); }
WF16_HD int wf16_logical(int wg, int nblk) { return (nblk & 7) == 0 ? (wg & 7) * (nblk >> 3) + (wg >> 3) : wg; }
WF16_HD int wf16_pair(int logical, int ngroups) { return logical / ngroups; }        // ngroups = cout / (32 NCB)
WF16_HD int wf16_cout_group(int logical, int ngroups) { return logical % ngroups; }

// ---- U: byte offset of the stage (k-step s, frequency f) of 32-cout block cb32; nks = cin / 16 k-steps; lane l's fragment at + 16 l ----
WF16_HD size_t wf16_u_stage(int cb32, int nks, int s, int f) { return (((size_t)cb32 * nks + s) * 16 + f) * WF16_STAGE; }

// ---- the input transform's items: thread -> (tile, channel pair chp of a k-half's 8), for both k-halves of the step ----
// K1w's map: a 32-lane half of a wave is 8 consecutive tiles x 4 consecutive channel pairs, which keeps the patch reads (8 B) and the V
// writes (4 B) of a half wave on different banks.  Tile tt = board tt >> 4, tile row (tt >> 2) & 3, tile column tt & 3.
WF16_HD int wf16_item_tile(int tid) { return ((tid >> 5) & 3) * 8 + (tid & 7); }
WF16_HD int wf16_item_chp(int tid) { return ((tid >> 7) << 2) + ((tid >> 3) & 3); }

// ---- V images (offsets from the start of LDS) ----
WF16_HD int wf16_v_image(int img) { return WF16_LDS_V + img * WF16_VIMG; }
// inside an image: where item (tile, chp) of k-half kh puts frequency f's pair of f16 values (4 bytes)
WF16_HD int wf16_v_write(int f, int tile, int chp, int kh) { return f * WF16_VF + tile * WF16_VP + kh * WF16_VHALF + chp * 4; }
// inside an image: the MFMA B fragment of a lane for k-half kh -- tile lane & 31, channels 8 (lane >> 5) .. + 7 (16 bytes)
WF16_HD int wf16_v_read(int f, int lane, int kh) { return f * WF16_VF + (lane & 31) * WF16_VP + kh * WF16_VHALF + (lane >> 5) * 16; }

// ---- chunk buffers ----
WF16_HD int wf16_chunk_buffer(int buf) { return WF16_LDS_D + buf * WF16_DBUF; }
// a chunk = 128 pixel rows x 8 sixteen-byte pieces; thread tid moves piece (tid & 7) of pixel row 32 i + (tid >> 3), i = 0..3: a wave
// instruction reads eight whole 128-byte rows
WF16_HD int wf16_piece_row(int tid, int i) { return 32 * i + (tid >> 3); }
WF16_HD int wf16_pixel_offset(int row) { return (row >> 3) * WF16_RP + (row & 7) * WF16_PP; }  // row = board * 64 + y * 8 + x
WF16_HD int wf16_piece_dst(int tid, int i) { return wf16_pixel_offset(wf16_piece_row(tid, i)) + (tid & 7) * 16; }
// inside a buffer: patch pixel (i, j) of the item's tile, its channel pair of the chunk's half kh (8 bytes); a pixel off the board is
// read from the zero area at the same address mod 256 (the half's 64 bytes are added behind the redirection: the kernel keeps the
// sixteen offsets of half 0 and adds the half)
WF16_HD int wf16_patch_read(int tile, int chp, int i, int j, int kh) {
    const int board = tile >> 4, ty = (tile >> 2) & 3, tx = tile & 3;
    const int y = 2 * ty - 1 + i, x = 2 * tx - 1 + j;
    const int at = (board * 8 + y) * WF16_RP + x * WF16_PP + chp * 8;  // off the board: only its low 8 bits are used
    return (y >= 0 && y < 8 && x >= 0 && x < 8 ? at : WF16_DZERO + (at & 255)) + kh * WF16_DHALF;
}

// ---- the epilogue's exchange (offsets from the start of LDS) ----
// Z[q][c'][tile][unit]: unit u = couts 4 u .. 4 u + 3 of the cout block's 32 (16 bytes).  Wave q writes the rows of its 32 tiles (lane =
// tile lane & 31, units 2 g + (lane >> 5)); the wave that finishes tile row r reads, per lane, unit (lane & 7) of the tile its pixel
// belongs to, out of three frequency rows.
WF16_HD int wf16_z(int q, int c, int tile, int unit) { return ((q * 2 + c) * WF16_TILES + tile) * WF16_ZROW + ((unit ^ ((tile >> 1) & 7)) << 4); }
// the finishing wave r's output rows: lane = (pixel k * 8 + (lane >> 3) of its 32, unit lane & 7), k = 0..3; pixel p = board p >> 4,
// output row 2 r + ((p >> 3) & 1), column p & 7 -- eight lanes cover a row's 128 bytes
WF16_HD int wf16_out_pixel(int lane, int k) { return k * 8 + (lane >> 3); }
WF16_HD int wf16_out_row(int r, int p) { return (p >> 4) * 64 + (2 * r + ((p >> 3) & 1)) * 8 + (p & 7); }  // row inside the workgroup's 128
WF16_HD int wf16_out_tile(int r, int p) { return (p >> 4) * 16 + r * 4 + ((p & 7) >> 1); }

// ---- the transforms, in the kernel's operation order (T: float, or a vector of floats) ----
// B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1], applied down the patch's columns, then along its rows: V = B^T d B
template <class T>
WF16_HD void wf16_bt(const T d0, const T d1, const T d2, const T d3, T& o0, T& o1, T& o2, T& o3) {
    o0 = d0 - d2, o1 = d1 + d2, o2 = d2 - d1, o3 = d1 - d3;
}
// A^T = [1 1 1 0; 0 1 -1 -1]: Z = M A along a frequency row, Y = A^T Z down the rows; left to right
template <class T>
WF16_HD void wf16_at(const T m0, const T m1, const T m2, const T m3, T& y0, T& y1) {
    y0 = m0 + m1 + m2, y1 = m1 - m2 - m3;
}
// G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1]: U = G g G^T (the host's float64 transform, weight_layout.h: wino_transform)
template <class T>
WF16_HD void wf16_g(const T g0, const T g1, const T g2, T& u0, T& u1, T& u2, T& u3) {
    u0 = g0, u1 = 0.5 * g0 + 0.5 * g1 + 0.5 * g2, u2 = 0.5 * g0 - 0.5 * g1 + 0.5 * g2, u3 = g2;
}

}  // namespace cattus
