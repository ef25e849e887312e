// The small-tile Winograd F(2x2, 3x3) layer kernel (kernels_wino4s.hip, K1w4s), as far as it can be wrong without a GPU: which tile a
// workgroup takes, which item of the input transform a thread takes, and where everything lives in LDS.  Plain C++: host and device,
// no HIP call; the kernel is written with these functions and tests/test_wino4s_rule.py runs them on the CPU.
//
//   workgroup = 4 waves = 2 boards (32 tiles of 2x2 outputs, 128 pixel rows) x 32 couts; wave q owns frequency row q (f = 4 q + l)
//   LDS:  [ V image 0 | V image 1 | chunk buffer 0 | chunk buffer 1 ]; the epilogue's exchange lies over V image 0
//     V image (one k-step of 16 channels): [f 16][tile 32][16 ch hi | 16 ch lo | 16 B pad] -- K1w's image
//     chunk buffer (32 channels of the 128 pixel rows, f32): K1w's image -- pixel pitch 144 B, board rows of 8 pixels + 64 B, a zero
//       area behind the 16 board rows that patch pixels off the board are read from, at the read's own address mod 256 (the same banks)
//     exchange: [frequency row q][c' 2][tile 32][8 units of 4 couts, f32], the unit XORed with bits 1..3 of the tile
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define W4S_HD __host__ __device__ inline
#else
#define W4S_HD inline
#endif

namespace cattus {

constexpr int W4S_BOARDS = 2, W4S_TILES = 32, W4S_COUTS = 32, W4S_ROWS = 128;  // a workgroup's tile
constexpr int W4S_THREADS = 256;

constexpr int W4S_VP = 80;                   // a tile's row of a V image: 16 ch hi (32 B) | 16 ch lo (32 B) | 16 B pad
constexpr int W4S_VF = W4S_TILES * W4S_VP;   // one frequency
constexpr int W4S_VIMG = 16 * W4S_VF;        // one k-step's V: 40,960 B
constexpr int W4S_PP = 144;                  // pixel pitch of a chunk image: 128 B of data + 16
constexpr int W4S_RP = 8 * W4S_PP + 64;      // pitch of a board row
constexpr int W4S_DZERO = 16 * W4S_RP;       // behind the 16 board rows: the zero area
constexpr int W4S_ZAREA = 512;               // a redirected read keeps its address's low 8 bits: 255 + a half's 64 + 8 bytes, to 256
constexpr int W4S_DBUF = W4S_DZERO + W4S_ZAREA;  // 19,968 B
constexpr int W4S_LDS_V = 0;                     // the two V images
constexpr int W4S_LDS_D = 2 * W4S_VIMG;          // the two chunk buffers
constexpr int W4S_LDS_LOOP = W4S_LDS_D + 2 * W4S_DBUF;
constexpr int W4S_ZROW = 128;                          // a tile's row of the exchange: 32 couts f32
constexpr int W4S_LDS_Z = 4 * 2 * W4S_TILES * W4S_ZROW;  // the exchange: 32,768 B, over V image 0
constexpr int W4S_LDS_TOTAL = W4S_LDS_LOOP;              // 121,856 B
static_assert(W4S_DZERO % 256 == 0 && W4S_DBUF % 256 == 0 && W4S_LDS_D % 256 == 0, "the zero area keeps a read's banks only if it is 256-B aligned");
static_assert(W4S_ZAREA >= 255 + 64 + 8,"a read redirected into the zero area stays inside it");
static_assert(W4S_LDS_Z <= W4S_VIMG && W4S_LDS_TOTAL <= 160 * 1024, "LDS sizes");

// ---- the grid ----
// (board pair, cout block) with the cout block fastest, behind the XCD map of the tiled kernels (device_common.h: xcd_remap): workgroup
// ids go round the 8 XCDs, so on a grid that is a multiple of 8 every XCD gets one contiguous range of logical indices and the cout
// blocks of a board pair, which read the same rows, share an L2.
W4S_HD uint32_t wino4s_grid(uint32_t bpad, uint32_t cout) { return (bpad / W4S_BOARDS) * (cout / W4S_COUTS); }
W4S_HD int wino4s_logical(int wg, int nblk) { return (nblk & 7) == 0 ? (wg & 7) * (nblk >> 3) + (wg >> 3) : wg; }
W4S_HD int wino4s_pair(int logical, int ncb) { return logical / ncb; }        // ncb = cout / 32
W4S_HD int wino4s_cout_block(int logical, int ncb) { return logical % ncb; }

// ---- the input transform's item: thread -> (tile, channel pair of the k-step's 8) ----
// K1w's map: a 32-lane half of a wave is 8 consecutive tiles x 4 consecutive channel pairs, which keeps the patch reads (8 B) and the V
// writes (4 B) of a half wave on different banks.  Tile tt = board tt >> 4, tile row (tt >> 2) & 3, tile column tt & 3.
W4S_HD int wino4s_item_tile(int tid) { return ((tid >> 5) & 3) * 8 + (tid & 7); }
W4S_HD int wino4s_item_chp(int tid) { return ((tid >> 7) << 2) + ((tid >> 3) & 3); }

// ---- V images (offsets from the start of LDS) ----
W4S_HD int wino4s_v_image(int img) { return W4S_LDS_V + img * W4S_VIMG; }
// inside an image: where item (tile, chp) puts frequency f's pair of f16 values, part 0 = hi, 1 = lo (4 bytes)
W4S_HD int wino4s_v_write(int f, int tile, int chp, int part) { return f * W4S_VF + tile * W4S_VP + part * 32 + chp * 4; }
// inside an image: the MFMA B fragment of a lane -- tile lane & 31, channels 8 (lane >> 5) .. + 7 (16 bytes)
W4S_HD int wino4s_v_read(int f, int lane, int part) { return f * W4S_VF + (lane & 31) * W4S_VP + part * 32 + (lane >> 5) * 16; }

// ---- chunk buffers ----
W4S_HD int wino4s_chunk_buffer(int buf) { return W4S_LDS_D + buf * W4S_DBUF; }
// a chunk = 128 pixel rows x 8 sixteen-byte pieces; thread tid moves piece (tid & 7) of pixel row 32 i + (tid >> 3), i = 0..3: a wave
// instruction reads eight whole 128-byte rows
W4S_HD int wino4s_piece_row(int tid, int i) { return 32 * i + (tid >> 3); }
W4S_HD int wino4s_pixel_offset(int row) { return (row >> 3) * W4S_RP + (row & 7) * W4S_PP; }  // row = board * 64 + y * 8 + x
W4S_HD int wino4s_piece_dst(int tid, int i) { return wino4s_pixel_offset(wino4s_piece_row(tid, i)) + (tid & 7) * 16; }
// inside a buffer: patch pixel (i, j) of the item's tile, its channel pair of the chunk's half kp (8 bytes); a pixel off the board is
// read from the zero area at the same address mod 256 (the half's 64 bytes are added behind the redirection: the kernel keeps the
// sixteen offsets of half 0 and adds the half)
W4S_HD int wino4s_patch_read(int tile, int chp, int i, int j, int kp) {
    const int board = tile >> 4, ty = (tile >> 2) & 3, tx = tile & 3;
    const int y = 2 * ty - 1 + i, x = 2 * tx - 1 + j;
    const int at = (board * 8 + y) * W4S_RP + x * W4S_PP + chp * 8;  // off the board: only its low 8 bits are used
    return (y >= 0 && y < 8 && x >= 0 && x < 8 ? at : W4S_DZERO + (at & 255)) + kp * 64;
}

// ---- the epilogue's exchange (offsets from the start of LDS) ----
// Z[q][c'][tile][unit]: unit u = couts 4 u .. 4 u + 3 of the workgroup's 32 (16 bytes).  Wave q writes the rows of its 32 tiles (lane =
// tile lane & 31, units 2 g + (lane >> 5)); the wave that finishes tile row r reads, per lane, unit (lane & 7) of the tile its pixel
// belongs to, out of three frequency rows.
W4S_HD int wino4s_z(int q, int c, int tile, int unit) { return ((q * 2 + c) * W4S_TILES + tile) * W4S_ZROW + ((unit ^ ((tile >> 1) & 7)) << 4); }
// the finishing wave r's output rows: lane = (pixel k * 8 + (lane >> 3) of its 32, unit lane & 7), k = 0..3; pixel p = board p >> 4,
// output row 2 r + ((p >> 3) & 1), column p & 7 -- eight lanes cover a row's 128 bytes
W4S_HD int wino4s_out_pixel(int lane, int k) { return k * 8 + (lane >> 3); }
W4S_HD int wino4s_out_row(int r, int p) { return (p >> 4) * 64 + (2 * r + ((p >> 3) & 1)) * 8 + (p & 7); }  // row inside the workgroup's 128
W4S_HD int wino4s_out_tile(int r, int p) { return (p >> 4) * 16 + r * 4 + ((p & 7) >> 1); }

}  // namespace cattus
