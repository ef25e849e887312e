// The one-launch LDS-resident form of the exact f32 tower (dtype f32_resident: tower64_f32_kernel in kernels_t64f.hip), as far as it can be
// wrong without a GPU: the LDS plan, the step table the loader and the consumer waves both walk, which output elements a consumer lane owns and
// where an element lives in LDS, the tap rows, the layer table and the workgroup-shape choice.  Plain C++: host and device, no HIP call; the
// kernel and the evaluator are written with these functions and tests/test_t64f_rule.py runs them on the CPU.
//
// The arithmetic is conv3x3_mfma_v2_layer<float, ...>'s, operation for operation (kernels.hip): one Mfma<float>::mac chain per accumulator over
// (32-channel chunk) x (kernel row dy) x (3 taps dx x 4 k-slices), then + bias, + skip, ReLU under the pixel mask.  Only where the tensors live
// differs from the per-layer f32 tower:
//
//   X  the stream (the stem's and every conv2's output)   per layer: f32 rows in memory   here: LDS buffer 0
//   M  a block's middle (and first the expanded planes)   per layer: f32 rows in memory   here: LDS buffer 1
//
// A conv2 writes its output over its own skip rows: t64f_own() takes no layer argument, so the lane that adds a skip element is the lane that
// overwrites it, behind its own read.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define T64F_HD __host__ __device__ inline
#else
#define T64F_HD inline
#endif

namespace cattus {

// ---- the workgroup: 4 consumer waves and 4 loader waves, 256 / ch tower rows of 64 channels ----
// ch = 4: 64 rows (one 64-slot board), a consumer wave holds 32 pixels x 32 couts; ch = 2: 128 rows (two 64-slot boards or one 128-slot
// board), a wave holds 64 rows x 32 couts as two 32-pixel blocks.  An accumulator block is 32 x 32: 16 f32 per lane.
T64F_HD constexpr int t64f_rows(int ch) { return 256 / ch; }
T64F_HD constexpr int t64f_npb(int ch) { return ch == 4 ? 1 : 2; }
// 64-slot boards: one board per workgroup while the batch has at most 256 padded boards (no CU gets two workgroups' worth of rows in one);
// 128-slot boards always take 128 rows.  force = CATTUS_T64_CH (2 | 4; anything else: by grid size).
T64F_HD constexpr int t64f_ch(uint32_t boards, uint32_t slots, int force) {
    return slots != 64 ? 2 : force == 2 || force == 4 ? force : boards <= 256 ? 4 : 2;
}

// ---- 1. the LDS plan ----
// The weight ring first (ring slot and tap fold into ds_read immediates): 3 slabs of [3 taps][64 cout][128 B], the per-layer kernel's slab.
// Behind it two activation buffers of [2 chunks][rows][128 B] f32 (chunk c = channels 32c .. 32c + 31), each followed by a 256-byte zero
// area that off-board taps read at their row's own address mod 256 (device_common.h, ZAREA_SP).
constexpr int T64F_TAP_BYTES = 64 * 128;
constexpr int T64F_SLAB = 3 * T64F_TAP_BYTES;
constexpr int T64F_RING = 3;       // slabs in the ring
constexpr int T64F_AHEAD = 2;      // steps the loaders run ahead of the consumers
constexpr int T64F_ZAREA = 256;
constexpr int T64F_LDS_MAX = 163840;  // a CU's LDS
struct T64fLds {
    int ring;          // the ring's first byte
    int buf[2];        // the buffers' first bytes
    int chunk_stride;  // from chunk 0 to chunk 1 inside a buffer
    int zero_off;      // a buffer's zero area, from the buffer's first byte
    int total;
};
T64F_HD constexpr T64fLds t64f_lds(int ch) {
    const int cs = t64f_rows(ch) * 128, bytes = 2 * cs + T64F_ZAREA, b0 = T64F_RING * T64F_SLAB;
    return T64fLds{0, {b0, b0 + bytes}, cs, 2 * cs, b0 + 2 * bytes};
}

// ---- 2. the step table ----
// A step is one slab: (layer, chunk, dy).  The stem's input is one chunk (Cin_pad = 32): 3 steps; a hidden layer walks `nch` chunks: 6 steps,
// or 3 on a network of at most 32 filters (the narrow walk: chunk 1 of its weights and activations is all zero, fmaf(0, 0, acc) = acc and an
// accumulator that starts at +0 never becomes -0, so leaving those steps out changes no bit).  The step counter runs across the layers.
T64F_HD constexpr int t64f_hidden_chunks(uint32_t filters, bool narrow_on) { return narrow_on && filters <= 32 ? 1 : 2; }
T64F_HD constexpr int t64f_layer_chunks(int layer, int nch) { return layer == 0 ? 1 : nch; }
T64F_HD constexpr int t64f_row_bytes(int layer) { return layer == 0 ? 128 : 256; }  // a weight row: Cin_pad f32 (the stem's: 32, else 64)
T64F_HD constexpr int t64f_layer_weight_bytes(int layer) { return 9 * 64 * t64f_row_bytes(layer); }
T64F_HD constexpr int t64f_steps(int nlayers, int nch) { return 3 + (nlayers - 1) * 3 * nch; }
struct T64fStep {
    int layer, chunk, dy;
};
T64F_HD constexpr T64fStep t64f_step(int s, int nch) {
    if (s < 3) return T64fStep{0, 0, s};
    const int u = s - 3, per = 3 * nch, v = u % per;
    return T64fStep{1 + u / per, v / 3, v % 3};
}
T64F_HD constexpr int t64f_ring_slot(int s) { return s % T64F_RING; }
// byte offset, into the layer's [9][64][Cin_pad] f32 weight rows, of the step's slab: tap row dy (taps 3 dy .. 3 dy + 2), chunk's 128 bytes
T64F_HD constexpr int t64f_slab_src(T64fStep st) { return st.dy * 3 * 64 * t64f_row_bytes(st.layer) + st.chunk * 128; }
// A slab travels as 24 pieces of 1 KiB (8 cout rows x 128 B), one LDS-DMA instruction each: lane `lane` of piece `pid` fetches 16 bytes.
// The destination is lane-linear (pid * 1024 + lane * 16 inside the slab); the swizzle -- 16-byte slot c of row `row` lives in slot
// c ^ ((row >> 1) & 7) -- is applied on the source side.
constexpr int T64F_PIECES = 24;
T64F_HD constexpr int t64f_piece_src(int pid, int lane, int row_bytes) {  // from the slab's source offset
    const int tap = pid >> 3, row = (pid & 7) * 8 + (lane >> 3), c = (lane & 7) ^ ((row >> 1) & 7);
    return (tap * 64 + row) * row_bytes + c * 16;
}
T64F_HD constexpr int t64f_piece_dst(int pid) { return pid * 1024; }

// ---- 3. the ownership map ----
// Accumulator element e (0..15) of pixel block pb of lane `lane` of consumer wave `wave` is the output at (row of the workgroup, output
// channel).  No layer argument: every layer of the launch finishes the same elements in the same lanes.
struct T64fOwn {
    int row;      // 0 .. t64f_rows(ch) - 1
    int channel;  // 0 .. 63
};
T64F_HD constexpr T64fOwn t64f_own(int ch, int wave, int lane, int pb, int e) {
    const int r = lane & 31, h = lane >> 5;
    const int rb = ch == 2 ? wave >> 1 : 0;   // 64-row block of the wave
    const int pb0 = ch == 4 ? wave >> 1 : 0;  // first 32-pixel block of the wave inside its row block
    const int coutb = (wave & 1) * 32;        // first output channel of the wave
    return T64fOwn{rb * 64 + (pb0 + pb) * 32 + r, coutb + (e >> 2) * 8 + h * 4 + (e & 3)};
}

// ---- 4. where an element lives ----
// byte offset of (row, channel) inside an activation buffer: the channel's chunk, the row's 128 bytes, the 16-byte slot swizzled by the row.
// The epilogue stores four consecutive channels (elements 4g .. 4g + 3) as one 16-byte slot at the offset of the first.
T64F_HD constexpr int t64f_lds_offset(int ch, int row, int channel) {
    return (channel >> 5) * t64f_lds(ch).chunk_stride + row * 128 + ((((channel & 31) >> 2) ^ ((row >> 1) & 7)) << 4) + (channel & 3) * 4;
}
// what a fragment read of Mfma<float> takes: lane half h, k-slice ks of chunk `chunk` -- 16 bytes = k 8 ks + 4 h + j of the chunk in element j
T64F_HD constexpr int t64f_frag_offset(int ch, int chunk, int row, int ks, int h) {
    return chunk * t64f_lds(ch).chunk_stride + row * 128 + (((ks * 2 + h) ^ ((row >> 1) & 7)) << 4);
}
T64F_HD constexpr int t64f_frag_channel(int chunk, int ks, int h, int j) { return chunk * 32 + ks * 8 + h * 4 + j; }
// the same for a weight fragment inside a slab: tap dx, cout row
T64F_HD constexpr int t64f_wfrag_offset(int dx, int cout, int ks, int h) { return dx * T64F_TAP_BYTES + cout * 128 + (((ks * 2 + h) ^ ((cout >> 1) & 7)) << 4); }
// element index in the f32 rows [row][64] the last layer stores (row0: the workgroup's first tower row)
T64F_HD constexpr size_t t64f_out_index(size_t row0, T64fOwn o) { return (row0 + (size_t)o.row) * 64 + (size_t)o.channel; }

// ---- 5. the tap rows ----
// Tap (dy, dx) of pixel slot p of a board of edge S whose rows start at workgroup row board_row: the byte offset, inside CHUNK 0 of a buffer,
// of the row it reads (chunk 1: + chunk_stride, on-board taps only) and the swizzle term of lane half 0; off the board, or for a pixel slot
// the board does not have, the buffer's zero area at the row's own address mod 256.
struct T64fTap {
    int rel;   // byte offset from the buffer's first byte
    int swz;   // (row >> 1) & 7 of the row the tap names (its low bits also where it is off the board)
    bool ok;   // on the board
};
T64F_HD constexpr T64fTap t64f_tap(int ch, int S, int board_row, int p, int dy, int dx) {
    const int ph = p / S, pw = p - ph * S, hh = ph + dy - 1, ww = pw + dx - 1;
    const bool ok = p < S * S && hh >= 0 && hh < S && ww >= 0 && ww < S;
    const int q = hh * S + ww;  // may be negative off the board: only its low bits are used then
    return T64fTap{ok ? (board_row + q) * 128 : t64f_lds(ch).zero_off + (q & 1) * 128, (q >> 1) & 7, ok};
}

// ---- 6. the layer table ----
// The stem reads buffer 1 (the planes) and writes 0; a block's conv1 reads 0 and writes 1; its conv2 reads 1, adds the skip from 0 and writes 0.
constexpr int T64F_LDS_X = 0, T64F_LDS_M = 1;
T64F_HD constexpr uint32_t t64f_layers(uint32_t blocks) { return 1 + 2 * blocks; }
T64F_HD constexpr uint32_t t64f_blocks(uint32_t nlayers) { return (nlayers - 1) / 2; }
struct T64fLayer {
    int reads, writes;  // LDS buffers
    bool skip;          // adds the block input, read from the buffer it writes (every conv2)
    bool last;          // the tower's last layer: f32 rows to memory instead of LDS
};
T64F_HD constexpr T64fLayer t64f_layer(uint32_t l, uint32_t blocks) {
    const int reads = (l & 1) ? T64F_LDS_X : T64F_LDS_M;
    return T64fLayer{reads, 1 - reads, l > 0 && !(l & 1), l == 2 * blocks};
}

}  // namespace cattus
