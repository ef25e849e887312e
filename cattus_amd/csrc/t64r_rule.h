// The one-launch LDS-resident form of the f16 tower with an f32 residual stream (dtype f16r_resident: tower64_stream_kernel in kernels.hip),
// as far as it can be wrong without a GPU: which output elements a consumer lane owns, which of the two LDS buffers a layer reads and
// writes, and the launch's layer table.  Plain C++: host and device, no HIP call; the kernel and the evaluator are written with these
// functions and tests/test_t64r_rule.py runs them on the CPU.
//
// The arithmetic is f16r_rule.h's, element for element (f16r_finish); only where the tensors live differs from the per-layer tower:
//
//   S  the f32 residual stream   per layer: rows in memory        here: the owning lane's registers, 16 * T64R_CB * npb values, never in LDS
//   A  its f16 operand copy      per layer: rows in memory        here: LDS buffer 0
//   M  a block's middle          per layer: rows in memory        here: LDS buffer 1 (which first holds the expanded planes)
//
// S can stay in registers because t64r_own() takes no layer argument: the lane that adds a skip element is the lane that produced it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "f16r_rule.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define T64R_HD __host__ __device__ inline
#else
#define T64R_HD inline
#endif

namespace cattus {

// ---- the workgroup: 4 consumer waves (and 4 loader waves behind them), 256 / ch tower rows of 64 channels ----
// ch = 4: one 64-slot board per workgroup, a wave holds 32 pixels x 32 couts; ch = 2: 128 rows (two 64-slot boards or one 128-slot
// board), a wave holds 64 pixels x 32 couts as two 32-pixel blocks.  An accumulator block is 32 x 32: 16 f32 per lane.
constexpr int T64R_CB = 1;                                              // 32-cout blocks per consumer wave
T64R_HD constexpr int t64r_rows(int ch) { return 256 / ch; }           // tower rows of a workgroup
T64R_HD constexpr int t64r_npb(int ch) { return ch == 4 ? 1 : 2; }     // 32-pixel blocks per consumer wave
T64R_HD constexpr int t64r_stream_regs(int ch) { return 16 * T64R_CB * t64r_npb(ch); }  // f32 stream values a lane keeps

// ---- 1. the ownership map ----
// Accumulator element e (0..15) of block (cb, pb) of lane `lane` of consumer wave `wave` is the output at (row of the workgroup, output
// channel).  No layer argument: every layer of the launch finishes the same elements in the same lanes.
struct T64rOwn {
    int row;      // 0 .. t64r_rows(ch) - 1
    int channel;  // 0 .. 63
};
T64R_HD T64rOwn t64r_own(int ch, int wave, int lane, int cb, int pb, int e) {
    const int r = lane & 31, h = lane >> 5;
    const int rb = ch == 2 ? wave >> 1 : 0;   // 64-row block of the wave
    const int pb0 = ch == 4 ? wave >> 1 : 0;  // first 32-pixel block of the wave inside its row block
    const int coutb = (wave & 1) * 32;        // first output channel of the wave
    return T64rOwn{rb * 64 + (pb0 + pb) * 32 + r, coutb + cb * 32 + (e >> 2) * 8 + h * 4 + (e & 3)};
}
// where that element lives: byte offset inside an LDS activation buffer (128-byte rows of 64 f16, the row's 16-byte slots swizzled by
// the row), and element index in the f32 rows the last layer stores ([row][64]; row0 = the workgroup's first tower row)
T64R_HD int t64r_lds_offset(T64rOwn o) { return o.row * 128 + (((o.channel >> 3) ^ ((o.row >> 1) & 7)) << 4) + (o.channel & 7) * 2; }
T64R_HD size_t t64r_out_index(size_t row0, T64rOwn o) { return (row0 + (size_t)o.row) * 64 + (size_t)o.channel; }

// ---- 2. the LDS buffer of each layer ----
// The stem reads buffer 1 (the planes) and writes 0; a block's conv1 reads 0 and writes 1, its conv2 reads 1 and writes 0: a stream
// layer's operand copy lands in buffer 0, where the next conv1 reads.
constexpr int T64R_LDS_A = 0, T64R_LDS_M = 1;
T64R_HD int t64r_reads(uint32_t l) { return (l & 1) ? T64R_LDS_A : T64R_LDS_M; }
T64R_HD int t64r_writes(uint32_t l) { return 1 - t64r_reads(l); }

// ---- 3. the launch's layer table ----
T64R_HD uint32_t t64r_layers(uint32_t blocks) { return f16r_layers(blocks); }
T64R_HD uint32_t t64r_blocks(uint32_t nlayers) { return (nlayers - 1) / 2; }
struct T64rLayer {
    int reads, writes;  // LDS buffers
    bool stream;        // finished as a stream layer (the stem, every conv2): the lane's stream registers receive y
    bool skip;          // adds the lane's stream registers (every conv2)
    bool last;          // the tower's last layer: y alone, as f32 rows to memory; no copy, nothing counted
};
T64R_HD T64rLayer t64r_layer(uint32_t l, uint32_t blocks) {
    const bool stream = f16r_stream_layer(l);
    return T64rLayer{t64r_reads(l), t64r_writes(l), stream, stream && l > 0, f16r_is_last(l, blocks)};
}

}  // namespace cattus
