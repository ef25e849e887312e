// The direct single-term f16 tower with an f32 residual stream (dtype f16r, K1hr: conv3x3_f16r_kernel in kernels.hip), as far as it can be
// wrong without a GPU: the epilogue of one output element in the kernel's operation order, which of a lane's three activation buffers
// holds which tensor and what every layer reads, adds and writes, and where a point's activations live for cattus_hip_tap / _trace.
// Plain C++: host and device, no HIP call; the kernel and the evaluator are written with these functions and tests/test_f16r_rule.py runs
// them on the CPU.
//
//   S  the residual stream: plain f32 rows [board][slot][filters padded to 64], y itself, never rounded to f16 and never clamped
//   A  its operand copy: f16 rows of f16(min(y, 65504)), what the next conv1 multiplies; values beyond 65504 are counted in `saturated`
//   M  a block's middle activation: f16 rows, written by conv1 exactly as dtype f16 writes it
//
//   stem             planes -> y = relu(fmaf(acc, 2^-s, bias))       under the pixel mask;  S = y, A = f16(min(y, 65504))
//   conv1 of block i A -> M                                           dtype f16's layer: no skip, clamp, count
//   conv2 of block i M -> y = relu(fmaf(acc, 2^-s, bias) + S)         in f32;  S = y in place, A = f16(min(y, 65504))
//   the last layer   writes S alone (the f32 head kernels read it): no copy, nothing counted
// Weights, scales, biases and stream shifts are dtype f16's.  With no block the tower is dtype f16's stem, bit for bit; with blocks,
// point 1 (block 0 behind conv1) is dtype f16's, bit for bit, and point 0 rounds to dtype f16's point 0.
#pragma once
#include <stdint.h>

#include "tap_layout.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define F16R_HD __host__ __device__ inline
#else
#define F16R_HD inline
#endif

namespace cattus {

constexpr float F16R_COPY_MAX = 65504.0f;  // the largest f16: the operand copy saturates there instead of becoming an infinity

// ---- one output element, in the kernel's operation order ----
struct F16rOut {
    float stream;   // what S receives
    _Float16 copy;  // what A receives (not written by the tower's last layer)
    bool counted;   // the copy was clamped: one more in `saturated` (not counted by the tower's last layer)
};
// acc: the f32 MFMA sum, carrying the weights' power-of-two scale 2^s; inv_scale = 2^-s, so the product is exact and the fused
// multiply-add rounds once, as dtype f16's does; skip: the element's f32 stream value (read only where has_skip); valid: the pixel slot
// is on the board -- slots past it stay zero.  A NaN sum fails `> 0` and leaves as 0, as in every tower here.
F16R_HD F16rOut f16r_finish(float acc, float inv_scale, float bias, float skip, bool has_skip, bool valid) {
    float v = __builtin_fmaf(acc, inv_scale, bias);
    if (has_skip) v = v + skip;
    const float y = valid && v > 0.0f ? v : 0.0f;
    return F16rOut{y, (_Float16)(y < F16R_COPY_MAX ? y : F16R_COPY_MAX), y > F16R_COPY_MAX};
}

// ---- the lane's buffers ----
// Every lane has three activation buffers of bpad * slots * fpad * 4 bytes (evaluator.hip: Lane::a, ::t, ::y; they already hold f32 rows
// for the f16 towers' last layer) and the packed planes x0.  The roles never move: no swap, nothing new to allocate.
enum F16rBuf : int { F16R_NONE = -1, F16R_BUF_A = 0, F16R_BUF_T = 1, F16R_BUF_Y = 2, F16R_BUF_X0 = 3 };
constexpr int F16R_S = F16R_BUF_A;  // the stream, f32 rows
constexpr int F16R_M = F16R_BUF_T;  // the middle activation, f16 rows
constexpr int F16R_A = F16R_BUF_Y;  // the operand copy, f16 rows

F16R_HD uint32_t f16r_layers(uint32_t blocks) { return 1 + 2 * blocks; }  // launches of a pass: the stem, two per block
F16R_HD bool f16r_is_last(uint32_t l, uint32_t blocks) { return l == 2 * blocks; }
// layer l -- 0: the stem, 2i + 1: block i's conv1, 2i + 2: its conv2 -- runs on the stream kernel unless it is a conv1
F16R_HD bool f16r_stream_layer(uint32_t l) { return (l & 1) == 0; }

struct F16rLayer {
    int reads;         // the conv's input rows (X0: the planes, fused into the stem or packed)
    int adds;          // the skip rows, or F16R_NONE
    int writes;        // f32 stream rows (stream layers) or f16 rows (conv1)
    int writes_copy;   // the f16 operand copy of a stream layer, or F16R_NONE (conv1; the last layer)
};
F16R_HD F16rLayer f16r_layer(uint32_t l, uint32_t blocks) {
    const int copy = f16r_is_last(l, blocks) ? F16R_NONE : F16R_A;
    if (l == 0) return F16rLayer{F16R_BUF_X0, F16R_NONE, F16R_S, copy};
    if (l & 1) return F16rLayer{F16R_A, F16R_NONE, F16R_M, F16R_NONE};
    return F16rLayer{F16R_M, F16R_S, F16R_S, copy};
}
// the buffer the f32 head kernels read behind the last layer
F16R_HD int f16r_head_input() { return F16R_S; }

// ---- observation: where point `l` < 1 + 2 blocks lives and how it is decoded ----
// The buffer layer l wrote that a tap reads: the stream S behind a stream layer, M behind a conv1.
F16R_HD int f16r_tap_buffer(uint32_t l) { return f16r_stream_layer(l) ? F16R_S : F16R_M; }
F16R_HD TapSource f16r_tap_source(uint32_t l, uint32_t filters, uint32_t hw, uint32_t slots, uint32_t fpad) {
    TapSource s{};
    s.layout = f16r_stream_layer(l) ? TAP_ROWS_F32 : TAP_ROWS_F16;
    s.C = filters, s.hw = hw, s.slots = slots, s.pitch = fpad;
    return s;
}
// the stream points carry channel k at 2^t_k (stream_shifts) and a tap multiplies by 2^-t_k; the middle points are at 2^0
F16R_HD bool f16r_tap_shifted(uint32_t l) { return f16r_stream_layer(l); }

}  // namespace cattus
