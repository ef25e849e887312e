// Where an activation lives in the buffers an evaluator keeps between its layers, and how cattus_hip_trace folds a leaf's differences
// into one record (include/cattus_hip.h: cattus_hip_tap, cattus_hip_trace).  Pure functions for the host and the device alike -- no HIP
// call, nothing of the evaluator -- so that every layout and every edge of the record can be checked without a GPU
// (tests/test_tap_layout.py, tests/tap_layout_check.cpp); the kernels (kernels.hip: tap_rows_kernel, tap_gather_kernel,
// trace_compare_kernel) include this file and say the same thing.
//
// A tensor of a point has C live channels and hw = S * S live pixels per leaf.  The layouts:
//   rows, f32        element (leaf, c, p) is the float at byte ((leaf * slots + p) * pitch + c) * 4: NHWC rows of `pitch` channels
//                    (filters rounded up to 64), `slots` pixel slots per board (64 for S <= 8, else 128)
//   rows, bf16 / f16 the same rows of 2-byte elements: byte ((leaf * slots + p) * pitch + c) * 2
//   rows, f16x2      4 bytes per channel, interleaved per 32 channels: a row's group g = c / 32 is 128 bytes, [hi of its 32 channels |
//                    lo of the same 32]: hi at byte (leaf * slots + p) * pitch * 4 + g * 128 + (c % 32) * 2, lo 64 bytes behind it
//   rows, Winograd   the f32 rows above on 64-slot boards (the tower caps them at WINO_ACT_MAX; an address is an address)
//   NCHW             the generic tower: byte ((leaf * C + c) * hw + p) * 4 -- its head activations too (C = vhc + phc)
//   hv               the tuned heads' activations in MFMA fragment order, f32 or bf16: the value channels (c < vhc) are the matrix
//                    [leaf][kvp] at element 0, column k = c * hw + p; the policy channels the matrix [leaf][kpp] at element hv_pol,
//                    column k = (c - vhc) * hw + p; element (row, k) of a [rows][K] matrix sits at
//                    ((((row / 32) * (K / KSTEP) + k / KSTEP) * 2 + (k % KSTEP) / HALF) * 32 + row % 32) * HALF + k % HALF
//                    with KSTEP = 32 bytes of k (8 f32, 16 bf16) and HALF = KSTEP / 2 (device_common.h, frag_packed_index)
// A stored element is decoded exactly -- hi + lo in f32, the widening of a bf16 or an f16 -- and multiplied by 2^-t where the tensor
// carries that channel at 2^t (the f16 towers' residual stream: stream_shifts): a tapped value is a bit pattern, not an approximation.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifndef CATTUS_HD
#ifdef __HIPCC__
#define CATTUS_HD __host__ __device__
#else
#define CATTUS_HD
#endif
#endif

namespace cattus {

enum TapLayout : uint32_t {
    TAP_ROWS_F32 = 0,
    TAP_ROWS_BF16 = 1,
    TAP_ROWS_F16 = 2,
    TAP_ROWS_F16X2 = 3,
    TAP_ROWS_WINO_F32 = 4,
    TAP_NCHW_F32 = 5,
    TAP_HV_F32 = 6,
    TAP_HV_BF16 = 7,
};

// One tensor of one point as an evaluator holds it.  Rows layouts use slots and pitch; the hv layouts vhc, kvp, kpp and hv_pol.
struct TapSource {
    uint32_t layout;  // TapLayout
    uint32_t C, hw;   // live channels, live pixels per leaf
    uint32_t slots, pitch;
    uint32_t vhc, kvp, kpp, hv_pol;
};

CATTUS_HD inline bool tap_is_rows(uint32_t layout) { return layout <= TAP_ROWS_WINO_F32; }
CATTUS_HD inline bool tap_two_bytes(uint32_t layout) { return layout == TAP_ROWS_BF16 || layout == TAP_ROWS_F16 || layout == TAP_HV_BF16; }
CATTUS_HD inline bool tap_has_lo(uint32_t layout) { return layout == TAP_ROWS_F16X2; }
constexpr uint32_t TAP_LO_BYTES = 64;  // f16x2: the lo half of a channel sits this far behind its hi half

// element index of (row, k) of a [rows][K] matrix in MFMA fragment order, elements of `esz` bytes (device_common.h, frag_packed_index)
CATTUS_HD inline size_t tap_frag_index(uint32_t row, uint32_t k, uint32_t K, uint32_t esz) {
    const uint32_t kstep = 32 / esz, half = kstep / 2;
    return ((((size_t)(row >> 5) * (K / kstep) + k / kstep) * 2 + (k % kstep) / half) * 32 + (row & 31)) * half + k % half;
}

// Byte offset of the stored element (leaf, c, p), c < C, p < hw; of its hi half for f16x2 (the lo half: + TAP_LO_BYTES).
CATTUS_HD inline size_t tap_offset(const TapSource& s, uint32_t leaf, uint32_t c, uint32_t p) {
    const size_t row = (size_t)leaf * s.slots + p;
    switch (s.layout) {
        case TAP_ROWS_F32:
        case TAP_ROWS_WINO_F32: return (row * s.pitch + c) * 4;
        case TAP_ROWS_BF16:
        case TAP_ROWS_F16: return (row * s.pitch + c) * 2;
        case TAP_ROWS_F16X2: return row * s.pitch * 4 + (size_t)(c >> 5) * 128 + (c & 31) * 2;
        case TAP_NCHW_F32: return (((size_t)leaf * s.C + c) * s.hw + p) * 4;
        default: break;
    }
    const uint32_t esz = s.layout == TAP_HV_BF16 ? 2 : 4;
    const size_t at = c < s.vhc ? tap_frag_index(leaf, c * s.hw + p, s.kvp, esz) : s.hv_pol + tap_frag_index(leaf, (c - s.vhc) * s.hw + p, s.kpp, esz);
    return at * esz;
}

CATTUS_HD inline float tap_from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
CATTUS_HD inline uint32_t tap_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// the exact widenings
CATTUS_HD inline float tap_widen_bf16(uint16_t h) { return tap_from_bits((uint32_t)h << 16); }
CATTUS_HD inline float tap_widen_f16(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, ex = (h >> 10) & 31u, man = h & 0x3ffu;
    if (ex == 31) return tap_from_bits(sign | 0x7f800000u | (man << 13));  // infinities and NaNs
    if (ex != 0) return tap_from_bits(sign | ((ex + 112) << 23) | (man << 13));
    const float sub = (float)man * 5.9604644775390625e-08f;  // subnormals (and zero): man * 2^-24, exact
    return sign ? -sub : sub;
}

// 2^e as a float, -126 <= e <= 127: the exact inverse of a stream shift is tap_pow2(-t)
CATTUS_HD inline float tap_pow2(int e) { return tap_from_bits((uint32_t)(e + 127) << 23); }

// The value of element (leaf, c, p) in network units; shifts: NULL, or the exponent t_c each channel of this tensor is carried at.
CATTUS_HD inline float tap_decode(const TapSource& s, const void* base, const int* shifts, uint32_t leaf, uint32_t c, uint32_t p) {
    const char* at = static_cast<const char*>(base) + tap_offset(s, leaf, c, p);
    float v;
    if (tap_has_lo(s.layout)) {
        uint16_t hi, lo;
        memcpy(&hi, at, 2);
        memcpy(&lo, at + TAP_LO_BYTES, 2);
        v = tap_widen_f16(hi) + tap_widen_f16(lo);
    } else if (tap_two_bytes(s.layout)) {
        uint16_t h;
        memcpy(&h, at, 2);
        v = s.layout == TAP_ROWS_F16 ? tap_widen_f16(h) : tap_widen_bf16(h);
    } else {
        memcpy(&v, at, 4);
    }
    return shifts ? v * tap_pow2(-shifts[c]) : v;
}

// ---- cattus_hip_trace: one leaf of one point, the evaluator's values x against the shadow's ref ----
// The 32 bytes of a record (include/cattus_hip.h, cattus_trace_record).  Over the leaf's live elements, index i = c * hw + p:
//   max_diff   the largest float32(|double(x) - double(ref)|) (verify_rule.h's dlogit), `at` the lowest index that holds it; a NaN
//              difference takes no part; 0 at index 0 where no difference is positive.  x, ref: the two values at `at`.
//   rms_diff   float32(sqrt(sum (x - ref)^2 / count)), rms_ref float32(sqrt(sum ref^2 / count)), differences, squares and sums in
//              double over ALL live elements (a non-finite value makes them infinite or NaN; a NaN is the one quiet NaN 0x7fc00000)
//   flags      bit 0: some live x or ref is not finite
struct TraceRecord {
    float max_diff;
    uint32_t at;
    float x, ref;
    float rms_diff, rms_ref;
    uint32_t flags, reserved;
};
static_assert(sizeof(TraceRecord) == 32, "a record is two 16-byte stores");
constexpr uint32_t TRACE_NONFINITE = 1;

// What a thread (or the host loop) has seen so far.  The maximum combines in any order -- larger difference first, then lower index
// -- and the flag is an OR; the double sums are added in whatever fixed order the caller combines in.
struct TracePartial {
    double sum_d2, sum_r2;
    float best_d;
    uint32_t best_i, nonfinite;
};

CATTUS_HD inline TracePartial trace_partial() { return TracePartial{0.0, 0.0, 0.0f, 0xffffffffu, 0u}; }
CATTUS_HD inline bool trace_finite(float x) { return fabs((double)x) <= 3.4028234663852886e+38; }  // false for NaN
CATTUS_HD inline void trace_take_max(float d, uint32_t i, float& best_d, uint32_t& best_i) {
    if (d > best_d || (d == best_d && i < best_i)) best_d = d, best_i = i;
}
CATTUS_HD inline void trace_take(TracePartial& t, float x, float ref, uint32_t i) {
    const double d = (double)x - (double)ref, r = (double)ref;
    t.sum_d2 += d * d;
    t.sum_r2 += r * r;
    trace_take_max((float)fabs(d), i, t.best_d, t.best_i);
    if (!trace_finite(x) || !trace_finite(ref)) t.nonfinite = 1;
}
// a += b: `a` the partial that comes first in the caller's order
CATTUS_HD inline void trace_combine(TracePartial& a, const TracePartial& b) {
    a.sum_d2 += b.sum_d2;
    a.sum_r2 += b.sum_r2;
    trace_take_max(b.best_d, b.best_i, a.best_d, a.best_i);
    a.nonfinite |= b.nonfinite;
}
CATTUS_HD inline float trace_rms(double sum, uint32_t count) {
    const float r = (float)sqrt(sum / (double)count);
    return r != r ? tap_from_bits(0x7fc00000u) : r;
}
// Everything of the record but x and ref, which the caller reads at r.at.
CATTUS_HD inline TraceRecord trace_finish(const TracePartial& t, uint32_t count) {
    TraceRecord r;
    r.max_diff = t.best_d;
    r.at = t.best_d > 0.0f ? t.best_i : 0u;
    r.x = r.ref = 0.0f;
    r.rms_diff = trace_rms(t.sum_d2, count);
    r.rms_ref = trace_rms(t.sum_r2, count);
    r.flags = t.nonfinite ? TRACE_NONFINITE : 0u;
    r.reserved = 0;
    return r;
}

// The whole rule on one leaf in index order (count >= 1): what the kernel's workgroup computes in pieces.
inline TraceRecord trace_leaf(const float* x, const float* ref, uint32_t count) {
    TracePartial t = trace_partial();
    for (uint32_t i = 0; i < count; i++) trace_take(t, x[i], ref[i], i);
    TraceRecord r = trace_finish(t, count);
    r.x = x[r.at], r.ref = ref[r.at];
    return r;
}

}  // namespace cattus
