// The device layouts of one folded 3x3 conv layer, as host vectors: pure functions of the layer and its padded shape -- no HIP call,
// nothing of the evaluator -- so that every index can be checked without a GPU (tests/test_weight_layout.py).  Output channels are
// padded to cout_pad and input channels to the device layout of the producing layer (cin_pad, a multiple of one 128-byte row) with
// zero weights and zero bias: a padded channel computes relu(0) = 0, and as an input it adds fmaf(0, x, acc) = acc terms only, so the
// f32 chains of the real channels are bit for bit unchanged.  Compiled with -ffp-contract=off like all host code here.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "frag_index.h"
#include "winof4_rule.h"

namespace cattus {

struct Folded {
    std::vector<float> w;  // [taps][cout][cin]
    std::vector<float> b;  // [cout]
};
struct ConvShape { uint32_t cout, cin, cout_pad, cin_pad; };  // of the Folded layer; as laid out on the device

// Input channels of the stem as laid out on the device (cpad0): the planes in whole 128-byte rows of the tower's activation layout,
// row_channels to a row (kernels.h, act_kc: 32 for f32 and f16x2, 64 for bf16 and f16).  The f16x2 stem that expands the planes itself
// (STEM, at most 32 planes) runs that one chunk; on packed input it is an ordinary layer of conv3x3_splitw / conv3x3_split, whose loaders
// request two chunks up front, so its channels are then padded to whole pairs of chunks (64) -- chunk counts the hidden layers run too.
inline bool stem_is_fused(uint32_t planes, bool pack_separately) { return planes <= 32 && !pack_separately; }
inline uint32_t stem_cin_pad(uint32_t planes, uint32_t row_channels, bool f16x2, bool pack_separately) {
    const uint32_t to = f16x2 && !stem_is_fused(planes, pack_separately) ? 64 : row_channels;
    return (planes + to - 1) / to * to;
}

inline uint16_t f32_to_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // keep NaN a NaN
    u += 0x7fffu + ((u >> 16) & 1u);                                           // round to nearest even
    return (uint16_t)(u >> 16);
}

// The f16 towers' power-of-two scale 2^s of one output channel: its largest |w 2^s| lies in [2^10, 2^11), so the lo halves of all but
// the channel's tiniest weights are normal f16 numbers (22 significant bits per weight; single-term f16: no weight becomes a
// subnormal unless it is 2^-24 of the largest) and nothing comes near the f16 range limit.  2^-s -- applied to the f32 accumulator
// in the epilogue -- undoes the scale exactly.
inline int channel_shift(double max_abs) { return max_abs > 0.0 && std::isfinite(max_abs) ? std::min(100, std::max(-100, 10 - ilogb(max_abs))) : 0; }

// The f16 towers' stream shifts (evaluator.hip, choose_stream_shift, has the why).  s2[k] = sum of gamma^2 + beta^2 of stream channel k over
// the BatchNorms that write the stream, so sqrt(s2[k]) = s_k estimates the channel's RMS.  stream_shift_global: S = sqrt(median s2); 0 for
// S >= 1/2 (and for S = 0 or not finite), else -floor(log2 S), at most STREAM_SHIFT_MAX.
constexpr int STREAM_SHIFT_MAX = 16;
inline int stream_shift_global(std::vector<double> s2) {
    const size_t n = s2.size();
    if (!n) return 0;
    std::sort(s2.begin(), s2.end());
    const double S = std::sqrt(n % 2 ? s2[n / 2] : 0.5 * (s2[n / 2 - 1] + s2[n / 2]));
    if (!(S > 0.0) || !std::isfinite(S) || S >= 0.5) return 0;
    return std::min(STREAM_SHIFT_MAX, -ilogb(S));
}
// Channel k's own shift t_k = t + r_k >= t, t the global one: r_k = 0 where s_k 2^t >= 1/2 and where s_k is 0 (a dead channel) or not
// finite; a smaller channel is lifted into [1, 2), r_k = -floor(log2(s_k 2^t)), with t_k at most STREAM_SHIFT_MAX -- a bound on every
// exponent that the f32 products w 2^-t_k and the per-channel weight scales (channel_shift: within +-100) have to absorb.
inline int stream_shift_channel(double s2_k, int t) {
    const double s = std::sqrt(s2_k);
    if (!(s > 0.0) || !std::isfinite(s) || ldexp(s, t) >= 0.5) return t;
    return std::min(STREAM_SHIFT_MAX, -ilogb(s));  // = t - floor(log2(s 2^t)) > t
}
// `ceiling`: the rule above lifts a channel below the median and never holds back one far above it -- a median at 2^-8 beside channels at 1
// carries those at 2^8.  The direct form (f16 range 65,504) and the F(2x2) form (cap 16,376) have the room; the F(4x4) form, capped at 655,
// does not, so the estimate path passes it a ceiling (WINOF4_STREAM_CEILING below): while t_k > 0 and s_k 2^t_k >= ceiling, t_k drops
// by one.  The guard stops at 0 -- a stream is never shifted down -- so a guarded t_k can lie below the global shift, which stays
// stream_shift_global(s2).  A dead channel (s_k = 0) and one whose s_k is not finite keep the global shift, as they do above.  The
// default is no ceiling: every shift as it was (a finite s_k 2^16 is a finite double, never >= infinity).
constexpr double STREAM_NO_CEILING = HUGE_VAL;
inline std::vector<int> stream_shifts(const std::vector<double>& s2, double ceiling = STREAM_NO_CEILING) {
    const int t = stream_shift_global(s2);
    std::vector<int> tk(s2.size());
    for (size_t k = 0; k < s2.size(); k++) {
        tk[k] = stream_shift_channel(s2[k], t);
        const double s = std::sqrt(s2[k]);
        while (tk[k] > 0 && std::isfinite(s) && ldexp(s, tk[k]) >= ceiling) tk[k]--;
    }
    return tk;
}

// The same shifts from measurement (cattus_hip_create_calibrated): s2_measured[k] is the mean square of stream channel k over sample
// positions, taken on the exact f32 tower, abs_max[k] its largest |value| there -- what the gamma / beta sums only estimate (they miss
// a scale carried by the conv rows or the running statistics).  The rule is stream_shifts, fed with the measured mean squares; then a
// headroom guard, which the estimate has nothing to apply to: while t_k > 0 and abs_max[k] 2^t_k > STREAM_CAL_HEADROOM, t_k drops by
// one.  4096 = 2^12 is a quarter of the Winograd form's cap (WINO_ACT_MAX, 16376): a factor of four for positions outside the
// sample.  The guard stops at 0 -- a stream is never shifted down -- so a guarded t_k can lie below the global shift, which stays
// stream_shift_global(s2_measured).
// `headroom`: the F(4x4, 3x3) form passes a quarter of ITS cap (WINOF4_CAL_HEADROOM below).
constexpr double STREAM_CAL_HEADROOM = 4096.0;
// the headroom guard alone, on shifts from anywhere
inline std::vector<int> guarded_stream_shifts(std::vector<int> tk, const std::vector<double>& abs_max, double headroom = STREAM_CAL_HEADROOM) {
    for (size_t k = 0; k < tk.size() && k < abs_max.size(); k++)
        while (tk[k] > 0 && ldexp(abs_max[k], tk[k]) > headroom) tk[k]--;
    return tk;
}
inline std::vector<int> calibrated_stream_shifts(const std::vector<double>& s2_measured, const std::vector<double>& abs_max,
                                                 double headroom = STREAM_CAL_HEADROOM) {
    return guarded_stream_shifts(stream_shifts(s2_measured), abs_max, headroom);
}
// The single-term f16 Winograd tower (dtype f16w) keeps its stream in F32: a lift by 2^t commutes with every operation of it -- the rows,
// the one rounding of V = B^T d B and of U to 11 bits, the f32 sums -- as long as V stays a normal f16 number, and V's subnormal spacing
// (2^-24) stays below its ordinary rounding (rms 2^-12) for any channel whose rms is above 2^-12.  A measured lift therefore buys this
// tower nothing (measured: lifting a seeded network's stream by 2^3 .. 2^7 moved 29 of 15,040 logits, by at most 3e-8) and costs room
// under the cap.  What measurement does give it is the GUARD: calibrated, the tower runs the estimate's shifts (stream_shifts of the
// BatchNorm sums, as without calibration), each lowered while the channel's measured largest |value| 2^t_k exceeds the headroom.  A
// network whose estimate is right -- every seeded one -- keeps its shifts and its bits.
inline std::vector<int> calibrated_stream_shifts_f32_stream(const std::vector<int>& estimate, const std::vector<double>& abs_max,
                                                            double headroom = STREAM_CAL_HEADROOM) {
    return guarded_stream_shifts(estimate, abs_max, headroom);
}
constexpr double WINOF4_CAL_HEADROOM = WINOF4_ACT_MAX / 4;  // 163.75
// The F(4x4, 3x3) form's ceiling on the estimate path (stream_shifts' `ceiling`), where there is no abs_max to guard with.  2: a
// held-back channel ends with s_k 2^t_k in [1, 2) -- the point the lift rule aims at from below -- or at t_k = 0, its own size.  The
// estimate s_k stands for the channel's RMS; in float64 a channel's largest |value| is at most 3.4x its s_k on the seeded chess 2x128
// and 2x256 networks (median 1.5x, RMS 0.3x), so a channel held under 2 runs below 7 -- the guarded M8 twins of
// tests/test_winof4_range_gpu.py measure 4.8 and 4.3 where they ran at 864 and 986 -- of the 163.75 that calibration itself would
// allow (WINOF4_CAL_HEADROOM) and of the cap's 655: a factor of 24 and of 96 for what the estimate cannot see.  Every seeded network
// has t = 0, where the guard cannot act: the form's bits on them are what they were.
constexpr double WINOF4_STREAM_CEILING = 2.0;

// [cout_pad biases | cout_pad inverse scales 2^-shift]; without shifts (f32, bf16) the biases alone
inline std::vector<float> bias_and_scales(const Folded& f, const ConvShape& s, const std::vector<int>* shift = nullptr) {
    std::vector<float> b((size_t)(shift ? 2 : 1) * s.cout_pad, 0.0f);
    memcpy(b.data(), f.b.data(), s.cout * sizeof(float));
    for (uint32_t co = 0; shift && co < s.cout_pad; co++) b[s.cout_pad + co] = ldexpf(1.0f, -(*shift)[co]);
    return b;
}

// fn(t, co, ci, w) for every weight of the layer
template <class Fn>
void for_each_weight(const Folded& f, const ConvShape& s, Fn fn) {
    for (uint32_t t = 0; t < 9; t++)
        for (uint32_t co = 0; co < s.cout; co++)
            for (uint32_t ci = 0; ci < s.cin; ci++) fn(t, co, ci, f.w[((size_t)t * s.cout + co) * s.cin + ci]);
}

// channel_shift of every output channel over its 9 x cin weights (padded channels: 0)
inline std::vector<int> channel_shifts(const Folded& f, const ConvShape& s) {
    std::vector<float> m(s.cout_pad, 0.0f);
    for_each_weight(f, s, [&](uint32_t, uint32_t co, uint32_t, float w) { m[co] = std::max(m[co], fabsf(w)); });
    std::vector<int> sh(s.cout_pad);
    for (uint32_t co = 0; co < s.cout_pad; co++) sh[co] = channel_shift(m[co]);
    return sh;
}

// rows [9][cout_pad][cin_pad] of cvt(w, co)
template <class T, class Cvt>
std::vector<T> rows(const Folded& f, const ConvShape& s, Cvt cvt) {
    std::vector<T> w((size_t)9 * s.cout_pad * s.cin_pad, (T)0);
    for_each_weight(f, s, [&](uint32_t t, uint32_t co, uint32_t ci, float x) { w[((size_t)t * s.cout_pad + co) * s.cin_pad + ci] = cvt(x, co); });
    return w;
}
inline std::vector<float> rows_f32(const Folded& f, const ConvShape& s) { return rows<float>(f, s, [](float x, uint32_t) { return x; }); }
inline std::vector<uint16_t> rows_bf16(const Folded& f, const ConvShape& s) { return rows<uint16_t>(f, s, [](float x, uint32_t) { return f32_to_bf16(x); }); }
inline std::vector<_Float16> rows_f16(const Folded& f, const ConvShape& s, const std::vector<int>& shift) {  // single-term f16: f16(w 2^s)
    return rows<_Float16>(f, s, [&](float x, uint32_t co) { return (_Float16)ldexpf(x, shift[co]); });
}

// split precision: x as hi = f16(x), lo = f16(x - hi)
inline void split_f16(float x, _Float16& hi, _Float16& lo) { hi = (_Float16)x, lo = (_Float16)(x - (float)hi); }
// f16x2: the pair of w 2^s at at(t, co, ci, part 0 = hi / 1 = lo)
template <class Index>
std::vector<_Float16> split_weights(const Folded& f, const ConvShape& s, const std::vector<int>& shift, Index at) {
    std::vector<_Float16> w((size_t)9 * s.cout_pad * 2 * s.cin_pad, (_Float16)0.0f);
    for_each_weight(f, s, [&](uint32_t t, uint32_t co, uint32_t ci, float x) { split_f16(ldexpf(x, shift[co]), w[at(t, co, ci, 0)], w[at(t, co, ci, 1)]); });
    return w;
}
// rows [9][cout_pad][2 cin_pad]: [hi of 32 input channels | lo of the same 32] per 128 bytes (the LDS-ring kernel)
inline std::vector<_Float16> rows_f16x2(const Folded& f, const ConvShape& s, const std::vector<int>& shift) {
    return split_weights(f, s, shift, [&](uint32_t t, uint32_t co, uint32_t ci, uint32_t part) {
        return ((size_t)t * s.cout_pad + co) * 2 * s.cin_pad + (size_t)(ci >> 5) * 64 + (ci & 31) + 32 * part;
    });
}
// MFMA fragment order (CONV_W_FRAG, the register-ring kernels): a permutation of those rows
inline std::vector<_Float16> frag_f16x2(const Folded& f, const ConvShape& s, const std::vector<int>& shift) {
    return split_weights(f, s, shift, [&](uint32_t t, uint32_t co, uint32_t ci, uint32_t part) { return split_frag_index(t, co, ci, part, s.cin_pad); });
}

// Winograd F(2x2, 3x3) form: U = G g G^T per (cout, cin) in float64, [(co * cin + ci) * 16 + frequency], and one scale per output
// channel over all 16 frequencies of all its input channels
inline std::vector<double> wino_transform(const Folded& f, const ConvShape& s, std::vector<int>* shift) {
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    std::vector<double> U((size_t)s.cout * s.cin * 16);
    shift->assign(s.cout_pad, 0);
    for (uint32_t co = 0; co < s.cout; co++) {
        double m = 0.0;
        for (uint32_t ci = 0; ci < s.cin; ci++) {
            double g[3][3], t[4][3];
            for (int ky = 0; ky < 3; ky++)
                for (int kx = 0; kx < 3; kx++) g[ky][kx] = f.w[((size_t)(ky * 3 + kx) * s.cout + co) * s.cin + ci];
            for (int i = 0; i < 4; i++)
                for (int kx = 0; kx < 3; kx++) t[i][kx] = G[i][0] * g[0][kx] + G[i][1] * g[1][kx] + G[i][2] * g[2][kx];
            for (int i = 0; i < 4; i++)
                for (int l = 0; l < 4; l++) {
                    const double u = t[i][0] * G[l][0] + t[i][1] * G[l][1] + t[i][2] * G[l][2];
                    U[((size_t)co * s.cin + ci) * 16 + i * 4 + l] = u;
                    m = std::max(m, fabs(u));
                }
        }
        (*shift)[co] = channel_shift(m);
    }
    return U;
}
// U 2^s as (hi, lo) pairs in the Winograd kernels' fragment order, with the stages their weight ring reads past the end
inline std::vector<_Float16> wino_u(const std::vector<double>& U, const ConvShape& s, const std::vector<int>& shift) {
    std::vector<_Float16> wu((size_t)16 * s.cout_pad * s.cin_pad * 2 + (size_t)WINO_RING_STAGES * 1024, (_Float16)0.0f);
    for (uint32_t co = 0; co < s.cout; co++)
        for (uint32_t ci = 0; ci < s.cin; ci++)
            for (uint32_t q = 0; q < 16; q++)
                split_f16((float)ldexp(U[((size_t)co * s.cin + ci) * 16 + q], shift[co]), wu[wino_frag_index(q, co, ci, 0, s.cin_pad)], wu[wino_frag_index(q, co, ci, 1, s.cin_pad)]);
    return wu;
}
// f16(U 2^s) alone, in the single-term f16 Winograd kernel's fragment order (dtype f16w; wino_f16_frag_index): half of wino_u's bytes
inline std::vector<_Float16> wino_u_f16(const std::vector<double>& U, const ConvShape& s, const std::vector<int>& shift) {
    std::vector<_Float16> wu(wino_f16_u_elems(s.cout_pad, s.cin_pad), (_Float16)0.0f);
    for (uint32_t co = 0; co < s.cout; co++)
        for (uint32_t ci = 0; ci < s.cin; ci++)
            for (uint32_t q = 0; q < 16; q++)
                wu[wino_f16_frag_index(q, co, ci, s.cin_pad)] = (_Float16)(float)ldexp(U[((size_t)co * s.cin + ci) * 16 + q], shift[co]);
    return wu;
}
// f32(U) alone, no scale, in the f32-operand Winograd kernel's fragment order (dtype f32w; wino_f32_frag_index): the float64 transform
// rounded once
inline std::vector<float> wino_u_f32(const std::vector<double>& U, const ConvShape& s) {
    std::vector<float> wu(wino_f32_u_elems(s.cout_pad, s.cin_pad), 0.0f);
    for (uint32_t co = 0; co < s.cout; co++)
        for (uint32_t ci = 0; ci < s.cin; ci++)
            for (uint32_t q = 0; q < 16; q++) wu[wino_f32_frag_index(q, co, ci, s.cin_pad)] = (float)U[((size_t)co * s.cin + ci) * 16 + q];
    return wu;
}

// Winograd F(4x4, 3x3) form (winof4_rule.h): U = G g G^T per (cout, cin) in float64, [(co * cin + ci) * 36 + frequency], and one scale
// per output channel over all 36 frequencies of all its input channels
inline std::vector<double> winof4_transform(const Folded& f, const ConvShape& s, std::vector<int>* shift) {
    std::vector<double> U((size_t)s.cout * s.cin * WINOF4_FREQ);
    shift->assign(s.cout_pad, 0);
    for (uint32_t co = 0; co < s.cout; co++) {
        double m = 0.0;
        for (uint32_t ci = 0; ci < s.cin; ci++) {
            double g[3][3], t[6][3];
            for (int ky = 0; ky < 3; ky++)
                for (int kx = 0; kx < 3; kx++) g[ky][kx] = f.w[((size_t)(ky * 3 + kx) * s.cout + co) * s.cin + ci];
            for (int i = 0; i < 6; i++)
                for (int kx = 0; kx < 3; kx++) t[i][kx] = WINOF4_G[i][0] * g[0][kx] + WINOF4_G[i][1] * g[1][kx] + WINOF4_G[i][2] * g[2][kx];
            for (int i = 0; i < 6; i++)
                for (int l = 0; l < 6; l++) {
                    const double u = t[i][0] * WINOF4_G[l][0] + t[i][1] * WINOF4_G[l][1] + t[i][2] * WINOF4_G[l][2];
                    U[((size_t)co * s.cin + ci) * WINOF4_FREQ + i * 6 + l] = u;
                    m = std::max(m, fabs(u));
                }
        }
        (*shift)[co] = channel_shift(m);
    }
    return U;
}
// U 2^s as (hi, lo) pairs in the F(4x4) kernel's fragment order (winof4_frag_index); the kernel reads nothing past the payload
inline std::vector<_Float16> winof4_u(const std::vector<double>& U, const ConvShape& s, const std::vector<int>& shift) {
    std::vector<_Float16> wu(winof4_u_elems(s.cout_pad, s.cin_pad), (_Float16)0.0f);
    for (uint32_t co = 0; co < s.cout; co++)
        for (uint32_t ci = 0; ci < s.cin; ci++)
            for (uint32_t q = 0; q < (uint32_t)WINOF4_FREQ; q++)
                split_f16((float)ldexp(U[((size_t)co * s.cin + ci) * WINOF4_FREQ + q], shift[co]), wu[winof4_frag_index(q, co, ci, 0, s.cin_pad)],
                          wu[winof4_frag_index(q, co, ci, 1, s.cin_pad)]);
    return wu;
}

}  // namespace cattus
