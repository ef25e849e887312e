// Stand-alone program around cattus_amd/csrc/f16r_rule.h (tests/test_f16r_rule.py builds it plain and under sanitizers): the epilogue of
// one output element against an independent restatement and against dtype f16's epilogue, the three lane buffers' roles through towers
// of 0 .. 6 blocks, and the tap layout of every point decoded out of buffers of the lane's size.  Prints what fails and "f16r rule ok"
// when nothing does.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "f16r_rule.h"

using namespace cattus;

static int failures = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            failures++;                    \
            printf("FAIL %s: ", #cond);    \
            printf(__VA_ARGS__);           \
            printf("\n");                  \
        }                                  \
    } while (0)

static uint16_t bits16(_Float16 h) {
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

// f32 -> f16, round to nearest even, written out on the bits (finite x >= 0 that does not overflow: the epilogue clamps first)
static uint16_t round_f16(float x) {
    const uint32_t u = tap_bits(x);
    const int e = (int)((u >> 23) & 255) - 127;
    if (x == 0.0f) return 0;
    if (e < -25) return 0;
    uint64_t man = (u & 0x7fffffu) | 0x800000u;  // 24 bits, value man * 2^(e - 23)
    const int shift = e >= -14 ? 13 : 13 + (-14 - e);  // bits dropped: to 11 significant bits, or to multiples of 2^-24
    const uint64_t keep = man >> shift, rest = man & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    uint64_t q = keep + ((rest > half || (rest == half && (keep & 1))) ? 1 : 0);
    if (e >= -14) {  // q in [2^10, 2^11]: 2^11 carries into the exponent by itself in the sum below
        return (uint16_t)(((uint32_t)(e + 15) << 10) + (uint32_t)(q - 1024));
    }
    return (uint16_t)q;  // subnormal (q == 1024: the smallest normal, the same bits)
}

// dtype f16's epilogue (kernels.hip, conv3x3_mfma_v2_kernel<_Float16>): the skip is an f16 value, the result one f16 value
static _Float16 f16_epilogue(float acc, float ds, float bias, _Float16 skip, bool has_skip, bool valid, bool* counted) {
    float v = __builtin_fmaf(acc, ds, bias);
    if (has_skip) v = v + (float)skip;
    const float y = valid && v > 0.0f ? v : 0.0f;
    *counted = valid && y > 65504.0f;
    return (_Float16)(y < 65504.0f ? y : 65504.0f);
}

static void check_epilogue() {
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    int differ = 0;
    for (int it = 0; it < 200000; it++) {
        const int s = (int)(rng() % 12);
        const float ds = ldexpf(1.0f, -s), acc = (float)(u(rng) * ldexp(1.0, s + (int)(rng() % 6))), bias = (float)u(rng);
        const float skip = (float)fabs(u(rng) * ldexp(1.0, (int)(rng() % 8) - 3));
        const bool has_skip = rng() & 1, valid = (rng() % 8) != 0;
        const F16rOut o = f16r_finish(acc, ds, bias, skip, has_skip, valid);
        // restated: the product with a power of two is exact, so one rounding of (acc ds + bias) in double is the fused multiply-add
        float v = (float)((double)acc * (double)ds + (double)bias);
        if (has_skip) v = v + skip;
        const float y = !valid ? 0.0f : v > 0.0f ? v : 0.0f;
        CHECK(tap_bits(o.stream) == tap_bits(y), "stream %a, restated %a", o.stream, y);
        CHECK(bits16(o.copy) == round_f16(y), "copy %04x, restated %04x of %a", bits16(o.copy), round_f16(y), y);
        CHECK(!o.counted, "counted at %a", y);
        CHECK(valid || (o.stream == 0.0f && bits16(o.copy) == 0), "a slot past the board holds %a", o.stream);
        // against dtype f16: without a skip the copy is that tower's value, bit for bit (a 0-block net, the stem, point 1's input)
        bool c16;
        if (!has_skip) CHECK(bits16(o.copy) == bits16(f16_epilogue(acc, ds, bias, (_Float16)0.0f, false, valid, &c16)), "no skip: not dtype f16's bits");
        // with one: the bound tests/test_f16r_gpu.py holds the device to (f16 rounds the skip and the result to 11 bits, ReLU is
        // 1-Lipschitz), where both values are normal f16 numbers -- below 2^-14 an f16 rounding is absolute, 2^-25
        if (has_skip && valid && skip >= 6.2e-5f) {
            const _Float16 r16 = f16_epilogue(acc, ds, bias, (_Float16)skip, true, true, &c16);
            const double d = fabs((double)o.stream - (double)(float)r16), p0 = skip, p2 = o.stream;
            if ((float)r16 >= 6.2e-5f || (float)r16 == 0.0f)
                CHECK(d <= ldexp(p0, -11) + ldexp(p2, -11) + ldexp(p0 + p2, -20), "skip bound: |%a - %a| = %g", o.stream, (double)(float)r16, d);
            differ += d > 0;
        }
    }
    CHECK(differ > 1000, "the f32 skip never differed from dtype f16's (%d)", differ);

    // the edges
    struct { float acc, ds, bias, skip; bool has_skip, valid; float stream; uint16_t copy; bool counted; } const edge[] = {
        {65504.0f, 1.0f, 0.0f, 0.0f, false, true, 65504.0f, 0x7bff, false},   // the largest f16 itself: kept, not counted
        {65505.0f, 1.0f, 0.0f, 0.0f, false, true, 65505.0f, 0x7bff, true},    // beyond it: the stream keeps it, the copy is clamped and counted
        {65519.0f, 1.0f, 0.0f, 0.0f, false, true, 65519.0f, 0x7bff, true},    // (would still round to 65504: counted by note_saturation's rule, y > 65504)
        {60000.0f, 1.0f, 0.0f, 60000.0f, true, true, 120000.0f, 0x7bff, true},  // the skip takes it over
        {1e6f, 1.0f, 0.0f, 0.0f, false, false, 0.0f, 0, false},               // a slot past the board: zero, not counted
        {-3.0f, 1.0f, 1.0f, 1.0f, true, true, 0.0f, 0, false},                // ReLU
        {NAN, 1.0f, 0.0f, 0.0f, false, true, 0.0f, 0, false},                 // a NaN sum fails `> 0`
        {1.0f, 1.0f, 0.0f, NAN, false, true, 1.0f, 0x3c00, false},            // no skip: the skip value is not read
        {INFINITY, 1.0f, 0.0f, 0.0f, false, true, INFINITY, 0x7bff, true},    // the stream is not clamped
        {2048.0f, 0.5f, 0.5f, 0.0f, false, true, 1024.5f, 0x6400, false},     // 1024.5 -> 1024 (ties to even) in the copy alone
    };
    for (const auto& t : edge) {
        const F16rOut o = f16r_finish(t.acc, t.ds, t.bias, t.skip, t.has_skip, t.valid);
        CHECK(tap_bits(o.stream) == tap_bits(t.stream) && bits16(o.copy) == t.copy && o.counted == t.counted, "edge acc %g skip %g: stream %g copy %04x counted %d", t.acc,
              t.skip, o.stream, bits16(o.copy), (int)o.counted);
    }
}

// The buffers through a pass: what tensor each holds, by name.  S<k> = the stream behind k blocks, A<k> its copy, M<k> block k's middle.
static void check_plan() {
    for (uint32_t blocks = 0; blocks <= 6; blocks++) {
        enum Kind { EMPTY, PLANES, STREAM, COPY, MIDDLE };
        struct Held { Kind kind; int index; } buf[4] = {{EMPTY, 0}, {EMPTY, 0}, {EMPTY, 0}, {PLANES, 0}};
        CHECK(f16r_layers(blocks) == 1 + 2 * blocks, "launches");
        for (uint32_t l = 0; l < f16r_layers(blocks); l++) {
            const F16rLayer fl = f16r_layer(l, blocks);
            const int i = l == 0 ? -1 : (int)(l - 1) / 2;
            const bool last = f16r_is_last(l, blocks);
            CHECK(last == (l + 1 == f16r_layers(blocks)), "last layer");
            CHECK(fl.reads >= 0 && fl.reads <= 3 && fl.writes >= 0 && fl.writes <= 2, "layer %u: buffers", l);
            CHECK(fl.reads != fl.writes && fl.reads != fl.writes_copy, "layer %u reads a buffer it writes: a neighbour's rows would change under it", l);
            CHECK(fl.writes_copy == F16R_NONE || (fl.writes_copy != fl.writes && fl.writes_copy != fl.adds), "layer %u: the copy lies over another tensor", l);
            if (l == 0) {
                CHECK(f16r_stream_layer(l) && buf[fl.reads].kind == PLANES && fl.adds == F16R_NONE, "the stem reads the planes and adds nothing");
            } else if (l & 1) {
                CHECK(!f16r_stream_layer(l) && buf[fl.reads].kind == COPY && buf[fl.reads].index == i && fl.adds == F16R_NONE && fl.writes_copy == F16R_NONE,
                      "conv1 of block %d reads the copy of the stream behind %d blocks", i, i);
            } else {
                CHECK(f16r_stream_layer(l) && buf[fl.reads].kind == MIDDLE && buf[fl.reads].index == i, "conv2 of block %d reads its middle", i);
                CHECK(fl.adds == fl.writes && buf[fl.adds].kind == STREAM && buf[fl.adds].index == i, "conv2 of block %d adds the stream behind %d blocks, in place", i, i);
            }
            CHECK((fl.writes_copy == F16R_NONE) == (last || !f16r_stream_layer(l)), "layer %u: a copy from every stream layer but the last", l);
            if (f16r_stream_layer(l)) {
                CHECK(fl.writes == F16R_S, "the stream stays in its buffer");
                buf[fl.writes] = Held{STREAM, i + 1};
                if (fl.writes_copy != F16R_NONE) buf[fl.writes_copy] = Held{COPY, i + 1};
            } else {
                buf[fl.writes] = Held{MIDDLE, i};
            }
            // what a tap of this point reads is what the layer has just written
            CHECK(f16r_tap_buffer(l) == fl.writes, "point %u is tapped from the buffer its layer wrote", l);
            CHECK(f16r_tap_shifted(l) == f16r_stream_layer(l), "point %u: the stream points alone carry the shifts", l);
        }
        CHECK(buf[f16r_head_input()].kind == STREAM && buf[f16r_head_input()].index == (int)blocks, "the heads read the stream behind all %u blocks", blocks);
    }
    CHECK(F16R_S != F16R_A && F16R_S != F16R_M && F16R_A != F16R_M, "three buffers");
}

static void check_taps() {
    // a lane buffer is bpad * slots * fpad * 4 bytes whichever tensor it holds: every point decodes inside it, in its own layout
    const uint32_t shapes[][4] = {{8, 64, 64, 128}, {11, 121, 128, 64}, {3, 9, 64, 64}, {8, 64, 64, 16}};  // board, hw, slots, filters
    for (const auto& sh : shapes) {
        const uint32_t hw = sh[1], slots = sh[2], F = sh[3], FP = (F + 63) / 64 * 64, leaves = 256 / slots * 2, n = leaves - 1;
        const size_t bytes = (size_t)leaves * slots * FP * 4;
        std::vector<int> shifts(F);
        for (uint32_t c = 0; c < F; c++) shifts[c] = (int)(c % 5) - 1;
        for (uint32_t l = 0; l < 5; l++) {
            const TapSource s = f16r_tap_source(l, F, hw, slots, FP);
            CHECK(s.layout == (l % 2 == 0 ? (uint32_t)TAP_ROWS_F32 : (uint32_t)TAP_ROWS_F16) && s.C == F && s.hw == hw && s.slots == slots && s.pitch == FP, "point %u: source", l);
            std::vector<char> buf(bytes, 0);  // exactly the lane's allocation: the sanitizers see a decode past it
            const uint32_t esz = l % 2 == 0 ? 4 : 2;
            for (uint32_t leaf = 0; leaf < n; leaf++)
                for (uint32_t c = 0; c < F; c++)
                    for (uint32_t p = 0; p < hw; p++) {
                        const size_t at = tap_offset(s, leaf, c, p);
                        CHECK(at + esz <= bytes, "point %u: element (%u, %u, %u) at byte %zu of %zu", l, leaf, c, p, at, bytes);
                        if (at + esz > bytes) return;
                        const float x = (float)((leaf * 131 + c * 7 + p) % 2048) * 0.25f;  // exact in f16
                        const _Float16 h = (_Float16)x;
                        memcpy(buf.data() + at, esz == 4 ? (const void*)&x : (const void*)&h, esz);
                    }
            const int* const tk = f16r_tap_shifted(l) ? shifts.data() : nullptr;
            for (uint32_t leaf = 0; leaf < n; leaf++)
                for (uint32_t c = 0; c < F; c++)
                    for (uint32_t p = 0; p < hw; p += 7) {
                        const float want = (float)((leaf * 131 + c * 7 + p) % 2048) * 0.25f * (tk ? ldexpf(1.0f, -shifts[c]) : 1.0f);
                        const float got = tap_decode(s, buf.data(), tk, leaf, c, p);
                        CHECK(tap_bits(got) == tap_bits(want), "point %u (%u, %u, %u): %a, wanted %a", l, leaf, c, p, got, want);
                    }
        }
    }
}

int main() {
    check_epilogue();
    check_plan();
    check_taps();
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("f16r rule ok\n");
    return 0;
}
