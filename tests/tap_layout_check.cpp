// Stand-alone check of the observation layouts and of the trace record's rule (cattus_amd/csrc/tap_layout.h; built and run by
// tests/test_tap_layout.py with the host compiler, once plain and once under AddressSanitizer / UBSan: no HIP, no GPU).  Reads a file of
// cases:
//   "T layout C hw slots pitch vhc kvp kpp hv_pol n in.bin out.bin nshifts t[0] .. t[nshifts-1]"
//        one tensor: in.bin is the buffer as an evaluator would hold it (read into an allocation of exactly its size: an address past
//        it is AddressSanitizer's to find), decoded through tap_decode into out.bin, f32 [n][C][hw]; nshifts is 0 or C
//   "R count x[0] ref[0] .. x[count-1] ref[count-1]"
//        one leaf of a trace, floats as the hex of their 32 bits so that every NaN and both zeros arrive as they were written
//        -> the 32 bytes of its record as eight hex words
// and ends with "tap layout ok" when its own fixed points hold too.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "tap_layout.h"

using namespace cattus;

static int failures = 0;
#define CHECK(cond, ...) \
    do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check_fixed_points() {
    const float inf = INFINITY, nan = NAN;
    // the widenings: one, the largest f16, the smallest subnormal, a negative zero, an infinity
    CHECK(tap_widen_f16(0x3c00) == 1.0f && tap_widen_f16(0x7bff) == 65504.0f && tap_widen_f16(0x0001) == 5.9604644775390625e-08f, "f16 widening");
    CHECK(tap_bits(tap_widen_f16(0x8000)) == 0x80000000u && tap_widen_f16(0xfc00) == -inf && tap_widen_f16(0x7e00) != tap_widen_f16(0x7e00), "f16 specials");
    CHECK(tap_widen_bf16(0x3f80) == 1.0f && tap_widen_bf16(0xc000) == -2.0f, "bf16 widening");
    CHECK(tap_pow2(0) == 1.0f && tap_pow2(-16) == 1.52587890625e-05f && tap_pow2(7) == 128.0f, "powers of two");
    // the fragment order of the heads is the one the kernels write (device_common.h, frag_packed_index): spot values of the formula
    CHECK(tap_frag_index(0, 0, 16, 4) == 0 && tap_frag_index(1, 0, 16, 4) == 4 && tap_frag_index(0, 4, 16, 4) == 128 && tap_frag_index(0, 8, 16, 4) == 256, "f32 fragment order");
    CHECK(tap_frag_index(33, 9, 32, 2) == 32 * 32 + (size_t)((0 * 2 + 1) * 32 + 1) * 8 + 1, "bf16 fragment order, second leaf tile");
    // a record: a tie takes the lower index in whatever order the elements arrive, a NaN difference takes no part but is flagged
    const float x[6] = {0.0f, 2.0f, 0.5f, 2.0f, nan, 0.0f}, r[6] = {0.0f, 1.0f, 0.0f, 3.0f, 0.0f, 0.0f};
    const TraceRecord t = trace_leaf(x, r, 6);
    CHECK(t.max_diff == 1.0f && t.at == 1 && t.x == 2.0f && t.ref == 1.0f && t.flags == TRACE_NONFINITE, "a tie and a NaN: %g at %u, flags %u", t.max_diff, t.at, t.flags);
    CHECK(tap_bits(t.rms_diff) == 0x7fc00000u && t.rms_ref == (float)sqrt(10.0 / 6.0),"rms with a NaN on the x side: %08x %g", tap_bits(t.rms_diff), t.rms_ref);
    for (int split = 0; split <= 6; split++) {  // two partials, the later elements first
        TracePartial a = trace_partial(), b = trace_partial();
        for (int i = 5; i >= split; i--) trace_take(b, x[i], r[i], (uint32_t)i);
        for (int i = split - 1; i >= 0; i--) trace_take(a, x[i], r[i], (uint32_t)i);
        trace_combine(a, b);
        const TraceRecord c = trace_finish(a, 6);
        CHECK(c.max_diff == 1.0f && c.at == 1 && c.flags == TRACE_NONFINITE, "split at %d: %g at %u", split, c.max_diff, c.at);
    }
    const float same[3] = {1.5f, -2.0f, inf};
    const TraceRecord z = trace_leaf(same, same, 2);
    CHECK(z.max_diff == 0.0f && z.at == 0 && z.x == 1.5f && z.ref == 1.5f && z.rms_diff == 0.0f && z.flags == 0, "nothing differs: index 0");
    const TraceRecord w = trace_leaf(same + 2, same + 1, 1);
    CHECK(w.max_diff == inf && w.at == 0 && w.x == inf && w.ref == -2.0f && w.flags == TRACE_NONFINITE, "an infinity against a finite value");
}

static std::vector<char> read_all(const std::string& path) {
    std::ifstream in(path, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    check_fixed_points();
    if (argc > 1) {
        std::ifstream in(argv[1]);
        if (!in) {
            printf("cannot read %s\n", argv[1]);
            return 2;
        }
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            std::string kind;
            ls >> kind;
            if (kind == "T") {
                TapSource s{};
                uint32_t n = 0, nshifts = 0;
                std::string src, dst;
                ls >> s.layout >> s.C >> s.hw >> s.slots >> s.pitch >> s.vhc >> s.kvp >> s.kpp >> s.hv_pol >> n >> src >> dst >> nshifts;
                std::vector<int> shifts(nshifts);
                for (int& t : shifts) ls >> t;
                CHECK(!ls.fail() && (nshifts == 0 || nshifts == s.C), "bad line: %s", line.c_str());
                const std::vector<char> buf = read_all(src);  // exactly the file's bytes
                std::vector<float> out((size_t)n * s.C * s.hw);
                for (uint32_t leaf = 0; leaf < n; leaf++)
                    for (uint32_t c = 0; c < s.C; c++)
                        for (uint32_t p = 0; p < s.hw; p++)
                            out[((size_t)leaf * s.C + c) * s.hw + p] = tap_decode(s, buf.data(), nshifts ? shifts.data() : nullptr, leaf, c, p);
                std::ofstream o(dst, std::ios::binary);
                o.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * 4));
                CHECK(o.good(), "cannot write %s", dst.c_str());
            } else if (kind == "R") {
                uint32_t count = 0;
                ls >> count >> std::hex;
                std::vector<float> x(count), r(count);  // exactly count each
                for (uint32_t i = 0; i < count; i++) {
                    uint32_t ux = 0, ur = 0;
                    ls >> ux >> ur;
                    x[i] = tap_from_bits(ux), r[i] = tap_from_bits(ur);
                }
                CHECK(!ls.fail() && count >= 1, "bad line: %s", line.c_str());
                const TraceRecord t = trace_leaf(x.data(), r.data(), count);
                uint32_t wds[8];
                memcpy(wds, &t, 32);
                printf("%08x %08x %08x %08x %08x %08x %08x %08x\n", wds[0], wds[1], wds[2], wds[3], wds[4], wds[5], wds[6], wds[7]);
            }
        }
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("tap layout ok\n");
    return 0;
}
