// Stand-alone check of the stem's input-channel padding (cattus_amd/csrc/weight_layout.h: stem_cin_pad, stem_is_fused) and of the f16x2
// stem layouts that padding asks for (built and run by tests/test_stem_padding.py; host compiler, no HIP, no GPU).
#include <cstdio>
#include <cstdlib>

#include "weight_layout.h"

using namespace cattus;

static int failures = 0;
#define CHECK(cond, ...) \
    do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the four dtypes as the evaluator hands them to stem_cin_pad: channels per 128-byte row (kernels.h, act_kc), and whether rows hold pairs
struct Dtype { const char* name; uint32_t row_channels; bool f16x2; };
static const Dtype DTYPES[] = {{"f32", 32, false}, {"bf16", 64, false}, {"f16x2", 32, true}, {"f16", 64, false}};

static void check_rule() {
    for (const Dtype& t : DTYPES)
        for (uint32_t planes : {1u, 18u, 32u, 33u, 64u, 65u, 119u, 128u})
            for (bool sep : {false, true}) {
                const uint32_t c = stem_cin_pad(planes, t.row_channels, t.f16x2, sep);
                const bool fused = stem_is_fused(planes, sep);
                CHECK(fused == (planes <= 32 && !sep), "%s %u planes sep %d: fused %d", t.name, planes, sep, fused);
                CHECK(c >= planes && c - planes < 64, "%s %u planes sep %d: %u channels", t.name, planes, sep, c);
                if (t.f16x2 && fused) CHECK(c == 32, "f16x2 %u planes, fused stem: %u channels, want the one chunk of 32", planes, c);
                else if (t.f16x2) CHECK(c % 64 == 0 && c == (planes + 63) / 64 * 64, "f16x2 %u planes, packed: %u channels, want the next multiple of 64", planes, c);
                else if (t.row_channels == 64) CHECK(c == (planes + 63) / 64 * 64, "%s %u planes sep %d: %u channels, want the next multiple of 64", t.name, planes, sep, c);
                else CHECK(c == (planes + 31) / 32 * 32, "f32 %u planes sep %d: %u channels, want the next multiple of 32", planes, sep, c);
            }
}

// weight number k: 8 significant bits x (1 + 2^-12), so that every f16x2 pair has a lo half; distinct for k < 15 * 128
static float code(size_t k) { return ldexpf((float)(128 + k % 128), (int)(k / 128)) * (1.0f + ldexpf(1.0f, -12)); }

// the f16x2 stem of `cin` planes laid out for cin_pad channels, rows and fragment order: every weight where the index functions say,
// zero everywhere else (the padded channels, a whole chunk of them at cin_pad = 64 among them), and the scales of `ref_pad` channels
static void check_stem_layouts(uint32_t cout, uint32_t cin, uint32_t cout_pad, uint32_t cin_pad, uint32_t ref_pad) {
    const ConvShape s{cout, cin, cout_pad, cin_pad}, ref{cout, cin, cout_pad, ref_pad};
    Folded f;
    for (size_t k = 0; k < (size_t)9 * cout * cin; k++) f.w.push_back(code(k % (15 * 128)));
    for (uint32_t co = 0; co < cout; co++) f.b.push_back(0.5f + co);
    const std::vector<int> sh = channel_shifts(f, s), sh_ref = channel_shifts(f, ref);
    CHECK(sh == sh_ref, "zero channels moved a scale (cin_pad %u against %u)", cin_pad, ref_pad);
    CHECK(bias_and_scales(f, s, &sh) == bias_and_scales(f, ref, &sh_ref), "[biases | inverse scales] differ between cin_pad %u and %u", cin_pad, ref_pad);
    const auto wr = rows_f16x2(f, s, sh), wf = frag_f16x2(f, s, sh);
    const size_t size = (size_t)9 * cout_pad * 2 * cin_pad;
    CHECK(wr.size() == size && wf.size() == size, "buffer sizes");
    std::vector<char> ur(size), uf(size);
    auto take = [](std::vector<char>& u, size_t i) { return i < u.size() && !u[i] && (u[i] = 1); };
    for (uint32_t t = 0; t < 9; t++)
        for (uint32_t co = 0; co < cout; co++)
            for (uint32_t ci = 0; ci < cin; ci++) {
                _Float16 hi, lo;
                split_f16(ldexpf(f.w[((size_t)t * cout + co) * cin + ci], sh[co]), hi, lo);
                // kernels.h, Act::F16S: [hi of channels 32g .. 32g+31 | lo of the same 32] per 128 bytes
                const size_t rh = ((size_t)t * cout_pad + co) * 2 * cin_pad + (ci / 32) * 64 + ci % 32, rl = rh + 32;
                CHECK(take(ur, rh) && take(ur, rl) && wr[rh] == hi && wr[rl] == lo && (double)lo != 0.0, "rows (%u, %u, %u)", t, co, ci);
                const size_t fh = split_frag_index(t, co, ci, 0, cin_pad), fl = split_frag_index(t, co, ci, 1, cin_pad);
                CHECK(take(uf, fh) && take(uf, fl) && wf[fh] == hi && wf[fl] == lo, "fragment order (%u, %u, %u)", t, co, ci);
            }
    for (size_t i = 0; i < size; i++) {
        CHECK(ur[i] || (double)wr[i] == 0.0, "rows: element %zu is %g, no weight belongs there", i, (double)wr[i]);
        CHECK(uf[i] || (double)wf[i] == 0.0, "fragment order: element %zu is %g, no weight belongs there", i, (double)wf[i]);
    }
    // the padded channels by their own indices: every (tap, cout, channel >= cin) is zero in both halves
    for (uint32_t t = 0; t < 9; t++)
        for (uint32_t co = 0; co < cout_pad; co++)
            for (uint32_t ci = cin; ci < cin_pad; ci++)
                for (uint32_t part = 0; part < 2; part++) {
                    const size_t r = ((size_t)t * cout_pad + co) * 2 * cin_pad + (ci / 32) * 64 + ci % 32 + 32 * part;
                    CHECK((double)wr[r] == 0.0 && (double)wf[split_frag_index(t, co, ci, part, cin_pad)] == 0.0, "padded channel (%u, %u, %u) part %u", t, co, ci, part);
                }
}

int main() {
    check_rule();
    check_stem_layouts(5, 40, 64, 64, 96);  // 40 planes: 8 real channels in the second chunk; the scales of another padding
    check_stem_layouts(5, 18, 64, 64, 32);      // 18 planes packed separately: the second chunk all zero, the scales of the fused stem's layout
    printf(failures ? "%d check(s) failed\n" : "stem padding ok\n", failures);
    return failures ? 1 : 0;
}
