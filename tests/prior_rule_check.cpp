// Stand-alone check of the prior rule (cattus_amd/csrc/prior_rule.h; built and run by tests/test_prior_rule.py with the host compiler,
// once plain and once under AddressSanitizer / UBSan: no HIP, no GPU).  Reads a file of cases, floats as the hex of their 32 bits:
//   "L legal_count stride va vb pa[0] pb[0] .. pa[stride-1] pb[stride-1]"   one leaf -> the eight 32-bit words of its record
//   "F w0 .. w7  w0 .. w7  ..."      records (eight words each) folded in order into a fresh sticky record ->
//                                    "leaves flips nonfinite empty sum_tv sum_regret max_tv max_regret h0 .. h7 holder"
//                                    (doubles as the hex of their 64 bits; holder: the index of the record that holds max_tv, -1 for none)
//   "V a0 b0 a1 b1 ..."              value pairs folded in order -> "value_leaves sum_dvalue"
// and ends with "prior rule ok" when its own fixed points hold too.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "prior_rule.h"

using namespace cattus;

static int failures = 0;
#define CHECK(cond, ...) \
    do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static unsigned long long bits64(double d) {
    unsigned long long u;
    memcpy(&u, &d, 8);
    return u;
}

static void check_fixed_points() {
    const float a[4] = {0.5f, 0.25f, 0.25f, 0.0f}, b[4] = {0.25f, 0.5f, 0.25f, 0.0f};
    const PriorRecord same = prior_leaf(a, a, 4, 4, 0.5f, 0.5f);
    CHECK(same.tv == 0.0f && same.regret == 0.0f && same.top_a == same.top_b && same.max_dp == 0.0f && same.k_max == 0 && same.flags == 0 && same.count == 4,
          "identical rows");
    const PriorRecord swap = prior_leaf(a, b, 4, 4, 0.5f, -0.5f);
    CHECK(swap.tv == 0.25f && swap.top_a == 0 && swap.top_b == 1 && swap.regret == 0.25f && swap.max_dp == 0.25f && swap.k_max == 0 && swap.dvalue == 1.0f,
          "two entries swapped: tv %g regret %g", swap.tv, swap.regret);
    const float tie[3] = {0.25f, 0.375f, 0.375f};
    const PriorRecord t = prior_leaf(tie, tie, 3, 3, 0.0f, 0.0f);
    CHECK(t.top_a == 1 && t.top_b == 1, "the lowest index holds a tie");
    const PriorRecord none = prior_leaf(a, b, 0, 4, 0.0f, 0.0f);
    CHECK(none.flags == PRIOR_EMPTY && none.count == 0 && none.tv == 0.0f && none.regret == 0.0f, "no legal move");
    const PriorRecord cut = prior_leaf(a, b, 9, 3, 0.0f, 0.0f);
    CHECK(cut.flags == PRIOR_TRUNCATED && cut.count == 3, "legal_count above the stride");
    const float bad[2] = {NAN, 1.0f};
    const PriorRecord n = prior_leaf(bad, b, 2, 2, INFINITY, 0.0f);
    CHECK(n.flags == (PRIOR_NONFINITE | PRIOR_VALUE_NONFINITE) && bits(n.tv) == 0x7fc00000u && bits(n.regret) == 0x7fc00000u && n.top_a == 1, "a NaN probability");
    // the histogram's edges: a tv that equals an edge belongs to the next bucket
    CHECK(prior_bucket(0.0f) == 0 && prior_bucket(1.0f) == 7 && prior_bucket(0.5f) == 7 && prior_bucket(0.05f) == 6, "buckets");
    // strictly larger replaces, the first of equals stays
    PriorStats s;
    PriorRecord r = same;
    CHECK(prior_fold(s, r) && s.seeded && s.max_tv == 0.0f, "the first compared leaf seeds the entry");
    CHECK(!prior_fold(s, r), "an equal tv replaces nothing");
    r.tv = 0.125f;
    CHECK(prior_fold(s, r) && !prior_fold(s, r) && s.max_tv == 0.125f && s.leaves == 4, "a strictly larger one does");
    CHECK(!prior_fold(s, none) && !prior_fold(s, n) && s.empty == 1 && s.nonfinite == 1 && s.leaves == 6 && s.sum_tv == 0.25, "flagged leaves enter no sum");
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
            if (kind == "L") {
                uint32_t count = 0, stride = 0, uva = 0, uvb = 0;
                ls >> std::dec >> count >> stride >> std::hex >> uva >> uvb;
                std::vector<float> a(stride), b(stride);  // exactly `stride` each: a read past a row is AddressSanitizer's to find
                for (uint32_t k = 0; k < stride; k++) {
                    uint32_t ua = 0, ub = 0;
                    ls >> ua >> ub;
                    a[k] = from_bits(ua), b[k] = from_bits(ub);
                }
                const PriorRecord r = prior_leaf(a.data(), b.data(), count, stride, from_bits(uva), from_bits(uvb));
                uint32_t w[8];
                memcpy(w, &r, 32);
                for (int i = 0; i < 8; i++) printf("%08x%c", w[i], i == 7 ? '\n' : ' ');
            } else if (kind == "F") {
                PriorStats s;
                long holder = -1, at = 0;
                ls >> std::hex;
                for (;; at++) {
                    uint32_t w[8];
                    bool whole = true;
                    for (int i = 0; i < 8; i++) whole = whole && (ls >> w[i]);
                    if (!whole) break;
                    PriorRecord r;
                    memcpy(&r, w, 32);
                    if (prior_fold(s, r)) holder = at;
                }
                ls.clear();
                printf("%llu %llu %llu %llu %016llx %016llx %08x %08x", (unsigned long long)s.leaves, (unsigned long long)s.top1_flips,
                       (unsigned long long)s.nonfinite, (unsigned long long)s.empty, bits64(s.sum_tv), bits64(s.sum_regret), bits(s.max_tv), bits(s.max_regret));
                for (int i = 0; i < PRIOR_BUCKETS; i++) printf(" %llu", (unsigned long long)s.tv_hist[i]);
                printf(" %ld\n", holder);
            } else if (kind == "V") {
                PriorStats s;
                uint32_t ua = 0, ub = 0;
                ls >> std::hex;
                while (ls >> ua >> ub) prior_fold_value(s, from_bits(ua), from_bits(ub));
                ls.clear();
                printf("%llu %016llx\n", (unsigned long long)s.value_leaves, bits64(s.sum_dvalue));
            }
            CHECK(!ls.fail(), "bad line: %s", line.c_str());
        }
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("prior rule ok\n");
    return 0;
}
