// Stand-alone check of the verification rule (cattus_amd/csrc/verify_rule.h; built and run by tests/test_verify_rule.py with the host
// compiler, once plain and once under AddressSanitizer / UBSan: no HIP, no GPU).  Reads a file of cases, floats as the hex of their
// 32 bits so that every NaN and both zeros arrive as they were written:
//   "P a b"                              one pair      -> "dlogit logit_inside value_inside dvalue"       (floats again as bit hex)
//   "L M va vb a[0] b[0] .. a[M-1] b[M-1]"   one leaf  -> "max_dlogit move dvalue flags"                  (the 16 bytes of its record)
// and ends with "verify rule ok" when its own fixed points hold too.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "verify_rule.h"

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

static void check_fixed_points() {
    const float MIN = -3.40282347e+38f, inf = INFINITY, nan = NAN;
    CHECK(verify_logit_inside(MIN, MIN) && verify_dlogit(MIN, MIN) == 0.0f, "two scrubbed logits are equal");
    CHECK(!verify_logit_inside(MIN, 1.0f) && !verify_logit_inside(1.0f, MIN), "a scrubbed logit against a finite one");
    CHECK(!verify_logit_inside(inf, inf) && !verify_logit_inside(nan, 0.0f) && !verify_logit_inside(0.0f, nan) && !verify_logit_inside(1.0f, -inf), "non-finite logits");
    CHECK(!verify_value_inside(inf, inf) && !verify_value_inside(nan, nan) && !verify_value_inside(0.5f, nan), "non-finite values");
    CHECK(verify_logit_inside(0.0f, -0.0f) && verify_value_inside(-0.0f, 0.0f), "the two zeros");
    CHECK(verify_value_inside(1.0f, 1.0f) && verify_value_inside(-1.0f, -1.0f) && !verify_value_inside(1.0f, -1.0f), "the tanh edge");
    CHECK(verify_value_inside(1.0f, 1.0f - 5.9604645e-8f) && !verify_value_inside(1.0f, 1.0f - 1.1e-5f), "one ulp below 1 is inside, 1.1e-5 below is not");
    CHECK(bits(verify_dvalue(nan, 0.0f)) == 0x7fc00000u && bits(verify_dvalue(inf, inf)) == 0x7fc00000u && verify_dvalue(inf, 0.0f) == inf, "dvalue of non-finite values");
    // the maximum does not depend on the order the moves arrive in, and the lowest index holds a tie
    const float a[6] = {0.0f, 2.0f, 0.5f, 2.0f, nan, 0.0f}, b[6] = {0.0f, 1.0f, 0.0f, 3.0f, 0.0f, 0.0f};
    const VerifyRecord r = verify_leaf(a, b, 6, 0.25f, 0.25f);
    CHECK(r.max_dlogit == 1.0f && r.move == 1 && r.dvalue == 0.0f && r.flags == VERIFY_LEAF_OUTSIDE, "a tie and a NaN: %g at %u, flags %u", r.max_dlogit, r.move, r.flags);
    float bd = 0.0f;
    uint32_t bi = 0xffffffffu;
    for (int i = 5; i >= 0; i--) verify_take_max(verify_dlogit(a[i], b[i]), (uint32_t)i, bd, bi);
    CHECK(bd == 1.0f && bi == 1, "the same from the back");
    const VerifyRecord z = verify_leaf(a, a + 0, 4, 1.0f, -1.0f);
    CHECK(z.max_dlogit == 0.0f && z.move == 0 && z.dvalue == 2.0f && z.flags == (VERIFY_LEAF_OUTSIDE | VERIFY_VALUE_OUTSIDE), "equal logits, opposite values");
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
            ls >> kind >> std::hex;
            if (kind == "P") {
                uint32_t ua = 0, ub = 0;
                ls >> ua >> ub;
                const float a = from_bits(ua), b = from_bits(ub);
                printf("%08x %d %d %08x\n", bits(verify_dlogit(a, b)), (int)verify_logit_inside(a, b), (int)verify_value_inside(a, b), bits(verify_dvalue(a, b)));
            } else if (kind == "L") {
                uint32_t M = 0, uva = 0, uvb = 0;
                ls >> std::dec >> M >> std::hex >> uva >> uvb;
                std::vector<float> a(M), b(M);  // exactly M each: a read past a row is AddressSanitizer's to find
                for (uint32_t m = 0; m < M; m++) {
                    uint32_t ua = 0, ub = 0;
                    ls >> ua >> ub;
                    a[m] = from_bits(ua), b[m] = from_bits(ub);
                }
                const VerifyRecord r = verify_leaf(a.data(), b.data(), M, from_bits(uva), from_bits(uvb));
                printf("%08x %08x %08x %08x\n", bits(r.max_dlogit), r.move, bits(r.dvalue), r.flags);
            }
            CHECK(!ls.fail(), "bad line: %s", line.c_str());
        }
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("verify rule ok\n");
    return 0;
}
