// Stand-alone check of calibrated_stream_shifts (cattus_amd/csrc/weight_layout.h; built and run by tests/test_stream_calibration.py with
// the host compiler: no HIP, no GPU).  Without arguments: the rule's fixed points.  With a file of cases, one per line --
// "F  s2[0] .. s2[F-1]  abs_max[0] .. abs_max[F-1]", numbers as strtod reads them (hex floats, inf, nan) -- it also prints
// "global t[0] .. t[F-1]" per case, which the test holds against its Python restatement.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "weight_layout.h"

using namespace cattus;

static int failures = 0;
#define CHECK(cond, ...) \
    do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

typedef std::vector<double> D;
typedef std::vector<int> I;

static double sq(double s) { return s * s; }

static void check_rule() {
    // headroom to spare: stream_shifts itself, fed with mean squares
    const D s2{1.0, sq(ldexp(1.5, -8)), 0.0, sq(2.0), sq(ldexp(1.0, -3)), 1.0};
    CHECK((calibrated_stream_shifts(s2, D(6, 1.0)) == stream_shifts(s2)) && (stream_shifts(s2) == I{0, 8, 0, 0, 3, 0}), "the rule without the guard");
    // the guard: abs_max 2^t_k may reach 4096 and not pass it
    const D small{sq(ldexp(1.0, -8))};
    CHECK((calibrated_stream_shifts(small, {16.0}) == I{8}), "abs_max 2^t = 4096 stays");
    CHECK((calibrated_stream_shifts(small, {nextafter(16.0, 0.0)}) == I{8}), "just under 4096 stays");
    CHECK((calibrated_stream_shifts(small, {nextafter(16.0, 17.0)}) == I{7}), "just over 4096 drops by one");
    CHECK((calibrated_stream_shifts(small, {33.0}) == I{6}), "drops until it fits");
    CHECK((calibrated_stream_shifts(small, {1e9}) == I{0}) && (calibrated_stream_shifts(small, {INFINITY}) == I{0}), "the guard stops at 0");
    CHECK((calibrated_stream_shifts({1.0}, {1e9}) == I{0}), "a channel that is not shifted is not touched");
    CHECK((calibrated_stream_shifts(small, {NAN}) == I{8}), "an abs_max that compares with nothing guards nothing");
    // below the global shift where one channel alone is large: the global shift stays the median's
    const D med{sq(ldexp(1.5, -8)), 1.0, sq(ldexp(1.5, -8))};
    CHECK((calibrated_stream_shifts(med, {0.05, 20.0, 0.05}) == I{8, 7, 8}) && stream_shift_global(med) == 8, "a guarded channel below the global shift");
    // cap, dead and non-finite channels, no channels
    CHECK((calibrated_stream_shifts({sq(ldexp(1.0, -30))}, {ldexp(1.0, -28)}) == I{16}), "the cap");
    CHECK((calibrated_stream_shifts({0.0, INFINITY, 1.0}, {0.0, INFINITY, 3.0}) == I{0, 0, 0}), "dead and non-finite channels");
    CHECK((calibrated_stream_shifts({NAN}, {1.0}) == I{0}), "nothing to go by");
    CHECK(calibrated_stream_shifts({}, {}).empty(), "no channels");
}

int main(int argc, char** argv) {
    check_rule();
    if (argc > 1) {
        std::ifstream in(argv[1]);
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            size_t F = 0;
            ls >> F;
            D v;
            for (std::string tok; ls >> tok;) v.push_back(strtod(tok.c_str(), nullptr));
            if (v.size() != 2 * F) {
                CHECK(false, "case '%s' does not hold 2 x %zu numbers", line.c_str(), F);
                continue;
            }
            const D s2(v.begin(), v.begin() + F), mx(v.begin() + F, v.end());
            printf("%d", stream_shift_global(s2));
            for (int t : calibrated_stream_shifts(s2, mx)) printf(" %d", t);
            printf("\n");
        }
    }
    printf(failures ? "%d check(s) failed\n" : "calibration rule ok\n", failures);
    return failures ? 1 : 0;
}
