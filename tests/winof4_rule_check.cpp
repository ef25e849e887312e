// Stand-alone check of cattus_amd/csrc/winof4_rule.h and of the F(4x4, 3x3) entries of weight_layout.h (built and run by
// tests/test_winof4_rule.py -- plain and under AddressSanitizer + UBSan; host compiler, no HIP, no GPU).
//
// Cases come from a file, one per line, numbers as the hex of their bits; the answers go to stdout the same way and the test compares
// them with its numpy restatement:
//   I <36 x u32>            a 6x6 patch d (f32)           -> the 36 values of V = B^T d B (winof4_input_2d<float>)
//   O <36 x u32>            a 6x6 M (f32)                 -> the 16 values of Y = A^T M A (winof4_output_2d<float>)
//   D <9 x u64> <36 x u64>  a 3x3 g and a 6x6 d (f64)     -> the 16 values of A^T [(G g G^T) . (B^T d B)] A in float64
//   S <h x u64> <n> <n x u64 s2> <n x u64 abs_max>        -> calibrated_stream_shifts with the DEFAULT headroom, then with headroom h
//   C <c x u64> <n> <n x u64 s2>                          -> the global shift | stream_shifts with the DEFAULT (no) ceiling | with ceiling c
// Everything that needs no outside opinion -- geometry, the U index, winof4_u's decoding, the cap -- is checked in here.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>

#include "weight_layout.h"

using namespace cattus;

static int failures = 0;
#define CHECK(cond, ...) \
    do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static float f32_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static double f64_of(uint64_t u) { double f; memcpy(&f, &u, 8); return f; }
static uint64_t bits_of(double f) { uint64_t u; memcpy(&u, &f, 8); return u; }

static void check_geometry() {
    int owners[8][8] = {};
    for (int ty = 0; ty < 2; ty++)
        for (int tx = 0; tx < 2; tx++) {
            for (int p = 0; p < 4; p++)
                for (int q = 0; q < 4; q++) {
                    const int y = winof4_out_y(ty, p), x = winof4_out_x(tx, q);
                    CHECK(winof4_on_board(y, x), "output (%d, %d) of tile (%d, %d) is off the board", p, q, ty, tx);
                    if (winof4_on_board(y, x)) owners[y][x]++;
                    // output (p, q) reads patch pixels (p .. p + 2, q .. q + 2): board pixels (y - 1 .. y + 1, x - 1 .. x + 1)
                    CHECK(winof4_patch_y(ty, p) == y - 1 && winof4_patch_x(tx, q) == x - 1, "patch origin of tile (%d, %d)", ty, tx);
                }
            for (int a = 0; a < 6; a++)
                for (int b = 0; b < 6; b++) {
                    const int y = winof4_patch_y(ty, a), x = winof4_patch_x(tx, b);
                    CHECK(y == 4 * ty - 1 + a && x == 4 * tx - 1 + b, "patch pixel");
                    CHECK(winof4_on_board(y, x) == (y >= 0 && y <= 7 && x >= 0 && x <= 7), "on_board(%d, %d)", y, x);
                }
        }
    for (int y = 0; y < 8; y++)
        for (int x = 0; x < 8; x++) CHECK(owners[y][x] == 1, "pixel (%d, %d) is written by %d (tile, y, x)", y, x, owners[y][x]);
    CHECK(!winof4_on_board(-1, 0) && !winof4_on_board(0, -1) && !winof4_on_board(8, 0) && !winof4_on_board(0, 8) && winof4_on_board(0, 0) && winof4_on_board(7, 7), "board edges");
    int per_wave[4] = {};
    std::vector<char> seen(36);
    for (int f = 0; f < WINOF4_FREQ; f++) {
        const int w = winof4_wave_of(f), s = winof4_wave_slot(f);
        CHECK(w >= 0 && w < 4 && s >= 0 && s < WINOF4_WAVE_FREQ && w * WINOF4_WAVE_FREQ + s == f && !seen[w * 9 + s], "frequency %d -> wave %d slot %d", f, w, s);
        seen[w * 9 + s] = 1, per_wave[w]++;
    }
    for (int w = 0; w < 4; w++) CHECK(per_wave[w] == 9, "wave %d holds %d frequencies", w, per_wave[w]);
}

static void check_cap() {
    float worst = 0;
    for (int i = 0; i < 6; i++) {
        float s = 0;
        for (int a = 0; a < 6; a++) s += fabsf(WINOF4_BT[i][a]);
        worst = std::max(worst, s);
    }
    CHECK(worst == 10.0f && worst * worst * WINOF4_ACT_MAX <= 65504.0f && worst * worst * (WINOF4_ACT_MAX + 1) > 65504.0f, "cap derivation: row sum %g", worst);
    // the patch that reaches the bound: d[a][b] = cap x sign(B^T[0][a]) sign(B^T[0][b]) -- and its V is a finite f16 number
    float d[6][6], v[6][6];
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++) d[a][b] = WINOF4_ACT_MAX * (WINOF4_BT[0][a] < 0 ? -1.0f : 1.0f) * (WINOF4_BT[0][b] < 0 ? -1.0f : 1.0f);
    winof4_input_2d(d, v);
    float m = 0;
    for (auto& row : v)
        for (float x : row) m = std::max(m, fabsf(x));
    CHECK(m == 65500.0f && std::isfinite((float)(_Float16)m), "worst-case |V| = %g", m);
    CHECK(WINOF4_CAL_HEADROOM == 163.75 && STREAM_CAL_HEADROOM == 4096.0, "calibration headrooms");
    CHECK(WINOF4_STREAM_CEILING == 2.0 && std::isinf(STREAM_NO_CEILING) && STREAM_NO_CEILING > 0, "the estimate's ceiling");
}

// the U index: a bijection from (f, co, ci, part) onto [0, 36 x cout_pad x cin_pad x 2)
static void check_index(uint32_t cout_pad, uint32_t cin_pad) {
    const size_t n = winof4_u_elems(cout_pad, cin_pad);
    CHECK(n == (size_t)36 * cout_pad * cin_pad * 2, "payload size");
    std::vector<char> used(n);
    for (uint32_t f = 0; f < 36; f++)
        for (uint32_t co = 0; co < cout_pad; co++)
            for (uint32_t ci = 0; ci < cin_pad; ci++)
                for (uint32_t part = 0; part < 2; part++) {
                    const size_t i = winof4_frag_index(f, co, ci, part, cin_pad);
                    CHECK(i < n && !used[i], "index (%u, %u, %u, %u) -> %zu", f, co, ci, part, i);
                    if (i < n) used[i] = 1;
                    // what the kernel reads: stage (cout block, k-step, f) of 2,048 B, part, lane = 32 (k-half) + cout % 32, 8 channels
                    const size_t stage = ((size_t)(co / 32) * (cin_pad / 16) + ci / 16) * 36 + f;
                    CHECK(i == stage * WINOF4_STAGE_ELEMS + part * 512 + (((ci >> 3) & 1) * 32 + co % 32) * 8 + ci % 8, "index formula (%u, %u, %u, %u)", f, co, ci, part);
                }
    for (size_t i = 0; i < n; i++) CHECK(used[i], "element %zu belongs to nobody", i);
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double rnd() {  // (-1, 1)
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(rng_state >> 11) / (double)(1ull << 52) - 1.0;
}

// winof4_u of a random folded layer: (hi + lo) 2^-s is the float64 U to 2^-21 relative -- of the element, or, for the few elements
// below 2^-13 of their channel's largest (|U 2^s| < 1/8: the lo half is then an f16 subnormal), of that floor
static void check_u(uint32_t cout, uint32_t cin, uint32_t cout_pad, uint32_t cin_pad) {
    const ConvShape s{cout, cin, cout_pad, cin_pad};
    Folded f;
    for (size_t k = 0; k < (size_t)9 * cout * cin; k++) f.w.push_back((float)(rnd() * ldexp(1.0, (int)(k % 7) - 3)));
    f.b.assign(cout, 0.0f);
    std::vector<int> sh;
    const std::vector<double> U = winof4_transform(f, s, &sh);
    const std::vector<_Float16> wu = winof4_u(U, s, sh);
    CHECK(U.size() == (size_t)36 * cout * cin && wu.size() == winof4_u_elems(cout_pad, cin_pad) && sh.size() == cout_pad, "sizes");
    std::vector<char> used(wu.size());
    for (uint32_t co = 0; co < cout; co++) {
        double m = 0;
        for (uint32_t ci = 0; ci < cin; ci++)
            for (uint32_t q = 0; q < 36; q++) {
                const double u = U[((size_t)co * cin + ci) * 36 + q];
                m = std::max(m, fabs(u));
                // U = G g G^T against the matrices, term by term
                double want = 0;
                for (int ky = 0; ky < 3; ky++)
                    for (int kx = 0; kx < 3; kx++) want += WINOF4_G[q / 6][ky] * (double)f.w[((size_t)(ky * 3 + kx) * cout + co) * cin + ci] * WINOF4_G[q % 6][kx];
                CHECK(fabs(u - want) <= 1e-14 * (1.0 + fabs(want)), "U (%u, %u, %u) = %g, G g G^T = %g", co, ci, q, u, want);
                const size_t hi = winof4_frag_index(q, co, ci, 0, cin_pad), lo = winof4_frag_index(q, co, ci, 1, cin_pad);
                used[hi] = used[lo] = 1;
                const double x = ldexp(u, sh[co]), got = (double)wu[hi] + (double)wu[lo];
                CHECK(fabs(got - x) <= ldexp(1.0, -21) * std::max(fabs(x), 0.125), "U decode (%u, %u, %u): %.17g for %.17g", co, ci, q, got, x);
                CHECK(std::isfinite(got), "U (%u, %u, %u) left the f16 range", co, ci, q);
            }
        const double ms = ldexp(m, sh[co]);
        CHECK(ms >= 1024.0 && ms < 2048.0, "channel %u: largest |U 2^s| = %g", co, ms);
    }
    for (uint32_t co = cout; co < cout_pad; co++) CHECK(sh[co] == 0, "scale of padded channel %u", co);
    for (size_t i = 0; i < wu.size(); i++) CHECK(used[i] || (double)wu[i] == 0.0, "element %zu is %g, no weight belongs there", i, (double)wu[i]);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    check_geometry();
    check_cap();
    check_index(64, 32);
    check_index(96, 48);
    check_u(40, 20, 64, 32);
    std::string line;
    int c;
    while (true) {
        line.clear();
        while ((c = fgetc(in)) != EOF && c != '\n') line.push_back((char)c);
        if (line.empty() && c == EOF) break;
        if (line.empty()) continue;
        std::istringstream ss(line);
        char kind;
        ss >> kind >> std::hex;
        if (kind == 'I' || kind == 'O') {
            float m[6][6];
            for (auto& row : m)
                for (float& x : row) {
                    uint32_t u = 0;
                    ss >> u;
                    x = f32_of(u);
                }
            if (kind == 'I') {
                float v[6][6];
                winof4_input_2d(m, v);
                for (auto& row : v)
                    for (float x : row) printf("%08" PRIx32 " ", bits_of(x));
            } else {
                float y[4][4];
                winof4_output_2d(m, y);
                for (auto& row : y)
                    for (float x : row) printf("%08" PRIx32 " ", bits_of(x));
            }
            printf("\n");
        } else if (kind == 'D') {
            double g[3][3], d[6][6], t[6][3], u[6][6], v[6][6], m[6][6], y[4][4];
            uint64_t w = 0;
            for (auto& row : g)
                for (double& x : row) ss >> w, x = f64_of(w);
            for (auto& row : d)
                for (double& x : row) ss >> w, x = f64_of(w);
            for (int i = 0; i < 6; i++)
                for (int k = 0; k < 3; k++) t[i][k] = WINOF4_G[i][0] * g[0][k] + WINOF4_G[i][1] * g[1][k] + WINOF4_G[i][2] * g[2][k];
            for (int i = 0; i < 6; i++)
                for (int l = 0; l < 6; l++) u[i][l] = t[i][0] * WINOF4_G[l][0] + t[i][1] * WINOF4_G[l][1] + t[i][2] * WINOF4_G[l][2];
            winof4_input_2d(d, v);
            for (int i = 0; i < 6; i++)
                for (int l = 0; l < 6; l++) m[i][l] = u[i][l] * v[i][l];
            winof4_output_2d(m, y);
            for (auto& row : y)
                for (double x : row) printf("%016" PRIx64 " ", bits_of(x));
            printf("\n");
        } else if (kind == 'S') {
            uint64_t w = 0;
            size_t n = 0;
            ss >> w;
            const double headroom = f64_of(w);
            ss >> std::dec >> n >> std::hex;
            std::vector<double> s2(n), mx(n);
            for (double& x : s2) ss >> w, x = f64_of(w);
            for (double& x : mx) ss >> w, x = f64_of(w);
            for (int t : calibrated_stream_shifts(s2, mx)) printf("%d ", t);
            printf("| ");
            for (int t : calibrated_stream_shifts(s2, mx, headroom)) printf("%d ", t);
            printf("\n");
        } else if (kind == 'C') {
            uint64_t w = 0;
            size_t n = 0;
            ss >> w;
            const double ceiling = f64_of(w);
            ss >> std::dec >> n >> std::hex;
            std::vector<double> s2(n);
            for (double& x : s2) ss >> w, x = f64_of(w);
            const std::vector<int> plain = stream_shifts(s2), none = stream_shifts(s2, STREAM_NO_CEILING), held = stream_shifts(s2, ceiling);
            CHECK(plain == none, "the default is no ceiling");
            const int t = stream_shift_global(s2);
            for (size_t k = 0; k < n; k++) {
                CHECK(plain[k] == stream_shift_channel(s2[k], t), "channel %zu: the unguarded rule moved", k);
                CHECK(held[k] >= 0 && held[k] <= plain[k], "channel %zu: guarded %d, unguarded %d", k, held[k], plain[k]);
            }
            printf("%d | ", t);
            for (int x : plain) printf("%d ", x);
            printf("| ");
            for (int x : held) printf("%d ", x);
            printf("\n");
        } else {
            CHECK(false, "unknown case '%c'", kind);
        }
        if (!ss) CHECK(false, "short case line '%c'", kind);
    }
    fclose(in);
    printf(failures ? "%d check(s) failed\n" : "winof4 rule ok\n", failures);
    return failures ? 1 : 0;
}
