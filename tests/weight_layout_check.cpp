// Stand-alone check of cattus_amd/csrc/weight_layout.h (built and run by tests/test_weight_layout.py; host compiler, no HIP, no GPU):
// every layout puts each weight of a layer exactly once, at the index the kernels read it from, and zero everywhere else.
#include <cstdio>
#include <cstdlib>

#include "weight_layout.h"

using namespace cattus;

static int failures = 0;
#define CHECK(cond, ...) \
    do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// weight number k of a layer: an integer with 8 significant bits (exact in bf16 and f16), distinct for k < 15 * 128
static float code(size_t k) { return ldexpf((float)(128 + k % 128), (int)(k / 128)); }

struct Marks {  // which elements of a buffer a weight has claimed
    std::vector<char> used;
    bool take(size_t i) { return i < used.size() && !used[i] && (used[i] = 1); }
};
template <class T>
static void rest_is_zero(const char* what, const std::vector<T>& w, const Marks& m) {
    for (size_t i = 0; i < w.size(); i++) CHECK(m.used[i] || (double)w[i] == 0.0, "%s: element %zu is %g, no weight belongs there", what, i, (double)w[i]);
}
static float bf16_value(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// the direct layouts of a cout x cin layer padded to cout_pad x cin_pad
static void check_direct(uint32_t cout, uint32_t cin, uint32_t cout_pad, uint32_t cin_pad) {
    const ConvShape s{cout, cin, cout_pad, cin_pad};
    Folded f, f2;  // f2: the same codes x (1 + 2^-12) -- 20 significant bits, so that the f16x2 pairs have a lo half
    for (size_t k = 0; k < (size_t)9 * cout * cin; k++) f.w.push_back(code(k)), f2.w.push_back(code(k) * (1.0f + ldexpf(1.0f, -12)));
    for (uint32_t co = 0; co < cout; co++) f.b.push_back(0.5f + co), f2.b.push_back(0.5f + co);
    const std::vector<int> sh = channel_shifts(f, s), sh2 = channel_shifts(f2, s);
    const std::vector<float> bias = bias_and_scales(f, s), bs = bias_and_scales(f, s, &sh);
    CHECK(bias.size() == cout_pad && bs.size() == 2 * cout_pad, "bias buffer sizes");
    for (uint32_t co = 0; co < cout_pad; co++) {
        CHECK(bias[co] == (co < cout ? 0.5f + co : 0.0f) && bs[co] == bias[co], "bias of channel %u", co);
        CHECK(bs[cout_pad + co] == ldexpf(1.0f, -sh[co]) && (co < cout || sh[co] == 0), "inverse scale of channel %u", co);
    }
    const auto w32 = rows_f32(f, s);
    const auto wbf = rows_bf16(f, s);
    const auto w16 = rows_f16(f, s, sh);
    const auto wr = rows_f16x2(f2, s, sh2), wf = frag_f16x2(f2, s, sh2);
    CHECK(w32.size() == (size_t)9 * cout_pad * cin_pad && wbf.size() == w32.size() && w16.size() == w32.size(), "row buffer sizes");
    CHECK(wr.size() == 2 * w32.size() && wf.size() == wr.size(), "split buffer sizes");
    Marks m32{std::vector<char>(w32.size())}, mbf = m32, m16 = m32, mr{std::vector<char>(wr.size())}, mf = mr;
    for (uint32_t t = 0; t < 9; t++)
        for (uint32_t co = 0; co < cout; co++)
            for (uint32_t ci = 0; ci < cin; ci++) {
                const size_t k = ((size_t)t * cout + co) * cin + ci, row = ((size_t)t * cout_pad + co) * cin_pad + ci;  // kernels.h: w [9][cout][cin]
                const double want = f.w[k], want2 = f2.w[k], inv = ldexp(1.0, -sh[co]), inv2 = ldexp(1.0, -sh2[co]);
                CHECK(m32.take(row) && w32[row] == want, "f32 rows (%u, %u, %u)", t, co, ci);
                CHECK(mbf.take(row) && bf16_value(wbf[row]) == want, "bf16 rows (%u, %u, %u)", t, co, ci);
                CHECK(m16.take(row) && (double)w16[row] * inv == want, "f16 rows (%u, %u, %u)", t, co, ci);
                // kernels.h, Act::F16S: [hi of channels 32g .. 32g+31 | lo of the same 32] per 128 bytes
                const size_t hi = ((size_t)t * cout_pad + co) * 2 * cin_pad + (ci / 32) * 64 + ci % 32, lo = hi + 32;
                CHECK(mr.take(hi) && mr.take(lo) && (double)wr[lo] != 0.0 && ((double)wr[hi] + (double)wr[lo]) * inv2 == want2, "f16x2 rows (%u, %u, %u)", t, co, ci);
                const size_t fh = split_frag_index(t, co, ci, 0, cin_pad), fl = split_frag_index(t, co, ci, 1, cin_pad);
                CHECK(mf.take(fh) && mf.take(fl) && wf[fh] == wr[hi] && wf[fl] == wr[lo], "f16x2 fragment order (%u, %u, %u)", t, co, ci);
            }
    rest_is_zero("f32 rows", w32, m32), rest_is_zero("bf16 rows", wbf, mbf), rest_is_zero("f16 rows", w16, m16);
    rest_is_zero("f16x2 rows", wr, mr), rest_is_zero("f16x2 fragment order", wf, mf);
}

// Winograd U of one-hot 3x3 filters: filter (co, ci) is c = 1 + co * cin + ci at tap ((co + ci) % 9) = (ky, kx), so that
// U[i][l] = c G[i][ky] G[l][kx]
static void check_wino(uint32_t n, uint32_t pad) {
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    const ConvShape s{n, n, pad, pad};
    Folded f;
    f.w.assign((size_t)9 * n * n, 0.0f), f.b.assign(n, 0.25f);
    for (uint32_t co = 0; co < n; co++)
        for (uint32_t ci = 0; ci < n; ci++) f.w[((size_t)((co + ci) % 9) * n + co) * n + ci] = (float)(1 + co * n + ci);
    std::vector<int> sh;
    const std::vector<double> U = wino_transform(f, s, &sh);
    const auto wu = wino_u(U, s, sh);
    const size_t body = (size_t)16 * pad * pad * 2;
    CHECK(wu.size() == body + (size_t)WINO_RING_STAGES * 1024 && sh.size() == pad, "U buffer size");
    Marks m{std::vector<char>(wu.size())};
    for (uint32_t co = 0; co < n; co++)
        for (uint32_t ci = 0; ci < n; ci++)
            for (uint32_t q = 0; q < 16; q++) {
                const uint32_t ky = (co + ci) % 9 / 3, kx = (co + ci) % 9 % 3;
                const double want = (1.0 + co * n + ci) * G[q / 4][ky] * G[q % 4][kx];
                const size_t hi = wino_frag_index(q, co, ci, 0, pad), lo = wino_frag_index(q, co, ci, 1, pad);
                CHECK(hi < body && lo < body && m.take(hi) && m.take(lo), "U index (%u, %u, %u)", q, co, ci);
                CHECK(U[((size_t)co * n + ci) * 16 + q] == want && ((double)wu[hi] + (double)wu[lo]) * ldexp(1.0, -sh[co]) == want, "U value (%u, %u, %u)", q, co, ci);
            }
    rest_is_zero("U", wu, m);  // the padded channels and the ring's tail among them
    for (uint32_t co = n; co < pad; co++) CHECK(sh[co] == 0, "U scale of padded channel %u", co);
}

// the stream-shift rule on per-channel sums of gamma^2 + beta^2 (s2; s = sqrt(s2) is what the rule speaks of)
static void check_stream_shifts() {
    auto sq = [](double s) { return s * s; };
    // the global part: the median, 0 from 1/2 up, lifted into [1, 2) below, at most 16, 0 for nothing to go by
    CHECK(stream_shift_global({}) == 0 && stream_shift_global({sq(0.5)}) == 0 && stream_shift_global({sq(0.49)}) == 2, "global shift at 1/2");
    CHECK(stream_shift_global({sq(0.25), 1.0, sq(0.01)}) == 2 && stream_shift_global({1.0, sq(0.25), 1.0, sq(0.25)}) == 0, "global shift is the median's");
    CHECK(stream_shift_global({sq(ldexp(1.5, -8))}) == 8 && stream_shift_global({sq(ldexp(1.0, -30))}) == 16, "global shift size and cap");
    CHECK(stream_shift_global({0.0, 0.0, 1.0}) == 0 && stream_shift_global({INFINITY}) == 0 && stream_shift_global({NAN}) == 0, "global shift of 0 / inf / nan");
    // a channel: t where s 2^t >= 1/2, where s is 0 or not finite; else lifted into [1, 2), at most 16
    CHECK(stream_shift_channel(sq(0.75), 0) == 0 && stream_shift_channel(sq(0.5), 0) == 0 && stream_shift_channel(sq(300.0), 0) == 0, "channels that stay");
    CHECK(stream_shift_channel(0.0, 0) == 0 && stream_shift_channel(0.0, 5) == 5 && stream_shift_channel(INFINITY, 3) == 3 && stream_shift_channel(NAN, 3) == 3, "dead and non-finite channels");
    CHECK(stream_shift_channel(sq(0.49), 0) == 2 && stream_shift_channel(sq(0.25), 0) == 2 && stream_shift_channel(sq(0.2), 0) == 3, "channels just below 1/2");
    CHECK(stream_shift_channel(sq(ldexp(1.0, -8)), 0) == 8 && stream_shift_channel(sq(ldexp(1.99, -8)), 0) == 8 && stream_shift_channel(sq(ldexp(0.99, -8)), 0) == 9, "a channel at 2^-8");
    CHECK(stream_shift_channel(sq(ldexp(1.0, -8)), 8) == 8 && stream_shift_channel(sq(ldexp(1.0, -9)), 8) == 8 && stream_shift_channel(sq(ldexp(1.0, -10)), 8) == 10, "remainder on a shifted tower");
    CHECK(stream_shift_channel(sq(1.0), 8) == 8 && stream_shift_channel(sq(ldexp(1.0, -40)), 0) == 16 && stream_shift_channel(sq(ldexp(1.0, -40)), 16) == 16, "large channels; the cap");
    CHECK(stream_shift_channel(sq(ldexp(1.0, -600)), 0) == 0, "s2 underflows to 0: dead");
    for (int t = 0; t <= 16; t++)
        for (int e = -45; e <= 10; e++)
            for (double m : {1.0, 1.25, 1.999}) {
                const double s = ldexp(m, e);
                const int tk = stream_shift_channel(sq(s), t);
                CHECK(tk >= t && tk <= STREAM_SHIFT_MAX, "t_k %d outside [t, 16] (s %g, t %d)", tk, s, t);
                if (ldexp(s, t) >= 0.5) CHECK(tk == t, "s 2^t >= 1/2 moved (s %g, t %d)", s, t);
                else if (tk < STREAM_SHIFT_MAX) CHECK(ldexp(s, tk) >= 1.0 && ldexp(s, tk) < 2.0, "s 2^t_k = %g not in [1, 2) (s %g, t %d)", ldexp(s, tk), s, t);
            }
    // all of it: Q8-like (every fourth channel at 2^-8 beside unit ones), a dead channel, and the reverse (unit channels beside a small median)
    const std::vector<int> q = stream_shifts({1.0, sq(ldexp(1.5, -8)), 0.0, sq(2.0), sq(ldexp(1.0, -3)), 1.0});
    CHECK((q == std::vector<int>{0, 8, 0, 0, 3, 0}), "per-channel shifts beside a unit median");
    const std::vector<int> m = stream_shifts({sq(ldexp(1.5, -8)), 1.0, sq(ldexp(1.5, -8)), 0.0, sq(ldexp(1.5, -12)), sq(ldexp(1.5, -8)), sq(ldexp(1.5, -8))});
    CHECK((m == std::vector<int>{8, 8, 8, 8, 12, 8, 8}), "per-channel shifts beside a small median");
    CHECK(stream_shifts({}).empty(), "no channels");
}

int main() {
    check_stream_shifts();
    CHECK(channel_shift(0.0) == 0 && channel_shift(1.0) == 10 && channel_shift(1500.0) == 0 && channel_shift(2048.0) == -1 && channel_shift(INFINITY) == 0, "channel_shift");
    check_direct(3, 5, 64, 32);   // one 32-channel chunk
    check_direct(3, 70, 64, 96);  // three chunks (the third partly filled), both k-halves and both 8-groups of a chunk
    check_wino(128, 128);
    check_wino(130, 192);
    printf(failures ? "%d check(s) failed\n" : "weight layouts ok\n", failures);
    return failures ? 1 : 0;
}
