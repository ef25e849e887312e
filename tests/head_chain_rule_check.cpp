// Stand-alone program around cattus_amd/csrc/head_chain_rule.h (tests/test_head_chain_rule.py builds it plain and under sanitizers): the
// grid map of head_fc_chain_kernel as a bijection onto (leaf, output unit), the walk order against the order derived from the MFMA lane
// pair, the operand offsets against tap_frag_index and the operands' allocations, the dot product against a plain loop bit for bit, and
// the epilogues against restatements.  Prints what fails and "head chain rule ok" when nothing does.
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <limits>
#include <random>
#include <vector>

#include "head_chain_rule.h"

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

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

struct Shape {
    uint32_t J, K;
};
static const Shape SHAPES[] = {{128, 48}, {9, 48}, {49, 784}, {128, 784}, {1880, 512}, {128, 336}};

// ---- 1. the grid map: every (leaf < n, unit < J) exactly once, for FC1 (J = 128 hidden units) and for a policy FC of J moves ----
static void check_grid() {
    CHECK(hc_leaves_per_lane(1) == 1 && hc_leaves_per_lane(HC_SINGLE_MAX) == 1 && hc_leaves_per_lane(HC_SINGLE_MAX + 1) == 2, "leaves per lane");
    CHECK(HC_THREADS == HC_UNITS && HC_HIDDEN == HC_UNITS, "a workgroup is one strip, and FC1 is exactly one strip");
    for (const Shape& sh : SHAPES)
        for (uint32_t n = 1; n <= 70; n++)
            for (uint32_t forced_nl = 0; forced_nl <= 2; forced_nl++) {  // the rule's choice, and both forms at every n
                const uint32_t M = sh.J, nl = forced_nl ? forced_nl : hc_leaves_per_lane(n);
                const uint32_t gx = hc_grid_x(M), gy = hc_grid_y(n, nl);
                std::vector<int> fc1((size_t)n * HC_HIDDEN, 0), pol((size_t)n * M, 0);
                for (uint32_t bx = 0; bx < gx; bx++)
                    for (uint32_t by = 0; by < gy; by++)
                        for (uint32_t tid = 0; tid < HC_THREADS; tid++)
                            for (uint32_t s = 0; s < nl; s++) {
                                const HcOut o = hc_map(bx, by, tid, s, nl, n, M);
                                const uint32_t J = hc_part_units(o.part, M);
                                CHECK((o.part == HC_FC1) == (bx == 0), "part of block column %u", bx);
                                CHECK(hc_load_leaf(o.leaf, n) < n && hc_load_row(o.unit, J) < J, "a dead output loads inside: leaf %u unit %u", o.leaf, o.unit);
                                CHECK(o.live == (o.leaf < n && o.unit < J), "live");
                                if (o.live) CHECK(hc_load_leaf(o.leaf, n) == o.leaf && hc_load_row(o.unit, J) == o.unit, "a live output loads its own operands");
                                if (o.live) (o.part == HC_FC1 ? fc1[(size_t)o.leaf * HC_HIDDEN + o.unit] : pol[(size_t)o.leaf * M + o.unit])++;
                                // the slots of a thread share the weight row
                                CHECK(o.unit == hc_map(bx, by, tid, 0, nl, n, M).unit, "one weight row per thread");
                            }
                for (int c : fc1) CHECK(c == 1, "FC1 J %u n %u nl %u: an output produced %d times", M, n, nl, c);
                for (int c : pol) CHECK(c == 1, "policy J %u n %u nl %u: an output produced %d times", M, n, nl, c);
                // FC1 -> FC2: the 128 hidden units of a leaf come from one workgroup (block column 0, one row of the grid)
                for (uint32_t leaf = 0; leaf < n; leaf++) CHECK(leaf / nl < gy, "leaf %u has a workgroup", leaf);
            }
}

// ---- 2. the walk: k = 8u + 4h + j, walked u, then j, then h (Mfma<float>::mac: four MFMAs j = 0..3, each adds lane half 0's product, then half 1's) ----
static std::vector<uint32_t> mfma_order(uint32_t K) {
    std::vector<uint32_t> o;
    for (uint32_t u = 0; u < K / 8; u++)
        for (uint32_t j = 0; j < 4; j++)
            for (uint32_t h = 0; h < 2; h++) o.push_back(8 * u + 4 * h + j);
    return o;
}
static void check_walk() {
    for (const Shape& sh : SHAPES) {
        const std::vector<uint32_t> want = mfma_order(sh.K);
        std::vector<int> seen(sh.K, 0);
        CHECK(want.size() == sh.K && hc_steps(sh.K) * HC_STEP_K == sh.K, "K %u is whole steps", sh.K);
        for (uint32_t t = 0; t < sh.K; t++) {
            CHECK(hc_term_k(t) == want[t], "K %u term %u: k %u, the MFMA pair's %u", sh.K, t, hc_term_k(t), want[t]);
            if (hc_term_k(t) < sh.K) seen[hc_term_k(t)]++;
        }
        for (uint32_t k = 0; k < sh.K; k++) CHECK(seen[k] == 1, "K %u: k %u visited %d times", sh.K, k, seen[k]);
    }
}

// ---- 3. operand offsets ----
static void check_offsets() {
    for (const Shape& sh : SHAPES) {
        const uint32_t K = sh.K, rows = (sh.J + 31) / 32 * 32;  // w1t: 128 rows; wpt: round32(M) rows
        const size_t alloc = (size_t)rows * K;
        std::vector<int> touched(alloc, 0);
        for (uint32_t unit = 0; unit < hc_strips(sh.J) * HC_UNITS; unit++) {
            const uint32_t row = hc_load_row(unit, sh.J);
            for (uint32_t u = 0; u < hc_steps(K); u++)
                for (uint32_t h = 0; h < 2; h++) {
                    const size_t at = hc_piece_index(row, u, h, K);
                    CHECK(at % 4 == 0 && at + 4 <= alloc, "weights J %u K %u row %u step %u half %u: piece at %zu of %zu", sh.J, K, row, u, h, at, alloc);
                    if (at + 4 > alloc) return;
                    for (uint32_t e = 0; e < 4; e++) {
                        CHECK(at + e == tap_frag_index(row, 8 * u + 4 * h + e, K, 4), "piece element against tap_frag_index");
                        if (unit < sh.J) touched[at + e]++;
                    }
                    // what the kernel's pointer arithmetic assumes
                    CHECK(at == hc_piece_index(row, 0, 0, K) + (size_t)u * HC_STEP_STRIDE + h * HC_HALF_STRIDE, "step / half strides");
                    if ((row & 31) != 31 && row + 1 < rows) CHECK(hc_piece_index(row + 1, u, h, K) == at + 4, "consecutive rows, consecutive 16 bytes");
                }
        }
        for (uint32_t row = 0; row < sh.J; row++)
            for (uint32_t k = 0; k < K; k++) CHECK(touched[tap_frag_index(row, k, K, 4)] == 1, "weights J %u K %u: (%u, %u) read %d times", sh.J, K, row, k, touched[tap_frag_index(row, k, K, 4)]);
    }
    // hv: the value part [hv_leaves][kvp] at 0, the policy part [hv_leaves][kpp] behind it
    const uint32_t kpairs[][2] = {{48, 80}, {784, 784}, {512, 512}, {336, 336}};
    for (uint32_t hv_leaves : {32u, 64u})
        for (const auto& kk : kpairs) {
            const uint32_t kvp = kk[0], kpp = kk[1];
            const size_t total = (size_t)hv_leaves * (kvp + kpp), pol = hc_hv_policy_at(hv_leaves, kvp);
            CHECK(pol == (size_t)hv_leaves * kvp, "policy part behind the value part");
            for (uint32_t n = 1; n <= hv_leaves && n <= 40; n += 13)
                for (uint32_t leaf_raw = 0; leaf_raw < n + 2; leaf_raw++) {
                    const uint32_t leaf = hc_load_leaf(leaf_raw, n);
                    for (uint32_t part = 0; part < 2; part++) {
                        const uint32_t K = part ? kpp : kvp;
                        const size_t base = part ? pol : 0, end = part ? total : pol;
                        for (uint32_t q = 0; q < K / 4; q++) {  // the kernel's staging loop: piece q is step q / 2, half q % 2
                            const size_t at = base + hc_piece_index(leaf, q >> 1, q & 1, K);
                            CHECK(at >= base && at + 4 <= end, "hv_leaves %u K %u leaf %u piece %u at %zu outside [%zu, %zu)", hv_leaves, K, leaf, q, at, base, end);
                            CHECK(at - base == tap_frag_index(leaf, 4 * q, K, 4), "hv piece against tap_frag_index");
                        }
                    }
                }
        }
    // LDS: the activations of nl leaves in plain k order, the hidden units behind them
    CHECK(hc_lds_hidden_at(2, 784, 512) == 2 * 784 && hc_lds_hidden_at(1, 48, 80) == 80, "hidden units behind the longer part");
    CHECK(hc_lds_bytes(2, 784, 784) == (2 * 784 + 2 * 128) * 4, "LDS bytes");
    CHECK(hc_lds_bytes(2, 32 * 121, 32 * 121) <= HC_LDS_MAX, "the largest head the MFMA path takes (32 channels x 121 pixels) fits 64 KiB: %u", hc_lds_bytes(2, 32 * 121, 32 * 121));
}

// ---- 4. the dot product ----
static uint32_t kperm_restated(uint32_t kk) { return (kk & ~7u) + ((kk & 1u) << 2) + ((kk & 7u) >> 1); }
static float plain_dot(const float* a, const float* b, uint32_t K) {
    float acc = 0.0f;
    for (uint32_t kk = 0; kk < K; kk++) {
        const uint32_t k = kperm_restated(kk);
        acc = std::fmaf(a[k], b[k], acc);
    }
    return acc;
}
static std::vector<float> pack(const std::vector<float>& m, uint32_t rows, uint32_t K) {
    std::vector<float> p((size_t)rows * K, 0.0f);
    for (uint32_t r = 0; r < rows; r++)
        for (uint32_t k = 0; k < K; k++) p[tap_frag_index(r, k, K, 4)] = m[(size_t)r * K + k];
    return p;
}
static void check_dot() {
    std::mt19937 rng(20240607);
    std::uniform_real_distribution<float> uni(-2.0f, 2.0f);
    for (const Shape& sh : SHAPES) {
        const uint32_t K = sh.K, live = K == 48 ? 36 : K == 336 ? 324 : K, rows = 64;
        std::vector<float> a((size_t)rows * K, 0.0f), b((size_t)rows * K, 0.0f);
        for (uint32_t r = 0; r < rows; r++)
            for (uint32_t k = 0; k < live; k++) a[(size_t)r * K + k] = uni(rng), b[(size_t)r * K + k] = uni(rng) * std::ldexp(1.0f, (int)(rng() % 40) - 20);
        // row 5: zeros throughout; row 6: the first product makes the partial sum a negative value that underflows to -0, and zero terms
        // (the padded ones among them) follow: fmaf(0, 0, -0.0f) is +0.0f, which the MFMA form computes too
        for (uint32_t k = 0; k < K; k++) a[(size_t)5 * K + k] = 0.0f, a[(size_t)6 * K + k] = 0.0f, b[(size_t)6 * K + k] = 0.0f;
        a[(size_t)6 * K] = -1e-30f, b[(size_t)6 * K] = 1e-30f;
        const std::vector<float> pa = pack(a, rows, K), pb = pack(b, rows, K);
        for (uint32_t ra = 0; ra < rows; ra += 3)
            for (uint32_t rb = 0; rb < rows; rb += 5) {
                const float got = hc_dot(pa.data(), ra, pb.data(), rb, K), want = plain_dot(&a[(size_t)ra * K], &b[(size_t)rb * K], K);
                CHECK(bits(got) == bits(want), "K %u rows (%u, %u): %08x, plain loop %08x", K, ra, rb, bits(got), bits(want));
            }
        const float under = hc_dot(pa.data(), 6, pb.data(), 6, K);
        CHECK(bits(std::fmaf(-1e-30f, 1e-30f, 0.0f)) == 0x80000000u, "the product underflows to -0");
        CHECK(bits(under) == bits(plain_dot(&a[(size_t)6 * K], &b[(size_t)6 * K], K)) && bits(under) == 0u, "K %u: the underflowed chain ends at %08x", K, bits(under));
    }
    // one step, term by term
    const float a0[4] = {1.5f, -2.25f, 3.0f, 0.1f}, a1[4] = {0.7f, 1e-3f, -5.0f, 2.0f}, b0[4] = {0.3f, 0.9f, -1.1f, 7.0f}, b1[4] = {-0.2f, 4.0f, 0.6f, 1e5f};
    float want = 0.25f;
    for (int j = 0; j < 4; j++) want = std::fmaf(a0[j], b0[j], want), want = std::fmaf(a1[j], b1[j], want);
    CHECK(bits(hc_step(0.25f, a0, a1, b0, b1)) == bits(want), "one step");
}

// ---- 5. the epilogues ----
static void check_epilogues() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float accs[] = {0.0f, -0.0f, 1.25f, -3.5f, 1e-40f, -1e-40f, FLT_MAX, -FLT_MAX}, biases[] = {0.0f, 0.5f, -1.25f, FLT_MAX, -FLT_MAX};
    for (float acc : accs)
        for (float bias : biases) {
            const float y = acc + bias;
            CHECK(bits(hc_fc1_epilogue(acc, bias)) == bits(y > 0.0f ? y : 0.0f), "FC1 epilogue of %g + %g", acc, bias);
            const float p = std::isfinite(y) ? y : -FLT_MAX;
            CHECK(bits(hc_policy_epilogue(acc, bias)) == bits(p), "policy epilogue of %g + %g", acc, bias);
        }
    CHECK(bits(hc_policy_epilogue(1.0f, inf)) == bits(-FLT_MAX) && bits(hc_policy_epilogue(1.0f, -inf)) == bits(-FLT_MAX) && bits(hc_policy_epilogue(1.0f, nan)) == bits(-FLT_MAX),
          "the scrub: +inf, -inf, NaN -> -FLT_MAX");
    CHECK(bits(hc_policy_epilogue(inf, 0.0f)) == bits(-FLT_MAX) && bits(hc_policy_epilogue(nan, 0.0f)) == bits(-FLT_MAX), "the scrub on a non-finite sum");
    CHECK(bits(hc_fc1_epilogue(nan, 0.0f)) == 0u, "relu(NaN) is 0, as y > 0 ? y : 0 says");
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
    float w2[HC_HIDDEN], h[HC_HIDDEN];
    for (uint32_t k = 0; k < HC_HIDDEN; k++) w2[k] = uni(rng), h[k] = uni(rng) > 0 ? uni(rng) * 3 : 0.0f;
    float acc = 0.0f;
    for (uint32_t kk = 0; kk < 128; kk++) acc = std::fmaf(w2[kperm_restated(kk)], h[kperm_restated(kk)], acc);
    CHECK(bits(hc_fc2_sum(w2, h, 0.125f)) == bits(acc + 0.125f), "FC2: the 128-term chain, then + b2");
}

int main() {
    check_grid();
    check_walk();
    check_offsets();
    check_dot();
    check_epilogues();
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("head chain rule ok\n");
    return 0;
}
