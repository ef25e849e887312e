// Stand-alone check of cattus_amd/csrc/head_fuse_rule.h (tests/test_head_fuse_rule.py builds it plain and under -fsanitize=address,undefined
// and runs both as programs).  Everything the header states is held against a restatement made here from the kernels it describes:
// head_conv_tile<float>'s walk and epilogue, the resident f16 towers' LDS plan, the MFMA accumulator layout.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "head_fuse_rule.h"

using namespace cattus;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

struct Range {
    int lo, hi;  // [lo, hi)
};
static bool inside(Range a, Range b) { return a.lo >= b.lo && a.hi <= b.hi && a.lo < a.hi; }
static bool disjoint(Range a, Range b) { return a.hi <= b.lo || b.hi <= a.lo; }

// restated: kernels.hip, tower64_lds_bytes
constexpr int SLAB = 3 * 64 * 128;
static int t64_bytes(int ch, bool ls) { return ls ? 6 * SLAB + 2 * 64 * 128 : 3 * SLAB + 2 * ((256 / ch) * 128 + 256); }

// restated: device_common.h, frag_packed_index<float>
static size_t packed_f32(uint32_t row, uint32_t k, uint32_t K) {
    const uint32_t KSTEP = 8, HALF = 4;
    return ((((size_t)(row >> 5) * (K / KSTEP) + k / KSTEP) * 2 + (k % KSTEP) / HALF) * 32 + (row & 31)) * HALF + k % HALF;
}

// 16 lanes of a ds_read_b128 are served together (16 x 16 bytes = the 64 banks once): conflict-free when they touch 64 different banks
template <class At>
static void conflict_free_down_32_rows(At at) {
    for (int u = 0; u < 8; u++)
        for (int h = 0; h < 2; h++)
            for (int r0 = 0; r0 < 32; r0 += 16) {
                std::set<int> banks;
                for (int r = r0; r < r0 + 16; r++) {
                    const int a = at(r, u, h);
                    CHECK(a % 16 == 0);
                    for (int w = 0; w < 4; w++) banks.insert((a / 4 + w) % 64);
                }
                CHECK(banks.size() == 64);
            }
}

static void lds_plans() {
    // ---- the f16 family: (ch, ls) = (2, no), (4, no), (4, yes); BIG changes no byte of the plan ----
    const std::pair<int, bool> shapes[] = {{2, false}, {4, false}, {4, true}};
    for (auto [ch, ls] : shapes) {
        const HfLds L = hf_lds_t64(ch, ls);
        const int total = t64_bytes(ch, ls), rows = 256 / ch;
        const Range w{L.w, L.w + HF_W_BYTES}, b{L.b, L.b + HF_B_BYTES}, x{L.rows, L.rows + L.rows_bytes}, all{0, total};
        CHECK(L.rows_bytes == rows * HF_PITCH);
        CHECK(inside(w, all) && inside(b, all) && inside(x, all));
        CHECK(disjoint(w, b) && disjoint(w, x) && disjoint(b, x));
        CHECK(L.w % 16 == 0 && L.b % 16 == 0 && L.rows % 16 == 0);
        // what the last layer's last step still reads: its weight slab(s) and both activation buffers with their zero areas
        const Range act{(ls ? 6 : 3) * SLAB, total};
        // !ls: step t in slot t % 3, a layer has 3 steps: the last step, 3 nlayers - 1, reads slot 2.  ls: layer l in half l & 1, the last layer 2 blocks is even.
        for (int blocks = 0; blocks <= 6; blocks++) {
            const int nlayers = 1 + 2 * blocks;
            const Range slab = ls ? Range{((nlayers - 1) & 1) * 3 * SLAB, ((nlayers - 1) & 1) * 3 * SLAB + 3 * SLAB} : Range{((3 * nlayers - 1) % 3) * SLAB, ((3 * nlayers - 1) % 3 + 1) * SLAB};
            for (Range r : {w, b, x}) CHECK(disjoint(r, act) && disjoint(r, slab));
        }
        // the staged rows and the weights feed conflict-free fragment reads
        conflict_free_down_32_rows([&](int r, int u, int h) { return L.rows + hf_row_frag(r, u, h); });
        conflict_free_down_32_rows([&](int r, int u, int h) { return L.rows + hf_row_frag(rows - 32 + r, u, h); });
        conflict_free_down_32_rows([&](int r, int u, int h) { return L.w + hf_w_frag(r, u, h); });
        // every (row, channel) has 4 bytes of its own inside the rows; every weight inside the weights
        std::set<int> seen;
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < HF_K; c++) {
                const int a = hf_row_offset(r, c);
                CHECK(a >= 0 && a + 4 <= L.rows_bytes && seen.insert(a).second);
            }
    }
    // ---- the operands' way in: 512 pieces of 16 bytes, each weight once ----
    std::set<int> bytes;
    for (int q = 0; q < 2 * HF_STAGE_THREADS; q++) {
        const int d = hf_piece_dst(q);
        CHECK(d % 16 == 0 && d + 16 <= HF_W_BYTES);
        for (int e = 0; e < 4; e++) {
            const int flat = 4 * q + e;  // the source: [32][64] f32, row-major
            CHECK(d + 4 * e == hf_w_offset(flat / HF_K, flat % HF_K));
            CHECK(bytes.insert(d + 4 * e).second);
        }
    }
    CHECK((int)bytes.size() == HF_CHANNELS * HF_K);
}

static void ownership() {
    for (int ch : {2, 4}) {
        const int rows = 256 / ch;
        std::set<std::pair<int, int>> seen;
        int waves_with_tile = 0;
        for (int wave = 0; wave < 8; wave++) {
            const int tile = hf_tile_of_wave(ch, wave);
            if (tile < 0) continue;
            CHECK(wave < 4 && tile < hf_tiles(ch));
            waves_with_tile++;
            for (int lane = 0; lane < 64; lane++)
                for (int e = 0; e < 16; e++) {
                    const HfOwn o = hf_own(ch, wave, lane, e);
                    // restated: the accumulator of v_mfma_f32_32x32x2_f32 -- column lane % 32 (operand B's row: the tower row), row (e % 4) + 8 (e / 4) + 4 (lane / 32)
                    CHECK(o.row == tile * 32 + lane % 32 && o.channel == e % 4 + 8 * (e / 4) + 4 * (lane / 32));
                    CHECK(o.row >= 0 && o.row < rows && o.channel >= 0 && o.channel < HF_CHANNELS);
                    CHECK(seen.insert({o.row, o.channel}).second);
                }
        }
        CHECK(waves_with_tile == hf_tiles(ch) && (int)seen.size() == rows * HF_CHANNELS);
        // the tile is one of the wave's own pixel blocks in the tower's map (t64r_own): ch = 2, block wave & 1 of the wave's row block; ch = 4, the
        // wave's one block -- a wave reads back rows it, or the wave beside it, has just written
        for (int wave = 0; wave < 4; wave++)
            if (hf_tile_of_wave(ch, wave) >= 0) CHECK(hf_own(ch, wave, 0, 0).row == t64r_own(ch, wave, 0, 0, ch == 2 ? wave & 1 : 0, 0).row);
    }
}

static void chain_order() {
    // restated from head_conv_tile<float> with K = 64: one chunk, stages u = 0..7 ascending; a stage is Mfma<float>::mac = four
    // v_mfma_f32_32x32x2_f32, the j-th on element j of both fragments; one such MFMA adds the products of lane half 0, then of lane half 1;
    // a fragment of stage u in lane half h holds k = 8 u + 4 h + j in element j
    std::vector<uint32_t> walk;
    for (uint32_t u = 0; u < 8; u++)
        for (uint32_t j = 0; j < 4; j++)
            for (uint32_t h = 0; h < 2; h++) walk.push_back(8 * u + 4 * h + j);
    CHECK(walk.size() == (size_t)HF_K);
    std::set<uint32_t> ks;
    for (uint32_t t = 0; t < (uint32_t)HF_K; t++) {
        CHECK(hf_term_k(t) == walk[t]);
        // kperm, restated from kernels.hip
        CHECK(hf_term_k(t) == (t & ~7u) + ((t & 1u) << 2) + ((t & 7u) >> 1));
        ks.insert(hf_term_k(t));
        // where the term's operands are read: stage t >> 3, lane half t & 1, element (t & 7) >> 1
        const int u = t >> 3, h = t & 1, j = (t & 7) >> 1;
        CHECK(hf_w_frag(5, u, h) + 4 * j == hf_w_offset(5, (int)hf_term_k(t)));
        CHECK(hf_row_frag(77, u, h) + 4 * j == hf_row_offset(77, (int)hf_term_k(t)));
    }
    CHECK(ks.size() == (size_t)HF_K);
}

static uint32_t round16(uint32_t x) { return (x + 15) / 16 * 16; }

static void hv_index() {
    struct Shape {
        const char* name;
        uint32_t S, slots, vhc, phc;
    };
    const Shape shapes[] = {{"ttt", 3, 64, 4, 8}, {"hex7", 7, 64, 16, 16}, {"hex9", 9, 128, 4, 4}, {"chess", 8, 64, 8, 8}};
    const uint32_t hv_leaves = 64;  // max_batch 40, padded boards 40, rounded up to 32s
    for (const Shape& s : shapes) {
        const uint32_t hw = s.S * s.S, kvp = round16(s.vhc * hw), kpp = round16(s.phc * hw);
        const HfHead H{hw, s.vhc, s.vhc + s.phc, kvp, kpp, hv_leaves * kvp, s.slots};
        for (uint32_t n : {1u, 3u, 40u}) {
            std::set<size_t> written;
            const uint32_t padded_rows = (n * s.slots + 255) / 256 * 256;
            for (uint32_t grow = 0; grow < padded_rows; grow++)
                for (uint32_t i = 0; i < 32; i++) {
                    // restated from head_conv_tile's epilogue: J = n * slots rows, I = 32
                    const uint32_t J = n * s.slots, bb = grow / s.slots, p = grow % s.slots;
                    const bool want = grow < J && i < H.ocn && p < hw;
                    CHECK(hf_writes(H, n, grow, i) == want);
                    if (!want) continue;
                    const size_t at = i < s.vhc ? packed_f32(bb, i * hw + p, kvp) : H.hv_pol + packed_f32(bb, (i - s.vhc) * hw + p, kpp);
                    CHECK(hf_hv_index(H, grow, i) == at);
                    CHECK(at < (size_t)hv_leaves * (kvp + kpp) && written.insert(at).second);
                }
            CHECK(written.size() == (size_t)n * hw * H.ocn);
        }
    }
    for (uint32_t row = 0; row < 70; row++)
        for (uint32_t k = 0; k < 800; k++) CHECK(hf_packed_f32(row, k, 800) == packed_f32(row, k, 800));
}

static void predicate() {
    int taken = 0;
    for (HfPlan p : {HfPlan::Other, HfPlan::Resident64Bf16, HfPlan::Resident64F16, HfPlan::Resident64Split, HfPlan::Resident64Stream, HfPlan::Resident64F32}) {
        const bool want = p == HfPlan::Resident64F16 || p == HfPlan::Resident64Stream;  // the resident f32 tower keeps its head conv launch
        CHECK(hf_takes(p) == want);
        taken += hf_takes(p);
    }
    CHECK(taken == 2);
}

int main() {
    lds_plans();
    ownership();
    chain_order();
    hv_index();
    predicate();
    std::printf("head fuse rule ok\n");
    return 0;
}
