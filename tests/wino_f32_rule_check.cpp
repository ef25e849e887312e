// Stand-alone program around cattus_amd/csrc/wino_f32_rule.h (tests/test_wino_f32_rule.py builds it plain and under sanitizers): the grid
// map, the transform's items, every LDS offset of conv3x3_wino_f32_kernel, the bank slots of its accesses, the U index against the
// builder (weight_layout.h: wino_u_f32), the chain's channel order and the transforms' operation order against the matrices in float64.
// Prints what fails and "wino_f32 rule ok" when nothing does.
#include <math.h>
#include <stdio.h>

#include <random>
#include <set>
#include <utility>
#include <vector>

#include "weight_layout.h"
#include "wino_f32_rule.h"

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

// what occupies a byte of LDS during the loop / during the epilogue
static void claim(std::vector<int>& owner, int at, int len, int who, int lo, int hi, const char* what) {
    CHECK(at >= lo && at + len <= hi, "%s: [%d, %d) outside [%d, %d)", what, at, at + len, lo, hi);
    if (at < 0 || at + len > (int)owner.size()) return;
    for (int b = at; b < at + len; b++) {
        CHECK(owner[b] == -1 || owner[b] == who, "%s: byte %d claimed twice (%d, %d)", what, b, owner[b], who);
        owner[b] = who;
    }
}

// MI355X: a ds_read_b128 / ds_write_b128 is served in four groups of 16 lanes; a group is conflict-free when its lanes fall on 16
// different 16-byte slots of the 256-byte bank row
static const int GROUPS[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
template <class F>
static void check_b128(F&& address, const char* what) {
    for (int half = 0; half < 2; half++)
        for (int g = 0; g < 2; g++) {
            std::set<int> slots;
            for (int k = 0; k < 16; k++) {
                const int a = address(GROUPS[g][k] + 32 * half);
                CHECK(a % 16 == 0, "%s: address %d is not 16-byte aligned", what, a);
                slots.insert((a / 16) % 16);
            }
            CHECK(slots.size() == 16, "%s: lane group %d of half %d on %zu bank slots", what, g, half, slots.size());
        }
}
// an 8-byte access of a 32-lane half wave: conflict-free when its lanes fall on 32 different 8-byte pairs of the 64 banks
template <class F>
static void check_b64(F&& address, const char* what) {
    for (int h = 0; h < WF32_THREADS / 32; h++) {
        std::set<int> pairs;
        for (int l = 0; l < 32; l++) {
            const int a = address(h * 32 + l);
            CHECK(a % 8 == 0, "%s: address %d is not 8-byte aligned", what, a);
            pairs.insert((a / 8) % 32);
        }
        CHECK(pairs.size() == 32, "%s: half wave %d on %zu bank pairs", what, h, pairs.size());
    }
}

int main() {
    // ---- the grid: a bijection onto (board pair, cout group), for one and for two cout blocks per workgroup, on grids that are and are
    // not multiples of 8; with the XCD map the cout groups of a pair share index % 8 wherever an XCD's share is whole pairs ----
    const int filters[] = {128, 192, 256, 384}, bpads[] = {2, 4, 8, 12, 20, 80, 256};
    for (int cout : filters)
        for (int bpad : bpads)
            for (int ncb = 1; ncb <= 2; ncb++) {
                const int ng = cout / (32 * ncb), nblk = (int)wf32_grid((uint32_t)bpad, (uint32_t)cout, ncb);
                CHECK(nblk == bpad / 2 * ng, "grid %d", nblk);
                std::set<std::pair<int, int>> seen;
                std::vector<int> xcd(bpad / 2, -1);
                for (int wg = 0; wg < nblk; wg++) {
                    const int logical = wf32_logical(wg, nblk);
                    const int pair = wf32_pair(logical, ng), cg = wf32_cout_group(logical, ng);
                    CHECK(logical >= 0 && logical < nblk && pair >= 0 && pair < bpad / 2 && cg >= 0 && cg < ng, "wg %d of %d -> (%d, %d)", wg, nblk, pair, cg);
                    seen.insert({pair, cg});
                    if (pair < 0 || pair >= bpad / 2) continue;
                    if (nblk % 8 == 0 && (nblk / 8) % ng == 0) {  // an XCD's range of logical indices holds whole pairs
                        CHECK(xcd[pair] == -1 || xcd[pair] == wg % 8, "filters %d bpad %d: pair %d on XCDs %d and %d", cout, bpad, pair, xcd[pair], wg % 8);
                        xcd[pair] = wg % 8;
                    }
                }
                CHECK((int)seen.size() == nblk, "filters %d bpad %d ncb %d: %zu distinct tiles of %d", cout, bpad, ncb, seen.size(), nblk);
            }
    // the cout blocks per workgroup: two exactly when that grid has a workgroup for each of the 256 CUs
    CHECK(wf32_ncb(256, 256) == 2 && wf32_ncb(128, 256) == 2 && wf32_ncb(64, 256) == 1 && wf32_ncb(124, 256) == 1, "ncb on 256 filters");
    CHECK(wf32_ncb(256, 128) == 2 && wf32_ncb(252, 128) == 1 && wf32_ncb(80, 192) == 1 && wf32_ncb(172, 192) == 2 && wf32_ncb(168, 192) == 1, "ncb thresholds");
    for (int cout : filters)
        for (int bpad = 2; bpad <= 512; bpad += 2) {
            const int ncb = wf32_ncb((uint32_t)bpad, (uint32_t)cout);
            CHECK(ncb == ((int)wf32_grid((uint32_t)bpad, (uint32_t)cout, 2) >= WF32_CUS ? 2 : 1), "ncb(%d, %d) = %d", bpad, cout, ncb);
        }

    // ---- the transform's items cover every (tile, channel pair) of a step exactly once, so every (tile, channel) of its 16 ----
    {
        std::set<std::pair<int, int>> seen, channels;
        for (int tid = 0; tid < WF32_THREADS; tid++) {
            const int tt = wf32_item_tile(tid), chp = wf32_item_chp(tid);
            CHECK(tt >= 0 && tt < WF32_TILES && chp >= 0 && chp < 8, "item of thread %d: (%d, %d)", tid, tt, chp);
            seen.insert({tt, chp});
            for (int e = 0; e < 2; e++) channels.insert({tt, chp * 2 + e});
        }
        CHECK(seen.size() == 256, "%zu distinct items", seen.size());
        CHECK(channels.size() == 32 * WF32_STEP, "%zu distinct (tile, channel)", channels.size());
    }

    CHECK(WF32_LDS_TOTAL <= 160 * 1024, "LDS total %d", WF32_LDS_TOTAL);
    CHECK(wf32_chunk_buffer(1) + WF32_DBUF == WF32_LDS_TOTAL && wf32_v_image(2) == wf32_chunk_buffer(0), "areas do not tile LDS");

    // ---- the loop's LDS: V images and chunk buffers, writes inside their areas and on bytes of their own ----
    std::vector<int> owner(WF32_LDS_TOTAL, -1);
    for (int img = 0; img < 2; img++) {
        const int lo = wf32_v_image(img), hi = lo + WF32_VIMG;
        for (int tid = 0; tid < WF32_THREADS; tid++)
            for (int f = 0; f < 16; f++)
                claim(owner, lo + wf32_v_write(f, wf32_item_tile(tid), wf32_item_chp(tid)), 8, 1000000 + (img * 256 + tid) * 16 + f, lo, hi, "V write");
        // every byte a fragment read takes was written by somebody
        for (int f = 0; f < 16; f++)
            for (int lane = 0; lane < 64; lane++)
                for (int g = 0; g < 2; g++) {
                    const int a = lo + wf32_v_read(f, lane, g);
                    CHECK(a >= lo && a + 16 <= hi, "V read at %d", a);
                    for (int b = a; b < a + 16 && b < hi && b >= lo; b++) CHECK(owner[b] >= 1000000, "V read of byte %d nobody wrote", b);
                }
    }
    // a fragment is what the items wrote: tile r's channels 8 g + 4 h .. + 3 = channel pairs 4 g + 2 h, + 1; element j of the fragment is
    // k = 4 h + j of the group, the operand Mfma<float>::mac's MFMA j takes; the kernel adds the frequency and the group as constants
    for (int f = 0; f < 16; f++)
        for (int lane = 0; lane < 64; lane++)
            for (int g = 0; g < 2; g++) {
                for (int c = 0; c < 2; c++)
                    CHECK(wf32_v_read(f, lane, g) + 8 * c == wf32_v_write(f, lane & 31, 4 * g + 2 * (lane >> 5) + c), "fragment (%d, %d, %d)", f, lane, g);
                CHECK(wf32_v_read(f, lane, g) == wf32_v_read(0, lane, 0) + f * WF32_VF + g * WF32_VGROUP, "V read constants (%d, %d, %d)", f, lane, g);
                CHECK(wf32_v_write(f, lane & 31, lane >> 3) == wf32_v_write(0, lane & 31, lane >> 3) + f * WF32_VF, "V write constants");
            }
    for (int buf = 0; buf < 2; buf++) {
        const int lo = wf32_chunk_buffer(buf), hi = lo + WF32_DBUF;
        std::set<int> rows;
        for (int tid = 0; tid < WF32_THREADS; tid++)
            for (int i = 0; i < 4; i++) {
                const int row = wf32_piece_row(tid, i);
                CHECK(row >= 0 && row < WF32_ROWS, "piece row %d", row);
                rows.insert(row * 8 + (tid & 7));
                claim(owner, lo + wf32_piece_dst(tid, i), 16, 2000000 + (buf * 256 + tid) * 4 + i, lo, lo + WF32_DZERO, "chunk piece");
                CHECK(wf32_piece_dst(tid, i) == wf32_pixel_offset(row) + (tid & 7) * 16, "piece (%d, %d)", tid, i);
            }
        CHECK(rows.size() == 1024, "%zu distinct pieces of a chunk", rows.size());
        claim(owner, lo + WF32_DZERO, WF32_ZAREA, 3000000 + buf, lo, hi, "zero area");
        // patch reads: on the board the pixel's own bytes, off the board the zero area at the same address mod 256
        for (int tile = 0; tile < WF32_TILES; tile++)
            for (int chp = 0; chp < 8; chp++)
                for (int i = 0; i < 4; i++)
                    for (int j = 0; j < 4; j++)
                        for (int half = 0; half < 2; half++) {
                            const int a = wf32_patch_read(tile, chp, i, j, half);
                            const int y = 2 * ((tile >> 2) & 3) - 1 + i, x = 2 * (tile & 3) - 1 + j;
                            const bool on = y >= 0 && y < 8 && x >= 0 && x < 8;
                            CHECK(a % 8 == 0 && a >= 0 && a + 8 <= WF32_DBUF, "patch read at %d", a);
                            // channels 16 half + 2 chp, + 1 of the chunk's 32
                            if (on) CHECK(a == wf32_pixel_offset((tile >> 4) * 64 + y * 8 + x) + (16 * half + 2 * chp) * 4, "patch (%d, %d, %d, %d)", tile, chp, i, j);
                            else CHECK(a >= WF32_DZERO && a + 8 <= WF32_DZERO + WF32_ZAREA, "off-board read at %d", a);
                            CHECK(a == wf32_patch_read(tile, chp, i, j, 0) + half * WF32_DHALF, "the half is an added constant");
                            for (int b = lo + a; on && b < lo + a + 8; b++) CHECK(owner[b] >= 2000000 && owner[b] < 3000000, "patch read of byte %d no piece wrote", b);
                        }
    }
    // the overlap the header does state: the exchange lies over V image 0, and over nothing else
    CHECK(WF32_LDS_Z <= WF32_VIMG && wf32_v_image(0) == 0, "the exchange leaves V image 0");

    // ---- the exchange: inside its area, every 16 bytes written once, every read of a written slot ----
    {
        std::vector<int> z(WF32_LDS_Z, -1);
        for (int q = 0; q < 4; q++)
            for (int c = 0; c < 2; c++)
                for (int lane = 0; lane < 64; lane++)
                    for (int g = 0; g < 4; g++) claim(z, wf32_z(q, c, lane & 31, g * 2 + (lane >> 5)), 16, ((q * 2 + c) * 64 + lane) * 4 + g, 0, WF32_LDS_Z, "Z write");
        for (int b = 0; b < WF32_LDS_Z; b++) CHECK(z[b] >= 0, "exchange byte %d is never written", b);
        // the output rows: every (row of the 128, unit) once; the tile a pixel reads is the tile that computed it
        std::set<int> outs;
        for (int r = 0; r < 4; r++)
            for (int lane = 0; lane < 64; lane++)
                for (int k = 0; k < 4; k++) {
                    const int p = wf32_out_pixel(lane, k), row = wf32_out_row(r, p), tile = wf32_out_tile(r, p);
                    CHECK(p >= 0 && p < 32 && row >= 0 && row < WF32_ROWS && tile >= 0 && tile < WF32_TILES, "output (%d, %d, %d)", r, lane, k);
                    outs.insert(row * 8 + (lane & 7));
                    const int board = row >> 6, y = (row >> 3) & 7, x = row & 7;
                    CHECK(tile == board * 16 + (y >> 1) * 4 + (x >> 1) && (y >> 1) == r && (y & 1) == (k & 1) && (x & 1) == (p & 1), "pixel %d of wave %d", row, r);
                    for (int i = 0; i < 3; i++) {
                        const int a = wf32_z((k & 1) + i, p & 1, tile, lane & 7);
                        CHECK(a >= 0 && a + 16 <= WF32_LDS_Z && a % 16 == 0, "Z read at %d", a);
                    }
                }
        CHECK(outs.size() == 1024, "%zu distinct output pieces", outs.size());
    }

    // ---- bank slots: the 16-byte V reads and exchange accesses, the 8-byte V writes and patch reads of a half wave ----
    for (int f = 0; f < 16; f++)
        for (int g = 0; g < 2; g++)
            for (int img = 0; img < 2; img++) check_b128([&](int lane) { return wf32_v_image(img) + wf32_v_read(f, lane, g); }, "V fragment read");
    for (int q = 0; q < 4; q++)
        for (int c = 0; c < 2; c++)
            for (int g = 0; g < 4; g++) check_b128([&](int lane) { return wf32_z(q, c, lane & 31, g * 2 + (lane >> 5)); }, "Z write");
    for (int r = 0; r < 4; r++)
        for (int k = 0; k < 4; k++)
            for (int i = 0; i < 3; i++)
                check_b128([&](int lane) {
                    const int p = wf32_out_pixel(lane, k);
                    return wf32_z((k & 1) + i, p & 1, wf32_out_tile(r, p), lane & 7);
                }, "Z read");
    for (int f = 0; f < 16; f++)
        for (int img = 0; img < 2; img++)
            check_b64([&](int tid) { return wf32_v_image(img) + wf32_v_write(f, wf32_item_tile(tid), wf32_item_chp(tid)); }, "V write");
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            for (int half = 0; half < 2; half++)
                for (int buf = 0; buf < 2; buf++)
                    check_b64([&](int tid) { return wf32_chunk_buffer(buf) + wf32_patch_read(wf32_item_tile(tid), wf32_item_chp(tid), i, j, half); }, "patch read");

    // ---- the chain: every channel once, chunks and groups ascending, in a group Mfma<float>::mac's pairs (i, 4 + i) ----
    {
        std::set<int> seen;
        for (int n = 0; n < 256; n++) {
            const int c = wf32_chain_channel(n);
            seen.insert(c);
            CHECK(c / 8 == n / 8, "fmaf %d multiplies channel %d of another group", n, c);
            CHECK((c & 7) == ((n & 7) >> 1) + 4 * (n & 1), "fmaf %d multiplies channel %d", n, c);
        }
        CHECK(seen.size() == 256, "%zu distinct channels in the chain", seen.size());
        const int first[8] = {0, 4, 1, 5, 2, 6, 3, 7};
        for (int n = 0; n < 8; n++) CHECK(wf32_chain_channel(n) == first[n] && wf32_chain_channel(8 + n) == 8 + first[n], "chain position %d", n);
    }

    // ---- U: the index is a bijection onto the buffer, a stage is 1 KiB of it in the MFMA's A-fragment order, and the builder puts
    // f32(U) there ----
    {
        const uint32_t shapes[][2] = {{128, 128}, {192, 192}, {64, 128}};  // (cout_pad, cin_pad)
        for (auto& sh : shapes) {
            const uint32_t CO = sh[0], CI = sh[1];
            const size_t n = wino_f32_u_elems(CO, CI);
            std::vector<char> hit(n, 0);
            for (uint32_t f = 0; f < 16; f++)
                for (uint32_t co = 0; co < CO; co++)
                    for (uint32_t ci = 0; ci < CI; ci++) {
                        const size_t at = wino_f32_frag_index(f, co, ci, CI);
                        CHECK(at < n, "U index %zu of %zu", at, n);
                        if (at >= n) continue;
                        CHECK(!hit[at], "U index %zu twice", at);
                        hit[at] = 1;
                        // the kernel's address: the stage of (group ci / 8, f) of cout block co / 32, lane (ci / 4 & 1) * 32 + co % 32, element ci % 4
                        const size_t byte = wf32_u_stage((int)(co >> 5), (int)(CI / 8), (int)(ci >> 3), (int)f) + (((ci >> 2) & 1) * 32 + (co & 31)) * 16 + (ci & 3) * 4;
                        CHECK(byte == at * 4, "U stage offset (%u, %u, %u): %zu != %zu", f, co, ci, byte, at * 4);
                    }
            size_t total = 0;
            for (char h : hit) total += h;
            CHECK(total == n, "U: %zu of %zu elements", total, n);
            CHECK(wf32_u_stage((int)(CO / 32) - 1, (int)(CI / 8), (int)(CI / 8) - 1, 15) + WF32_STAGE == n * 4, "the last stage ends the buffer");
        }
        // the builder against the index, on a layer with padding (cout 100 of 128, cin 120 of 128)
        std::mt19937 rng(5);
        std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
        const ConvShape s{100, 120, 128, 128};
        Folded f;
        f.w.resize((size_t)9 * s.cout * s.cin);
        f.b.assign(s.cout, 0.25f);
        for (float& w : f.w) w = uni(rng);
        std::vector<int> shift;
        const std::vector<double> U = wino_transform(f, s, &shift);
        const std::vector<float> wu = wino_u_f32(U, s);
        CHECK(wu.size() == wino_f32_u_elems(s.cout_pad, s.cin_pad), "wino_u_f32: %zu elements", wu.size());
        size_t wrong = 0, nonzero_pad = 0;
        for (uint32_t co = 0; co < s.cout_pad; co++)
            for (uint32_t ci = 0; ci < s.cin_pad; ci++)
                for (uint32_t q = 0; q < 16; q++) {
                    const float got = wu[wino_f32_frag_index(q, co, ci, s.cin_pad)];
                    if (co >= s.cout || ci >= s.cin) {
                        nonzero_pad += got != 0.0f;
                        continue;
                    }
                    wrong += !(got == (float)U[((size_t)co * s.cin + ci) * 16 + q]);
                }
        CHECK(wrong == 0 && nonzero_pad == 0, "wino_u_f32: %zu wrong values, %zu nonzero padding", wrong, nonzero_pad);
        // wino_transform is G g G^T in wf32_g's order
        size_t gwrong = 0;
        for (uint32_t co = 0; co < s.cout; co += 7)
            for (uint32_t ci = 0; ci < s.cin; ci += 5) {
                double t[4][3], u[4][4];
                for (int kx = 0; kx < 3; kx++) {
                    const double g0 = f.w[((size_t)(0 * 3 + kx) * s.cout + co) * s.cin + ci], g1 = f.w[((size_t)(1 * 3 + kx) * s.cout + co) * s.cin + ci],
                                 g2 = f.w[((size_t)(2 * 3 + kx) * s.cout + co) * s.cin + ci];
                    wf32_g(g0, g1, g2, t[0][kx], t[1][kx], t[2][kx], t[3][kx]);
                }
                for (int i = 0; i < 4; i++) wf32_g(t[i][0], t[i][1], t[i][2], u[i][0], u[i][1], u[i][2], u[i][3]);
                for (int q = 0; q < 16; q++) gwrong += !(U[((size_t)co * s.cin + ci) * 16 + q] == u[q >> 2][q & 3]);
            }
        CHECK(gwrong == 0, "wino_transform against wf32_g: %zu", gwrong);
    }

    // ---- the transforms' operation orders reproduce the matrices: B^T d B, G g G^T and A^T m A against float64 matrix products, and
    // together the 3x3 correlation ----
    {
        static const double BT[4][4] = {{1, 0, -1, 0}, {0, 1, 1, 0}, {0, -1, 1, 0}, {0, 1, 0, -1}};
        static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
        static const double AT[2][4] = {{1, 1, 1, 0}, {0, 1, -1, -1}};
        std::mt19937 rng(11);
        std::uniform_real_distribution<double> uni(-1.0, 1.0);
        double worst_v = 0.0, worst_u = 0.0, worst_y = 0.0, worst_conv = 0.0, worst_f32 = 0.0;
        for (int trial = 0; trial < 200; trial++) {
            double d[4][4], g[3][3];
            for (auto& r : d)
                for (double& x : r) x = uni(rng);
            for (auto& r : g)
                for (double& x : r) x = uni(rng);
            // the header's order: columns first, then rows (the kernel's two passes)
            double t[4][4], v[4][4];
            for (int j = 0; j < 4; j++) wf32_bt(d[0][j], d[1][j], d[2][j], d[3][j], t[0][j], t[1][j], t[2][j], t[3][j]);
            for (int i = 0; i < 4; i++) wf32_bt(t[i][0], t[i][1], t[i][2], t[i][3], v[i][0], v[i][1], v[i][2], v[i][3]);
            float df[4][4], tf[4][4], vf[4][4];  // the same in f32, as the kernel runs it
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 4; j++) df[i][j] = (float)d[i][j];
            for (int j = 0; j < 4; j++) wf32_bt(df[0][j], df[1][j], df[2][j], df[3][j], tf[0][j], tf[1][j], tf[2][j], tf[3][j]);
            for (int i = 0; i < 4; i++) wf32_bt(tf[i][0], tf[i][1], tf[i][2], tf[i][3], vf[i][0], vf[i][1], vf[i][2], vf[i][3]);
            double tg[4][3], u[4][4];
            for (int kx = 0; kx < 3; kx++) wf32_g(g[0][kx], g[1][kx], g[2][kx], tg[0][kx], tg[1][kx], tg[2][kx], tg[3][kx]);
            for (int i = 0; i < 4; i++) wf32_g(tg[i][0], tg[i][1], tg[i][2], u[i][0], u[i][1], u[i][2], u[i][3]);
            for (int i = 0; i < 4; i++)
                for (int l = 0; l < 4; l++) {
                    double vm = 0.0, um = 0.0, vd = 0.0;
                    for (int a = 0; a < 4; a++)
                        for (int b = 0; b < 4; b++) vm += BT[i][a] * d[a][b] * BT[l][b], vd += BT[i][a] * (double)df[a][b] * BT[l][b];
                    for (int a = 0; a < 3; a++)
                        for (int b = 0; b < 3; b++) um += G[i][a] * g[a][b] * G[l][b];
                    worst_v = std::max(worst_v, fabs(vm - v[i][l]));
                    worst_u = std::max(worst_u, fabs(um - u[i][l]));
                    worst_f32 = std::max(worst_f32, fabs(vd - (double)vf[i][l]));
                }
            // M = U . V elementwise; Z = M A along the rows (the waves' pass), Y = A^T Z down them (the finishing pass)
            double m[4][4], z[4][2], y[2][2];
            for (int i = 0; i < 4; i++)
                for (int l = 0; l < 4; l++) m[i][l] = u[i][l] * v[i][l];
            for (int i = 0; i < 4; i++) wf32_at(m[i][0], m[i][1], m[i][2], m[i][3], z[i][0], z[i][1]);
            for (int c = 0; c < 2; c++) wf32_at(z[0][c], z[1][c], z[2][c], z[3][c], y[0][c], y[1][c]);
            for (int r = 0; r < 2; r++)
                for (int c = 0; c < 2; c++) {
                    double ym = 0.0, conv = 0.0;
                    for (int a = 0; a < 4; a++)
                        for (int b = 0; b < 4; b++) ym += AT[r][a] * m[a][b] * AT[c][b];
                    for (int ky = 0; ky < 3; ky++)
                        for (int kx = 0; kx < 3; kx++) conv += g[ky][kx] * d[r + ky][c + kx];
                    worst_y = std::max(worst_y, fabs(ym - y[r][c]));
                    worst_conv = std::max(worst_conv, fabs(conv - y[r][c]));
                }
        }
        // float64 sums of at most 16 terms of size <= 1: a few 1e-16 each
        CHECK(worst_v < 1e-14 && worst_u < 1e-14 && worst_y < 1e-14 && worst_conv < 1e-13, "transforms: V %g, U %g, Y %g, conv %g", worst_v, worst_u, worst_y, worst_conv);
        // in f32: three roundings of values <= 4, each <= 2^-22
        CHECK(worst_f32 < 4 * 2.4e-7, "the f32 transform is %g off", worst_f32);
    }

    // ---- the epilogue's last step: + bias, + skip, ReLU with -0 and NaN to +0 ----
    CHECK(wf32_finish(1.0f, 0.5f, false, 9.0f) == 1.5f && wf32_finish(1.0f, 0.5f, true, -2.0f) == 0.0f && wf32_finish(1.0f, 0.5f, true, 2.0f) == 3.5f, "finish");
    CHECK(!signbit(wf32_finish(-0.0f, -0.0f, false, 0.0f)) && wf32_finish(NAN, 0.0f, false, 0.0f) == 0.0f && isinf(wf32_finish(INFINITY, 0.0f, false, 0.0f)), "finish: -0, NaN, inf");

    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("wino_f32 rule ok\n");
    return 0;
}
