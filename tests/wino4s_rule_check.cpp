// Stand-alone program around cattus_amd/csrc/wino4s_rule.h (tests/test_wino4s_rule.py builds it plain and under sanitizers): the grid map,
// the transform's items, every LDS offset of conv3x3_wino4s_kernel and the bank slots of its 16-byte accesses.  Prints what fails and
// "wino4s rule ok" when nothing does.
#include <stdio.h>

#include <set>
#include <utility>
#include <vector>

#include "wino4s_rule.h"

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

int main() {
    // ---- the grid: a bijection onto (board pair, cout block); with the XCD map the cout blocks of a pair share index % 8 ----
    const int filters[] = {128, 192, 256, 384}, bpads[] = {4, 8, 20, 256};
    for (int cout : filters)
        for (int bpad : bpads) {
            const int ncb = cout / W4S_COUTS, nblk = (int)wino4s_grid((uint32_t)bpad, (uint32_t)cout);
            CHECK(nblk == bpad / 2 * ncb, "grid %d", nblk);
            std::set<std::pair<int, int>> seen;
            std::vector<int> xcd(bpad / 2, -1);
            for (int wg = 0; wg < nblk; wg++) {
                const int logical = wino4s_logical(wg, nblk);
                const int pair = wino4s_pair(logical, ncb), cb = wino4s_cout_block(logical, ncb);
                CHECK(logical >= 0 && logical < nblk && pair >= 0 && pair < bpad / 2 && cb >= 0 && cb < ncb, "wg %d of %d -> (%d, %d)", wg, nblk, pair, cb);
                seen.insert({pair, cb});
                if (pair < 0 || pair >= bpad / 2) continue;
                if (nblk % 8 == 0 && (nblk / 8) % ncb == 0) {  // an XCD's range of logical indices holds whole pairs
                    CHECK(xcd[pair] == -1 || xcd[pair] == wg % 8, "filters %d bpad %d: pair %d on XCDs %d and %d", cout, bpad, pair, xcd[pair], wg % 8);
                    xcd[pair] = wg % 8;
                }
            }
            CHECK((int)seen.size() == nblk, "filters %d bpad %d: %zu distinct tiles of %d", cout, bpad, seen.size(), nblk);
        }

    // ---- the transform's items cover (tile, channel pair) once ----
    {
        std::set<std::pair<int, int>> seen;
        for (int tid = 0; tid < W4S_THREADS; tid++) {
            const int tt = wino4s_item_tile(tid), chp = wino4s_item_chp(tid);
            CHECK(tt >= 0 && tt < W4S_TILES && chp >= 0 && chp < 8, "item of thread %d: (%d, %d)", tid, tt, chp);
            seen.insert({tt, chp});
        }
        CHECK(seen.size() == 256, "%zu distinct items", seen.size());
    }

    CHECK(W4S_LDS_TOTAL <= 160 * 1024, "LDS total %d", W4S_LDS_TOTAL);
    CHECK(wino4s_chunk_buffer(1) + W4S_DBUF == W4S_LDS_TOTAL && wino4s_v_image(2) == wino4s_chunk_buffer(0), "areas do not tile LDS");

    // ---- the loop's LDS: V images and chunk buffers, writes inside their areas and on bytes of their own ----
    std::vector<int> owner(W4S_LDS_TOTAL, -1);
    for (int img = 0; img < 2; img++) {
        const int lo = wino4s_v_image(img), hi = lo + W4S_VIMG;
        for (int tid = 0; tid < W4S_THREADS; tid++)
            for (int f = 0; f < 16; f++)
                for (int part = 0; part < 2; part++)
                    claim(owner, lo + wino4s_v_write(f, wino4s_item_tile(tid), wino4s_item_chp(tid), part), 4, 1000000 + ((img * 256 + tid) * 16 + f) * 2 + part, lo, hi, "V write");
        // every byte a fragment read takes was written by somebody
        for (int f = 0; f < 16; f++)
            for (int lane = 0; lane < 64; lane++)
                for (int part = 0; part < 2; part++) {
                    const int a = lo + wino4s_v_read(f, lane, part);
                    CHECK(a >= lo && a + 16 <= hi, "V read at %d", a);
                    for (int b = a; b < a + 16 && b < hi && b >= lo; b++) CHECK(owner[b] >= 1000000, "V read of byte %d nobody wrote", b);
                }
    }
    // a fragment is what the items wrote: tile r's channels 8 h .. 8 h + 7 = channel pairs 4 h .. 4 h + 3
    for (int f = 0; f < 16; f += 5)
        for (int lane = 0; lane < 64; lane++)
            for (int part = 0; part < 2; part++)
                for (int c = 0; c < 4; c++)
                    CHECK(wino4s_v_read(f, lane, part) + 4 * c == wino4s_v_write(f, lane & 31, 4 * (lane >> 5) + c, part), "fragment (%d, %d, %d)", f, lane, part);
    for (int buf = 0; buf < 2; buf++) {
        const int lo = wino4s_chunk_buffer(buf), hi = lo + W4S_DBUF;
        std::set<int> rows;
        for (int tid = 0; tid < W4S_THREADS; tid++)
            for (int i = 0; i < 4; i++) {
                const int row = wino4s_piece_row(tid, i);
                CHECK(row >= 0 && row < W4S_ROWS, "piece row %d", row);
                rows.insert(row * 8 + (tid & 7));
                claim(owner, lo + wino4s_piece_dst(tid, i), 16, 2000000 + (buf * 256 + tid) * 4 + i, lo, lo + W4S_DZERO, "chunk piece");
                CHECK(wino4s_piece_dst(tid, i) == wino4s_pixel_offset(row) + (tid & 7) * 16, "piece (%d, %d)", tid, i);
            }
        CHECK(rows.size() == 1024, "%zu distinct pieces of a chunk", rows.size());
        claim(owner, lo + W4S_DZERO, W4S_ZAREA, 3000000 + buf, lo, hi, "zero area");
        // patch reads: on the board the pixel's own bytes, off the board the zero area at the same address mod 256
        for (int tile = 0; tile < W4S_TILES; tile++)
            for (int chp = 0; chp < 8; chp++)
                for (int i = 0; i < 4; i++)
                    for (int j = 0; j < 4; j++)
                        for (int kp = 0; kp < 2; kp++) {
                            const int a = wino4s_patch_read(tile, chp, i, j, kp);
                            const int y = 2 * ((tile >> 2) & 3) - 1 + i, x = 2 * (tile & 3) - 1 + j;
                            const bool on = y >= 0 && y < 8 && x >= 0 && x < 8;
                            CHECK(a % 8 == 0 && a >= 0 && a + 8 <= W4S_DBUF, "patch read at %d", a);
                            if (on) CHECK(a == wino4s_pixel_offset((tile >> 4) * 64 + y * 8 + x) + kp * 64 + chp * 8, "patch (%d, %d, %d, %d)", tile, chp, i, j);
                            else CHECK(a >= W4S_DZERO && a + 8 <= W4S_DZERO + W4S_ZAREA, "off-board read at %d", a);
                            CHECK(a == wino4s_patch_read(tile, chp, i, j, 0) + kp * 64, "the half is an added constant");
                            for (int b = lo + a; on && b < lo + a + 8; b++) CHECK(owner[b] >= 2000000 && owner[b] < 3000000, "patch read of byte %d no piece wrote", b);
                        }
    }

    // ---- the exchange: inside its area (over V image 0), every 16 bytes written once, every read of a written slot ----
    {
        std::vector<int> z(W4S_LDS_Z, -1);
        CHECK(W4S_LDS_Z <= W4S_VIMG, "the exchange leaves V image 0");
        for (int q = 0; q < 4; q++)
            for (int c = 0; c < 2; c++)
                for (int lane = 0; lane < 64; lane++)
                    for (int g = 0; g < 4; g++) claim(z, wino4s_z(q, c, lane & 31, g * 2 + (lane >> 5)), 16, ((q * 2 + c) * 64 + lane) * 4 + g, 0, W4S_LDS_Z, "Z write");
        for (int b = 0; b < W4S_LDS_Z; b++) CHECK(z[b] >= 0, "exchange byte %d is never written", b);
        // the output rows: every (row of the 128, unit) once; the tile a pixel reads is the tile that computed it
        std::set<int> outs;
        for (int r = 0; r < 4; r++)
            for (int lane = 0; lane < 64; lane++)
                for (int k = 0; k < 4; k++) {
                    const int p = wino4s_out_pixel(lane, k), row = wino4s_out_row(r, p), tile = wino4s_out_tile(r, p);
                    CHECK(p >= 0 && p < 32 && row >= 0 && row < W4S_ROWS && tile >= 0 && tile < W4S_TILES, "output (%d, %d, %d)", r, lane, k);
                    outs.insert(row * 8 + (lane & 7));
                    const int board = row >> 6, y = (row >> 3) & 7, x = row & 7;
                    CHECK(tile == board * 16 + (y >> 1) * 4 + (x >> 1) && (y >> 1) == r && (y & 1) == (k & 1) && (x & 1) == (p & 1), "pixel %d of wave %d", row, r);
                    for (int i = 0; i < 3; i++) {
                        const int a = wino4s_z((k & 1) + i, p & 1, tile, lane & 7);
                        CHECK(a >= 0 && a + 16 <= W4S_LDS_Z && a % 16 == 0, "Z read at %d", a);
                    }
                }
        CHECK(outs.size() == 1024, "%zu distinct output pieces", outs.size());
    }

    // ---- bank slots of the 16-byte accesses ----
    for (int f = 0; f < 16; f++)
        for (int part = 0; part < 2; part++)
            for (int img = 0; img < 2; img++) check_b128([&](int lane) { return wino4s_v_image(img) + wino4s_v_read(f, lane, part); }, "V fragment read");
    for (int q = 0; q < 4; q++)
        for (int c = 0; c < 2; c++)
            for (int g = 0; g < 4; g++) check_b128([&](int lane) { return wino4s_z(q, c, lane & 31, g * 2 + (lane >> 5)); }, "Z write");
    for (int r = 0; r < 4; r++)
        for (int k = 0; k < 4; k++)
            for (int i = 0; i < 3; i++)
                check_b128([&](int lane) {
                    const int p = wino4s_out_pixel(lane, k);
                    return wino4s_z((k & 1) + i, p & 1, wino4s_out_tile(r, p), lane & 7);
                }, "Z read");
    // the transform's 4-byte V writes: a 32-lane half on 32 different banks
    for (int f = 0; f < 16; f++)
        for (int part = 0; part < 2; part++)
            for (int h = 0; h < 8; h++) {
                std::set<int> banks;
                for (int l = 0; l < 32; l++) banks.insert(wino4s_v_write(f, wino4s_item_tile(h * 32 + l), wino4s_item_chp(h * 32 + l), part) / 4 % 32);
                CHECK(banks.size() == 32, "V write: half wave %d on %zu banks", h, banks.size());
            }

    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("wino4s rule ok\n");
    return 0;
}
