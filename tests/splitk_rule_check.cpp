// Stand-alone program around cattus_amd/csrc/splitk_rule.h (tests/test_splitk_rule.py builds it plain and under sanitizers): the K split,
// the reduction tree, the grid map, every LDS offset of conv3x3_splitk_kernel and the bank slots of its 16-byte accesses.  Prints what
// fails and "splitk rule ok" when nothing does.
#include <stdio.h>

#include <set>
#include <string>
#include <utility>
#include <vector>

#include "splitk_rule.h"

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

// what occupies a byte of LDS during one phase of the kernel
static void claim(std::vector<int>& owner, int at, int len, int who, int lo, int hi, const char* what) {
    CHECK(at >= lo && at + len <= hi, "%s: [%d, %d) outside [%d, %d)", what, at, at + len, lo, hi);
    if (at < 0 || at + len > (int)owner.size()) return;
    for (int b = at; b < at + len; b++) {
        CHECK(owner[b] == -1 || owner[b] == who, "%s: byte %d claimed twice (%d, %d)", what, b, owner[b], who);
        owner[b] = who;
    }
}

// MI355X: a ds_read_b128 is served in four groups of 16 lanes, banks = (address / 4) mod 64: a group is conflict-free when its lanes fall
// on 16 different 16-byte slots of the 256-byte bank row, or read the very same address (a broadcast)
static const int GROUPS[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
template <class F>
static void check_read_b128(F&& address, const char* what) {
    for (int half = 0; half < 2; half++)
        for (int g = 0; g < 2; g++) {
            std::set<int> slots, addresses;
            for (int k = 0; k < 16; k++) {
                const int a = address(GROUPS[g][k] + 32 * half);
                CHECK(a % 16 == 0, "%s: address %d is not 16-byte aligned", what, a);
                slots.insert((a / 16) % 16);
                addresses.insert(a);
            }
            CHECK(slots.size() == addresses.size(), "%s: lane group %d of half %d: %zu addresses on %zu bank slots", what, g, half, addresses.size(), slots.size());
        }
}
// a ds_write_b128 is served in eight groups of 8 contiguous lanes, banks = (address / 4) mod 32: 8 different slots of the 128-byte row
template <class F>
static void check_write_b128(F&& address, const char* what) {
    for (int g = 0; g < 8; g++) {
        std::set<int> slots;
        for (int k = 0; k < 8; k++) {
            const int a = address(g * 8 + k);
            CHECK(a % 16 == 0, "%s: address %d is not 16-byte aligned", what, a);
            slots.insert((a / 16) % 8);
        }
        CHECK(slots.size() == 8, "%s: lane group %d on %zu bank slots", what, g, slots.size());
    }
}

// the tree written as a formula: sum(first, count) = (sum(first, count / 2) + sum(first + count / 2, count / 2))
static std::string tree_formula(int first, int count) {
    if (count == 1) return "p" + std::to_string(first);
    return "(" + tree_formula(first, count / 2) + "+" + tree_formula(first + count / 2, count / 2) + ")";
}

int main() {
    // ---- the K split: contiguous, non-empty ranges that partition [0, chunks); a function of the chunk count alone ----
    CHECK(SK_MAX_CHUNKS == 16 && SK_MAX_FILTERS == 512 && SK_MIN_CHUNKS == 4, "bounds %d %d %d", SK_MAX_CHUNKS, SK_MAX_FILTERS, SK_MIN_CHUNKS);
    for (int chunks = SK_MIN_CHUNKS; chunks <= SK_MAX_CHUNKS; chunks++)
        for (int forced : {0, 1, 2, 4, 8, 3, 16, -1}) {
            const int ways = splitk_ways(chunks, forced);
            CHECK(ways == 1 || ways == 2 || ways == 4 || ways == 8, "chunks %d forced %d: %d ways", chunks, forced, ways);
            CHECK(ways <= chunks && ways <= SK_MAX_WAYS, "chunks %d forced %d: %d ways", chunks, forced, ways);
            if (forced == 1 || forced == 2 || forced == 4 || forced == 8)  // taken as it is, or halved until every wave has a chunk
                CHECK(ways == (forced <= chunks ? forced : 4), "chunks %d forced %d: %d ways", chunks, forced, ways);
            else CHECK(ways == (chunks >= 8 ? 8 : 4), "chunks %d: %d ways by the rule (a forced count that is no way count is ignored)", chunks, ways);
            CHECK(splitk_bound(chunks, ways, 0) == 0 && splitk_bound(chunks, ways, ways) == chunks, "chunks %d ways %d: ends %d %d", chunks, ways,
                  splitk_bound(chunks, ways, 0), splitk_bound(chunks, ways, ways));
            std::vector<int> seen(chunks, 0);
            int longest = 0, shortest = chunks;
            for (int w = 0; w < ways; w++) {
                const int lo = splitk_bound(chunks, ways, w), hi = splitk_bound(chunks, ways, w + 1);
                CHECK(lo < hi, "chunks %d ways %d: wave %d has the empty range [%d, %d)", chunks, ways, w, lo, hi);
                for (int c = lo; c < hi && c < chunks; c++) seen[c]++;
                longest = hi - lo > longest ? hi - lo : longest;
                shortest = hi - lo < shortest ? hi - lo : shortest;
            }
            for (int c = 0; c < chunks; c++) CHECK(seen[c] == 1, "chunks %d ways %d: chunk %d walked %d times", chunks, ways, c, seen[c]);
            CHECK(longest - shortest <= 1, "chunks %d ways %d: ranges of %d and %d chunks", chunks, ways, shortest, longest);
            // the exchange lies over the images: a wave's tile fits the images of the chunks in front of and including its own
            CHECK(ways * SK_XWAVE <= splitk_lds_bytes(chunks), "chunks %d ways %d: the exchange does not fit the images", chunks, ways);
        }
    // the shapes the GPU tests name
    CHECK(splitk_ways(4) == 4 && splitk_ways(6) == 4 && splitk_ways(8) == 8 && splitk_ways(10) == 8 && splitk_ways(16) == 8, "ways of 4, 6, 8, 10, 16 chunks");
    CHECK(splitk_bound(6, 4, 1) == 2 && splitk_bound(6, 4, 2) == 4 && splitk_bound(6, 4, 3) == 5, "6 chunks: ranges 2, 2, 1, 1");

    // ---- the reduction tree: ways - 1 steps, every partial read exactly once, the pairwise order by wave index ----
    for (int ways : {1, 2, 4, 8}) {
        std::vector<std::string> slot(ways);
        std::vector<int> live(ways, 1);
        for (int w = 0; w < ways; w++) slot[w] = "p" + std::to_string(w);
        for (int s = 0; s + 1 < ways; s++) {
            const int dst = splitk_tree_dst(ways, s), src = splitk_tree_src(ways, s);
            CHECK(dst >= 0 && src > dst && src < ways && src - dst == splitk_tree_span(ways, s), "ways %d step %d: %d <- %d", ways, s, dst, src);
            if (dst < 0 || src <= dst || src >= ways) continue;
            CHECK(live[dst] && live[src], "ways %d step %d: slot %d or %d was already added into another", ways, s, dst, src);
            slot[dst] = "(" + slot[dst] + "+" + slot[src] + ")";
            live[src] = 0;
        }
        int left = 0;
        for (int w = 0; w < ways; w++) left += live[w];
        CHECK(left == 1 && live[0], "ways %d: %d slots left", ways, left);
        CHECK(slot[0] == tree_formula(0, ways), "ways %d: %s, not %s", ways, slot[0].c_str(), tree_formula(0, ways).c_str());
        for (int w = 0; w < ways; w++) {
            const std::string name = "p" + std::to_string(w);
            size_t count = 0;
            for (size_t at = slot[0].find(name); at != std::string::npos; at = slot[0].find(name, at + 1)) count++;
            CHECK(count == 1, "ways %d: partial %d read %zu times", ways, w, count);
        }
    }

    // ---- the grid: a bijection onto (board, cout block); with the XCD map the cout blocks of a board share index % 8 ----
    for (int cout : {128, 192, 256, 320, 512})
        for (int boards : {4, 8, 12, 20, 36, 40, 128}) {
            const int ncb = cout / SK_COUTS, nblk = (int)splitk_grid((uint32_t)boards, (uint32_t)cout);
            CHECK(nblk == boards * ncb, "grid %d", nblk);
            std::set<std::pair<int, int>> seen;
            std::vector<int> xcd(boards, -1);
            for (int wg = 0; wg < nblk; wg++) {
                const int logical = splitk_logical(wg, nblk);
                const int board = splitk_board(logical, ncb), cb = splitk_cout_block(logical, ncb);
                CHECK(logical >= 0 && logical < nblk && board >= 0 && board < boards && cb >= 0 && cb < ncb, "wg %d of %d -> (%d, %d)", wg, nblk, board, cb);
                seen.insert({board, cb});
                if (board < 0 || board >= boards) continue;
                if (nblk % 8 == 0 && (nblk / 8) % ncb == 0) {  // an XCD's range of logical indices holds whole boards
                    CHECK(xcd[board] == -1 || xcd[board] == wg % 8, "filters %d boards %d: board %d on XCDs %d and %d", cout, boards, board, xcd[board], wg % 8);
                    xcd[board] = wg % 8;
                }
            }
            CHECK((int)seen.size() == nblk, "filters %d boards %d: %zu of %d tiles taken", cout, boards, seen.size(), nblk);
        }

    // ---- LDS during the K walk: images and zero areas on bytes of their own, inside the total, the total inside 160 KiB ----
    for (int chunks = SK_MIN_CHUNKS; chunks <= SK_MAX_CHUNKS; chunks++) {
        const int total = splitk_lds_bytes(chunks);
        CHECK(total <= 160 * 1024, "chunks %d: %d bytes of LDS", chunks, total);
        std::vector<int> owner(total, -1);
        for (int c = 0; c < chunks; c++) {
            const int img = splitk_image(c);
            CHECK(img % 256 == 0, "image %d at %d", c, img);
            std::set<int> pieces;
            for (int i = 0; i < 8; i++)
                for (int lane = 0; lane < 64; lane++) {
                    const int row = splitk_piece_row(lane, i);
                    CHECK(row >= 0 && row < SK_ROWS, "piece row %d", row);
                    CHECK(splitk_piece_dst(lane, i) == row * SK_PP + (lane & 7) * 16, "piece (%d, %d)", lane, i);
                    pieces.insert(row * 8 + (lane & 7));
                    claim(owner, img + splitk_piece_dst(lane, i), 16, 2 * c, img, img + SK_DZERO, "image piece");
                }
            CHECK(pieces.size() == 512, "a chunk's %zu pieces", pieces.size());
            for (int lane = 0; lane < SK_ZAREA / 16; lane++) claim(owner, img + SK_DZERO + lane * 16, 16, 2 * c + 1, img + SK_DZERO, img + SK_IMG, "zero area");
        }
        // ---- LDS during the reduction: the waves' exchange tiles on bytes of their own, inside the total ----
        for (int forced : {0, 1, 2, 4, 8}) {
            const int ways = splitk_ways(chunks, forced);
            std::vector<int> xo(total, -1);
            for (int w = 0; w < ways; w++)
                for (int p = 0; p < SK_ROWS; p++)
                    for (int u = 0; u < 8; u++) claim(xo, splitk_x(w, p, u), 16, (w * SK_ROWS + p) * 8 + u, w * SK_XWAVE, (w + 1) * SK_XWAVE, "exchange unit");
            CHECK(ways * SK_XWAVE <= total, "chunks %d ways %d: exchange past the end", chunks, ways);
        }
    }

    // ---- the image's fill: one ds_write_b128 per piece index ----
    for (int i = 0; i < 8; i++) check_write_b128([&](int lane) { return splitk_piece_dst(lane, i); }, "image fill");

    // ---- the pixel fragments: ds_read_b128 of (tap, pixel block, k-half, hi / lo) for every board edge; off-board reads in the zero area ----
    for (int S = 1; S <= 8; S++)
        for (int tap = 0; tap < 9; tap++)
            for (int pb = 0; pb < 2; pb++)
                for (int k = 0; k < 2; k++)
                    for (int lo = 0; lo < 2; lo++) {
                        auto address = [&](int lane) { return splitk_tap_read(S, pb * 32 + (lane & 31), tap, lane >> 5) + splitk_frag_offset(k, lo); };
                        check_read_b128(address, "pixel fragment");
                        for (int lane = 0; lane < 64; lane++) {
                            const int p = pb * 32 + (lane & 31), py = p / S, px = p % S, hh = py + tap / 3 - 1, ww = px + tap % 3 - 1;
                            const bool on = p < S * S && hh >= 0 && hh < S && ww >= 0 && ww < S;
                            const int a = address(lane);
                            if (on) {
                                CHECK(a == (hh * S + ww) * SK_PP + (lane >> 5) * 16 + k * 32 + lo * 64, "S %d tap %d pixel %d: %d", S, tap, p, a);
                                CHECK(a >= 0 && a + 16 <= SK_DZERO && a % SK_PP + 16 <= 128, "S %d tap %d pixel %d reads [%d, +16): not a row's data", S, tap, p, a);
                            } else {
                                CHECK(a >= SK_DZERO && a + 16 <= SK_DZERO + SK_ZAREA, "S %d tap %d pixel %d: off-board read at %d outside the zero area", S, tap, p, a);
                            }
                        }
                    }

    // ---- the exchange: the accumulators' ds_write_b128 and the finishing threads' ds_read_b128 ----
    {
        std::set<int> sw;
        for (int p = 0; p < 8; p++) sw.insert(splitk_x_swizzle(p));
        CHECK(sw.size() == 8, "the swizzle of 8 consecutive pixels: %zu values", sw.size());
    }
    for (int w = 0; w < SK_MAX_WAYS; w++)
        for (int pb = 0; pb < 2; pb++)
            for (int g = 0; g < 4; g++)
                check_write_b128([&](int lane) { return splitk_x(w, pb * 32 + (lane & 31), g * 2 + (lane >> 5)); }, "exchange write");
    {
        // every (wave's tile, pixel, unit) is written once by (pixel block, g, lane) and read once by (item, half)
        std::set<int> written, read;
        for (int pb = 0; pb < 2; pb++)
            for (int g = 0; g < 4; g++)
                for (int lane = 0; lane < 64; lane++) written.insert(splitk_x(0, pb * 32 + (lane & 31), g * 2 + (lane >> 5)));
        for (int item = 0; item < SK_ITEMS; item++)
            for (int half = 0; half < 2; half++) read.insert(splitk_x(0, splitk_item_pixel(item), 2 * splitk_item_cg(item) + half));
        CHECK(written.size() == 512 && read == written, "exchange: %zu units written, %zu read", written.size(), read.size());
    }
    for (int w = 0; w < SK_MAX_WAYS; w++)
        for (int first = 0; first < SK_ITEMS; first += 64)  // a wave's 64 items of one trip, whatever the thread count
            for (int half = 0; half < 2; half++)
                check_read_b128([&](int lane) { return splitk_x(w, splitk_item_pixel(first + lane), 2 * splitk_item_cg(first + lane) + half); }, "exchange read");
    for (int threads : {64, 128, 256, 512})
        for (int tid = 0; tid < threads; tid++)
            for (int item = tid; item < SK_ITEMS; item += threads) CHECK(splitk_item_cg(item) == splitk_item_cg(tid), "thread %d of %d: item %d", tid, threads, item);

    if (failures) printf("%d checks failed\n", failures);
    else printf("splitk rule ok\n");
    return failures ? 1 : 0;
}
