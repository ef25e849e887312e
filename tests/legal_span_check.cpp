// Stand-alone check of the ragged legal-list layout (cattus_amd/csrc/legal_span.h; built and run by tests/test_legal_span.py with the host
// compiler, once plain and once under AddressSanitizer / UBSan: no HIP, no GPU).  Reads a file of cases, all numbers decimal:
//   "L moves count i0 .. i(count-1)"        one leaf's list            -> "fault at"   (legal_list_check; at = 0 unless fault == 2)
//   "O n o0 .. on"                           an offset table            -> "fault at"   (legal_offsets_check)
//   "A leaves m slot0 count0 .. slot(m-1) count(m-1)"   m submits with a list into a batch that ends with `leaves` leaves; the j-th index
//                                            appended overall is j % 65521  -> "total o0 .. o(leaves)" after legal_close, or "bad" when the
//                                            lists do not lie at their offsets
//   "W n o0 .. on"                           a valid table              -> the owner of every element k < on, space separated
// and ends with "legal span ok" when its own fixed points hold too.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "legal_span.h"

using namespace cattus;

static int failures = 0;
#define CHECK(cond, ...) \
    do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check_fixed_points() {
    const uint32_t moves = 1880;
    uint32_t at = 77;
    // counts 0, 1, 1024, 1025: exactly-sized lists, so that a read past one is AddressSanitizer's to find
    for (uint32_t count : {0u, 1u, 1024u, 1025u}) {
        std::vector<uint16_t> list(count);
        for (uint32_t k = 0; k < count; k++) list[k] = (uint16_t)(k % moves);
        const LegalFault f = legal_list_check(list.data(), count, moves, &at);
        CHECK(f == (count > LEGAL_CAP ? LEGAL_TOO_LONG : LEGAL_OK), "count %u: fault %d", count, (int)f);
    }
    std::vector<uint16_t> list{5, 1879, 1880, 7};
    CHECK(legal_list_check(list.data(), 4, moves, &at) == LEGAL_BAD_INDEX && at == 2, "an index equal to moves, at %u", at);
    CHECK(legal_list_check(list.data(), 2, moves, &at) == LEGAL_OK, "the largest index");
    CHECK(legal_list_check(nullptr, 0, moves, nullptr) == LEGAL_OK, "no list, no entries");

    const uint32_t good[5] = {0, 0, 3, 3, 1027}, from1[3] = {1, 2, 3}, down[4] = {0, 5, 4, 9}, wide[3] = {0, 1025, 1025}, none[4] = {0, 0, 0, 0};
    CHECK(legal_offsets_check(good, 4, &at) == LEGAL_OK, "empty spans and a full one");
    CHECK(legal_offsets_check(from1, 2, &at) == LEGAL_BAD_OFFSETS && at == 0, "offsets not starting at 0");
    CHECK(legal_offsets_check(down, 3, &at) == LEGAL_BAD_OFFSETS && at == 1, "offsets descending, at %u", at);
    CHECK(legal_offsets_check(wide, 2, &at) == LEGAL_TOO_LONG && at == 0, "a span of 1025");
    CHECK(legal_offsets_check(none, 3, &at) == LEGAL_OK && none[3] == 0, "total == 0");
    CHECK(legal_offsets_check(none, 0, &at) == LEGAL_OK, "no leaf at all");
    CHECK(legal_span(good, 1).begin == 0 && legal_span(good, 1).count == 3 && legal_span(good, 3).begin == 3 && legal_span(good, 3).count == 1024 &&
              legal_span(good, 0).count == 0 && legal_span(good, 2).count == 0,
          "spans");
    CHECK(legal_owner(good, 4, 0) == 1 && legal_owner(good, 4, 2) == 1 && legal_owner(good, 4, 3) == 3 && legal_owner(good, 4, 1026) == 3, "owners");

    // append: plain leaves in slots 0 and 2, lists in 1 and 3, one plain leaf behind them
    std::vector<uint16_t> idx;
    std::vector<uint32_t> off;
    const uint16_t a[3] = {9, 8, 7}, b[1] = {6};
    legal_append(idx, off, 1, a, 3);
    legal_append(idx, off, 3, b, 1);
    legal_close(off, 5);
    CHECK(off == (std::vector<uint32_t>{0, 0, 3, 3, 4, 4}) && idx == (std::vector<uint16_t>{9, 8, 7, 6}), "append");
    std::vector<uint32_t> plain;
    legal_close(plain, 3);
    CHECK(plain == (std::vector<uint32_t>{0, 0, 0, 0}), "a batch without a list");
    std::vector<uint16_t> idx0;
    std::vector<uint32_t> off0;
    legal_append(idx0, off0, 0, nullptr, 0);
    legal_close(off0, 1);
    CHECK(off0 == (std::vector<uint32_t>{0, 0}) && idx0.empty(), "a list of no entries in slot 0");
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
                uint32_t moves = 0, count = 0, at = 0;
                ls >> moves >> count;
                std::vector<uint16_t> list(count);
                for (auto& v : list) {
                    uint32_t x = 0;
                    ls >> x;
                    v = (uint16_t)x;
                }
                const LegalFault f = legal_list_check(list.data(), count, moves, &at);
                printf("%d %u\n", (int)f, f == LEGAL_BAD_INDEX ? at : 0u);
            } else if (kind == "O" || kind == "W") {
                uint32_t n = 0, at = 0;
                ls >> n;
                std::vector<uint32_t> off((size_t)n + 1);
                for (auto& v : off) ls >> v;
                const LegalFault f = legal_offsets_check(off.data(), n, &at);
                if (kind == "O") {
                    printf("%d %u\n", (int)f, f ? at : 0u);
                } else {
                    CHECK(f == LEGAL_OK, "W line with a bad table");
                    for (uint32_t k = 0; f == LEGAL_OK && k < off[n]; k++) {
                        const uint32_t leaf = legal_owner(off.data(), n, k);
                        const LegalSpan sp = legal_span(off.data(), leaf);
                        CHECK(leaf < n && sp.begin <= k && k - sp.begin < sp.count, "element %u is not in leaf %u's span", k, leaf);
                        printf("%s%u", k ? " " : "", leaf);
                    }
                    printf("\n");
                }
            } else if (kind == "A") {
                uint32_t leaves = 0, m = 0, next = 0;
                ls >> leaves >> m;
                std::vector<uint16_t> idx;
                std::vector<uint32_t> off, slots, counts;
                for (uint32_t j = 0; j < m; j++) {
                    uint32_t slot = 0, count = 0;
                    ls >> slot >> count;
                    std::vector<uint16_t> list(count);
                    for (auto& v : list) v = (uint16_t)(next++ % 65521);
                    legal_append(idx, off, slot, list.data(), count);
                    slots.push_back(slot), counts.push_back(count);
                }
                legal_close(off, leaves);
                bool good = off.size() == (size_t)leaves + 1 && off.back() == idx.size() && legal_offsets_check(off.data(), leaves, nullptr) != LEGAL_BAD_OFFSETS;
                for (uint32_t j = 0, seen = 0; good && j < m; j++) {
                    const LegalSpan sp = legal_span(off.data(), slots[j]);
                    good = sp.count == counts[j] && sp.begin == seen;
                    for (uint32_t k = 0; good && k < sp.count; k++) good = idx[sp.begin + k] == (uint16_t)((seen + k) % 65521);
                    seen += counts[j];
                }
                if (!good) {
                    printf("bad\n");
                } else {
                    printf("%zu", idx.size());
                    for (uint32_t v : off) printf(" %u", v);
                    printf("\n");
                }
            }
            CHECK(!ls.fail(), "bad line: %s", line.c_str());
        }
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("legal span ok\n");
    return 0;
}
