// Stand-alone program around cattus_amd/csrc/t64f_rule.h (tests/test_t64f_rule.py builds it plain and under sanitizers): the LDS plan of
// tower64_f32_kernel's three instances, the step table of towers of 0 .. 6 blocks at 16 / 32 / 33 / 64 filters beside the per-layer walk,
// the ownership map of the consumer lanes as a bijection onto the workgroup's rows x 64 channels, the LDS offset the epilogue stores to
// against the offset the next layer's fragment read takes the same (row, k) from, the bank slots of the fragment reads and of the
// epilogue's stores, the tap rows, and the resident dataflow walked beside the per-layer f32 plan, tensor for tensor.  Prints what fails
// and "t64f rule ok" when nothing does.
#include <stdio.h>
#include <string.h>

#include <set>
#include <vector>

#include "t64f_rule.h"

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

static const int SHAPES[][2] = {{4, 64}, {2, 64}, {2, 128}};  // (CH, pixel slots per board): the kernel's three instances

// ---- 1. the LDS plan ----
static void check_lds() {
    const int want_total[] = {107008, 139776, 139776};
    int i = 0;
    for (const auto& sh : SHAPES) {
        const int ch = sh[0], rows = t64f_rows(ch);
        const T64fLds L = t64f_lds(ch);
        // regions in order: ring, buffer 0 (two chunks), its zero area, buffer 1, its zero area
        const int begin[] = {L.ring, L.buf[0], L.buf[0] + L.chunk_stride, L.buf[0] + L.zero_off, L.buf[1], L.buf[1] + L.chunk_stride, L.buf[1] + L.zero_off};
        const int size[] = {T64F_RING * T64F_SLAB, rows * 128, rows * 128, T64F_ZAREA, rows * 128, rows * 128, T64F_ZAREA};
        for (int a = 0; a < 7; a++) {
            CHECK(begin[a] % 16 == 0 && size[a] % 16 == 0 && begin[a] >= 0, "CH %d region %d at %d + %d", ch, a, begin[a], size[a]);
            CHECK(begin[a] + size[a] == (a + 1 < 7 ? begin[a + 1] : L.total), "CH %d region %d ends at %d", ch, a, begin[a] + size[a]);
        }
        CHECK(L.total <= T64F_LDS_MAX && L.total == want_total[i], "CH %d: %d bytes", ch, L.total);
        CHECK((L.buf[0] + L.zero_off) % 256 == 0 && (L.buf[1] + L.zero_off) % 256 == 0 && L.buf[0] % 256 == 0 && L.buf[1] % 256 == 0 && L.chunk_stride % 256 == 0,
              "CH %d: the zero areas and the chunks keep a row's banks only if they are 256-B aligned", ch);
        i++;
    }
    CHECK(T64F_SLAB == 24576 && T64F_PIECES * 1024 == T64F_SLAB, "slab %d", T64F_SLAB);
}

// ---- 2. the step table ----
static void check_steps() {
    const uint32_t filters_of[] = {16, 32, 33, 64};
    for (uint32_t blocks = 0; blocks <= 6; blocks++)
        for (uint32_t filters : filters_of)
            for (int narrow_on = 0; narrow_on < 2; narrow_on++) {
                const int nlayers = (int)t64f_layers(blocks), nch = t64f_hidden_chunks(filters, narrow_on != 0);
                CHECK(nch == (narrow_on && filters <= 32 ? 1 : 2), "%u filters, narrow %d: %d chunks", filters, narrow_on, nch);
                // the per-layer walk, layer by layer: for chunk, for dy -- a hidden layer of the per-layer kernel has cin / 32 = 2 chunks
                std::vector<T64fStep> want, full;
                for (int l = 0; l < nlayers; l++)
                    for (int c = 0; c < (l == 0 ? 1 : 2); c++)
                        for (int dy = 0; dy < 3; dy++) {
                            full.push_back(T64fStep{l, c, dy});
                            if (!(nch == 1 && l > 0 && c == 1)) want.push_back(T64fStep{l, c, dy});  // the narrow walk drops exactly the chunk-1 steps of hidden layers
                        }
                const int T = t64f_steps(nlayers, nch);
                CHECK(T == (int)want.size(), "%u blocks, %u filters, narrow %d: %d steps, want %zu", blocks, filters, narrow_on, T, want.size());
                if (nch == 2) CHECK(want.size() == full.size(), "the full walk is the per-layer walk");
                if (T != (int)want.size()) continue;
                int per_layer = 0, last_layer = -1;
                for (int s = 0; s < T; s++) {
                    const T64fStep st = t64f_step(s, nch);
                    CHECK(st.layer == want[s].layer && st.chunk == want[s].chunk && st.dy == want[s].dy, "step %d: (%d, %d, %d), want (%d, %d, %d)", s, st.layer, st.chunk,
                          st.dy, want[s].layer, want[s].chunk, want[s].dy);
                    CHECK(st.chunk < t64f_layer_chunks(st.layer, nch), "step %d: chunk %d of layer %d", s, st.chunk, st.layer);
                    per_layer = st.layer == last_layer ? per_layer + 1 : 1;
                    last_layer = st.layer;
                    // the kernel's consumers take ring slot dy: every layer has a multiple of three steps
                    CHECK(t64f_ring_slot(s) == s % 3 && t64f_ring_slot(s) == st.dy, "step %d: ring slot %d, dy %d", s, t64f_ring_slot(s), st.dy);
                    // while step s is read, the slabs of steps s + 1 .. s + AHEAD are being written: other slots
                    for (int a = 1; a <= T64F_AHEAD && s + a < T; a++) CHECK(t64f_ring_slot(s + a) != t64f_ring_slot(s), "steps %d and %d share a ring slot", s, s + a);
                    // the slab written behind barrier s (step s + AHEAD) is the slot of step s - 1, which everybody has left
                    if (s >= 1 && s + T64F_AHEAD < T) CHECK(t64f_ring_slot(s + T64F_AHEAD) == t64f_ring_slot(s - 1), "step %d's refill", s);
                    // source bytes stay inside the layer's [9][64][Cin_pad] f32 rows, and are the per-layer kernel's: tap row dy, the chunk's 128 bytes
                    const int rb = t64f_row_bytes(st.layer), src = t64f_slab_src(st), bytes = t64f_layer_weight_bytes(st.layer);
                    CHECK(rb == (st.layer == 0 ? 32 : 64) * 4 && bytes == 9 * 64 * rb, "layer %d: %d-byte rows", st.layer, rb);
                    CHECK(src == (st.dy * 3) * 64 * rb + st.chunk * 128, "step %d: slab source %d", s, src);
                    std::set<int> dst16;
                    for (int pid = 0; pid < T64F_PIECES; pid++)
                        for (int lane = 0; lane < 64; lane++) {
                            const int off = src + t64f_piece_src(pid, lane, rb), dst = t64f_piece_dst(pid) + lane * 16;
                            CHECK(off >= 0 && off + 16 <= bytes && off % 16 == 0, "step %d piece %d lane %d: source %d of %d", s, pid, lane, off, bytes);
                            CHECK(dst >= 0 && dst + 16 <= T64F_SLAB, "piece %d lane %d: destination %d", pid, lane, dst);
                            dst16.insert(dst);
                            // what landed there is (tap, cout, 16-byte slot c) of the chunk, where the weight fragment read looks for it
                            const int tap = pid >> 3, cout = (pid & 7) * 8 + (lane >> 3);
                            const int c = (off - src - (tap * 64 + cout) * rb) / 16;
                            CHECK(c >= 0 && c < 8 && (off - src) == (tap * 64 + cout) * rb + c * 16, "piece %d lane %d: slot %d", pid, lane, c);
                            CHECK(dst == t64f_wfrag_offset(tap, cout, c >> 1, c & 1), "piece %d lane %d: lands at %d, read at %d", pid, lane, dst, t64f_wfrag_offset(tap, cout, c >> 1, c & 1));
                        }
                    CHECK(dst16.size() == (size_t)T64F_SLAB / 16, "step %d: %zu of %d slots of the slab written", s, dst16.size(), T64F_SLAB / 16);
                }
            }
}

// ---- 3. the ownership map, 4. where an element lives ----
static void check_ownership() {
    for (const auto& sh : SHAPES) {
        const int ch = sh[0], slots = sh[1], rows = t64f_rows(ch), npb = t64f_npb(ch);
        const T64fLds L = t64f_lds(ch);
        CHECK(rows == 256 / ch && rows % slots == 0, "CH %d: %d rows, %d slots", ch, rows, slots);
        const size_t row0 = (size_t)3 * rows;  // the fourth workgroup of a launch
        std::vector<int> owners((size_t)rows * 64, 0);
        std::vector<int> lds_owner((size_t)rows * 64, -1);  // per f32 of a buffer's two chunks
        std::vector<int> out_owner((size_t)rows * 64, -1);
        for (int wave = 0; wave < 4; wave++)
            for (int lane = 0; lane < 64; lane++)
                for (int pb = 0; pb < npb; pb++)
                    for (int e = 0; e < 16; e++) {
                        const T64fOwn o = t64f_own(ch, wave, lane, pb, e);
                        CHECK(o.row >= 0 && o.row < rows && o.channel >= 0 && o.channel < 64, "CH %d wave %d lane %d pb %d e %d: (%d, %d)", ch, wave, lane, pb, e, o.row, o.channel);
                        if (o.row < 0 || o.row >= rows || o.channel < 0 || o.channel >= 64) return;
                        owners[(size_t)o.row * 64 + o.channel]++;
                        const T64fOwn first = t64f_own(ch, wave, lane & 32, pb, e);
                        CHECK((row0 + (size_t)o.row) / slots == (row0 + (size_t)first.row) / slots, "CH %d wave %d pb %d: a pixel block crosses a board", ch, wave, pb);
                        // a wave writes one chunk only: its cout half
                        CHECK((o.channel >> 5) == (wave & 1), "CH %d wave %d: channel %d", ch, wave, o.channel);
                        const int at = t64f_lds_offset(ch, o.row, o.channel);
                        CHECK(at >= 0 && at + 4 <= L.zero_off && at % 4 == 0, "CH %d: LDS offset %d of %d", ch, at, L.zero_off);
                        if (at < 0 || at + 4 > L.zero_off) return;
                        CHECK(lds_owner[at / 4] == -1, "CH %d: LDS byte %d written twice", ch, at);
                        lds_owner[at / 4] = o.row * 64 + o.channel;
                        // elements 4g .. 4g + 3 are one aligned 16-byte slot: the store is the first one's offset
                        const T64fOwn g0 = t64f_own(ch, wave, lane, pb, e & ~3);
                        CHECK(at == t64f_lds_offset(ch, g0.row, g0.channel) + (e & 3) * 4 && t64f_lds_offset(ch, g0.row, g0.channel) % 16 == 0, "CH %d e %d: not a 16-byte group", ch, e);
                        const size_t oi = t64f_out_index(row0, o);
                        CHECK(oi >= row0 * 64 && oi < (row0 + rows) * 64 && oi == (row0 + o.row) * 64 + o.channel, "CH %d: output index %zu", ch, oi);
                        if (oi < row0 * 64 || oi >= (row0 + rows) * 64) return;
                        out_owner[oi - row0 * 64] = o.row * 64 + o.channel;
                        CHECK(t64f_out_index(row0, g0) % 4 == 0, "CH %d: the last layer's 16-byte store is aligned", ch);
                    }
        for (size_t i = 0; i < owners.size(); i++) {
            CHECK(owners[i] == 1, "CH %d: (row %zu, channel %zu) owned %d times", ch, i / 64, i % 64, owners[i]);
            CHECK(lds_owner[i] >= 0 && out_owner[i] == (int)i, "CH %d: element %zu", ch, i);
        }
        // what the epilogue stored is what the next layer's fragment read takes (row, k) from, under Mfma<float>'s lane map
        for (int row = 0; row < rows; row++)
            for (int chunk = 0; chunk < 2; chunk++)
                for (int ks = 0; ks < 4; ks++)
                    for (int h = 0; h < 2; h++) {
                        const int at = t64f_frag_offset(ch, chunk, row, ks, h);
                        CHECK(at % 16 == 0 && at >= 0 && at + 16 <= L.zero_off, "CH %d: fragment offset %d", ch, at);
                        for (int j = 0; j < 4; j++) {
                            const int k = t64f_frag_channel(chunk, ks, h, j);
                            CHECK(k == chunk * 32 + ks * 8 + 4 * h + j, "k of (chunk %d, ks %d, h %d, j %d)", chunk, ks, h, j);  // device_common.h: lane half h holds k = 4h + j
                            CHECK(at + 4 * j == t64f_lds_offset(ch, row, k), "CH %d row %d k %d: read at %d, stored at %d", ch, row, k, at + 4 * j, t64f_lds_offset(ch, row, k));
                            if (at + 4 * j == t64f_lds_offset(ch, row, k)) CHECK(lds_owner[(at + 4 * j) / 4] == row * 64 + k, "CH %d row %d k %d: another element lives there", ch, row, k);
                        }
                    }
    }
}

// ---- the bank slots: a ds_read_b128 / ds_write_b128 is served in groups of 16 lanes, a group is conflict-free on 16 different 16-byte slots of the 256-byte bank row ----
static int epilogue_slots_pinned = 0;
static void check_banks() {
    for (const auto& sh : SHAPES) {
        const int ch = sh[0], slots = sh[1], npb = t64f_npb(ch);
        const T64fLds L = t64f_lds(ch);
        const bool big = slots == 128;
        for (int S = (big ? 9 : 2); S <= (big ? 11 : 8); S++)
            for (int wave = 0; wave < 4; wave++) {
                const int rb = ch == 2 ? wave >> 1 : 0, pb0 = ch == 4 ? wave >> 1 : 0;
                const int pslot0 = big ? (rb & 1) * 64 : 0, board_row = big ? 0 : rb * 64;
                for (int pb = 0; pb < npb; pb++)
                    for (int dy = 0; dy < 3; dy++)
                        for (int dx = 0; dx < 3; dx++)
                            for (int chunk = 0; chunk < 2; chunk++)
                                for (int ks = 0; ks < 4; ks++)
                                    for (int grp = 0; grp < 4; grp++) {
                                        std::set<int> bank;
                                        for (int l = 0; l < 16; l++) {
                                            const int lane = grp * 16 + l, r = lane & 31, h = lane >> 5;
                                            const int p = pslot0 + (pb0 + pb) * 32 + r;
                                            const T64fTap tap = t64f_tap(ch, S, board_row, p, dy, dx);
                                            const int at = tap.rel + (tap.ok ? chunk * L.chunk_stride : 0) + (((h ^ tap.swz) << 4) ^ (ks << 5));  // the kernel's address, from the buffer's base
                                            CHECK(at >= 0 && at + 16 <= L.zero_off + T64F_ZAREA && at % 16 == 0, "CH %d S %d: tap address %d", ch, S, at);
                                            if (tap.ok) {
                                                // an on-board tap reads its pixel's row where the epilogue stored it
                                                const int ph = p / S, pw = p % S, q = (ph + dy - 1) * S + pw + dx - 1;
                                                CHECK(q >= 0 && q < S * S && at == t64f_frag_offset(ch, chunk, board_row + q, ks, h), "CH %d S %d p %d tap (%d, %d): address %d", ch, S, p, dy, dx, at);
                                            } else {
                                                CHECK(at >= L.zero_off, "CH %d S %d p %d tap (%d, %d): an off-board tap outside the zero area (%d)", ch, S, p, dy, dx, at);
                                            }
                                            bank.insert((at % 256) / 16);
                                        }
                                        CHECK(bank.size() == 16, "CH %d S %d wave %d tap (%d, %d) ks %d lanes %d..: %zu bank slots", ch, S, wave, dy, dx, ks, grp * 16, bank.size());
                                    }
            }
        // the epilogue's stores (and its skip reads, the same addresses): per 16-lane group of one (pb, g)
        for (int wave = 0; wave < 4; wave++)
            for (int pb = 0; pb < npb; pb++)
                for (int g = 0; g < 4; g++)
                    for (int grp = 0; grp < 4; grp++) {
                        std::set<int> bank;
                        for (int l = 0; l < 16; l++) {
                            const T64fOwn o = t64f_own(ch, wave, grp * 16 + l, pb, g * 4);
                            bank.insert((t64f_lds_offset(ch, o.row, o.channel) % 256) / 16);
                        }
                        CHECK(bank.size() == 16, "CH %d wave %d pb %d g %d lanes %d..: the stores hit %zu bank slots", ch, wave, pb, g, grp * 16, bank.size());
                        if (bank.size() == 16) epilogue_slots_pinned++;
                    }
    }
    // pinned: every one of the 4 waves x npb x 4 groups x 4 lane groups of the three instances stores to 16 different slots
    CHECK(epilogue_slots_pinned == 4 * 4 * 4 * (1 + 2 + 2), "%d store groups on 16 slots", epilogue_slots_pinned);
}

// ---- 6. the layer table and the dataflow beside the per-layer f32 plan ----
static void check_dataflow() {
    for (uint32_t blocks = 0; blocks <= 6; blocks++) {
        const uint32_t nl = t64f_layers(blocks);
        CHECK(nl == 1 + 2 * blocks && t64f_blocks(nl) == blocks, "%u blocks: %u layers", blocks, nl);
        // per layer (Forward::per_layer_step): the stem writes a; conv1 reads a, writes t; conv2 reads t, adds a, writes y, and y becomes a;
        // the heads read a.  Every tensor is tagged with the layer that wrote it (-1: the planes, -2: nothing yet).
        int a = -2, t = -2, y = -2;
        const int planes = -1;
        int lds[2] = {-2, planes};  // the resident launch: buffer 1 first holds the expanded planes
        int out = -2;
        for (uint32_t l = 0; l < nl; l++) {
            int want_operand, want_skip = -2;
            if (l == 0) want_operand = planes, a = 0;
            else if (l & 1) want_operand = a, t = (int)l;
            else {
                want_operand = t, want_skip = a, y = (int)l;
                const int tmp = a;
                a = y, y = tmp;
            }
            const T64fLayer rl = t64f_layer(l, blocks);
            CHECK(rl.reads != rl.writes && (rl.reads | rl.writes) == 1 && rl.reads >= 0 && rl.writes >= 0, "layer %u: buffers %d -> %d", l, rl.reads, rl.writes);
            CHECK(lds[rl.reads] == want_operand, "layer %u reads the tensor of layer %d, per layer %d", l, lds[rl.reads], want_operand);
            CHECK(rl.skip == (want_skip != -2), "layer %u: skip %d", l, (int)rl.skip);
            if (rl.skip) CHECK(lds[rl.writes] == want_skip, "layer %u adds the tensor of layer %d, per layer %d", l, lds[rl.writes], want_skip);
            CHECK(rl.last == (l + 1 == nl), "layer %u of %u: last %d", l, nl, (int)rl.last);
            if (rl.last) out = (int)l;
            else lds[rl.writes] = (int)l;
            CHECK(rl.reads == (l == 0 ? T64F_LDS_M : (l & 1) ? T64F_LDS_X : T64F_LDS_M), "layer %u reads buffer %d", l, rl.reads);
        }
        CHECK(out == a && out == (int)nl - 1, "%u blocks: the heads read layer %d's rows, per layer %d's", blocks, out, a);
        (void)t, (void)y;
    }
}

// ---- 7. the workgroup-shape choice ----
static void check_shape_choice() {
    CHECK(t64f_ch(8, 64, 0) == 4 && t64f_ch(256, 64, 0) == 4 && t64f_ch(260, 64, 0) == 2 && t64f_ch(4096, 64, 0) == 2, "64-slot boards by grid size");
    CHECK(t64f_ch(8, 64, 2) == 2 && t64f_ch(4096, 64, 4) == 4 && t64f_ch(8, 64, 3) == 4, "CATTUS_T64_CH on 64-slot boards");
    CHECK(t64f_ch(2, 128, 0) == 2 && t64f_ch(2, 128, 4) == 2 && t64f_ch(2, 128, 2) == 2, "128-slot boards take 128 rows whatever is forced");
    for (const auto& sh : SHAPES) CHECK(256 % t64f_rows(sh[0]) == 0, "whole workgroups in a 256-row group");
}

int main() {
    check_lds();
    check_steps();
    check_ownership();
    check_banks();
    check_dataflow();
    check_shape_choice();
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("t64f rule ok\n");
    return 0;
}
