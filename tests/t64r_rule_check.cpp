// Stand-alone program around cattus_amd/csrc/t64r_rule.h (tests/test_t64r_rule.py builds it plain and under sanitizers): the ownership
// map of tower64_stream_kernel's consumer lanes as a bijection onto the workgroup's rows x 64 channels, the LDS address it gives against
// the address a conv's fragment read takes the same element from, the f32 row index of the last layer's store, the two LDS buffers
// through towers of 0 .. 6 blocks, and the resident plan (stream in registers, two LDS buffers) walked beside f16r_rule.h's per-layer
// plan (three buffers in memory), tensor for tensor.  Prints what fails and "t64r rule ok" when nothing does.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "t64r_rule.h"

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

// ---- 1. the ownership map ----
static void check_ownership() {
    CHECK(t64r_stream_regs(4) == 16 && t64r_stream_regs(2) == 32, "stream registers per lane: %d, %d", t64r_stream_regs(4), t64r_stream_regs(2));
    const int shapes[][2] = {{4, 64}, {2, 64}, {2, 128}};  // (CH, pixel slots per board): one board, two boards, one 128-slot board per workgroup
    for (const auto& sh : shapes) {
        const int ch = sh[0], slots = sh[1], rows = t64r_rows(ch), npb = t64r_npb(ch);
        CHECK(rows == 256 / ch && rows % slots == 0, "CH %d: %d rows, %d slots", ch, rows, slots);
        const size_t row0 = (size_t)3 * rows;  // the fourth workgroup of a launch
        std::vector<int> owners((size_t)rows * 64, 0);       // per (row, channel)
        std::vector<int> lds_owner((size_t)rows * 64, -1);   // per 2-byte element of an LDS buffer: the (row, channel) written there
        std::vector<int> out_owner((size_t)rows * 64, -1);   // per f32 of the workgroup's output rows
        int seen = 0;
        for (int wave = 0; wave < 4; wave++)
            for (int lane = 0; lane < 64; lane++)
                for (int cb = 0; cb < T64R_CB; cb++)
                    for (int pb = 0; pb < npb; pb++)
                        for (int e = 0; e < 16; e++) {
                            const T64rOwn o = t64r_own(ch, wave, lane, cb, pb, e);
                            CHECK(o.row >= 0 && o.row < rows && o.channel >= 0 && o.channel < 64, "CH %d wave %d lane %d pb %d e %d: (%d, %d)", ch, wave, lane, pb, e, o.row, o.channel);
                            if (o.row < 0 || o.row >= rows || o.channel < 0 || o.channel >= 64) return;
                            owners[(size_t)o.row * 64 + o.channel]++;
                            seen++;
                            // the board and pixel slot of the row: a lane's 32 pixels of a block lie in one board
                            const size_t grow = row0 + (size_t)o.row;
                            const T64rOwn first = t64r_own(ch, wave, lane & 32, cb, pb, e);
                            CHECK(grow / slots == (row0 + (size_t)first.row) / slots, "CH %d wave %d pb %d: a pixel block crosses a board", ch, wave, pb);
                            // where it is stored: inside the buffer, every element once, a group of four elements in 8 consecutive bytes / 4 floats
                            const int at = t64r_lds_offset(o);
                            CHECK(at >= 0 && at + 2 <= rows * 128 && at % 2 == 0, "CH %d: LDS offset %d of %d", ch, at, rows * 128);
                            if (at < 0 || at + 2 > rows * 128) return;
                            CHECK(lds_owner[at / 2] == -1, "CH %d: LDS byte %d written twice", ch, at);
                            lds_owner[at / 2] = o.row * 64 + o.channel;
                            const size_t oi = t64r_out_index(row0, o);
                            CHECK(oi >= row0 * 64 && oi < (row0 + rows) * 64, "CH %d: output index %zu", ch, oi);
                            if (oi < row0 * 64 || oi >= (row0 + rows) * 64) return;
                            CHECK(out_owner[oi - row0 * 64] == -1, "CH %d: output %zu written twice", ch, oi);
                            out_owner[oi - row0 * 64] = o.row * 64 + o.channel;
                            CHECK(oi == (row0 + (size_t)o.row) * 64 + (size_t)o.channel, "plain f32 rows [row][64]");
                            const T64rOwn g = t64r_own(ch, wave, lane, cb, pb, e & ~3);
                            CHECK(g.row == o.row && g.channel + (e & 3) == o.channel && g.channel % 4 == 0, "four elements: four consecutive channels of one row");
                            CHECK(t64r_lds_offset(g) % 8 == 0 && t64r_lds_offset(g) + 2 * (e & 3) == at, "four elements: one 8-byte store");
                            CHECK(t64r_out_index(row0, g) % 4 == 0 && t64r_out_index(row0, g) + (size_t)(e & 3) == oi, "four elements: one 16-byte store");
                        }
        CHECK(seen == rows * 64, "CH %d: %d elements for %d", ch, seen, rows * 64);
        for (size_t i = 0; i < owners.size(); i++) CHECK(owners[i] == 1, "CH %d: (row %zu, channel %zu) has %d owners", ch, i / 64, i % 64, owners[i]);
        // the fragment read of the next conv: lane half h, k-step ks of pixel row `row` takes 8 f16 = channels (ks * 2 + h) * 8 .. + 7 from
        // row * 128 + (((h ^ ((row >> 1) & 7)) << 4) ^ (ks << 5))  (kernels.hip: swz ^ (ks << 5)) -- the element written there is that one
        for (int row = 0; row < rows; row++)
            for (int h = 0; h < 2; h++)
                for (int ks = 0; ks < 4; ks++)
                    for (int j = 0; j < 8; j++) {
                        const int at = row * 128 + (((h ^ ((row >> 1) & 7)) << 4) ^ (ks << 5)) + j * 2;
                        CHECK(lds_owner[at / 2] == row * 64 + (ks * 2 + h) * 8 + j, "CH %d: the conv reads (row %d, channel %d) where (row %d, channel %d) was written", ch, row,
                              (ks * 2 + h) * 8 + j, lds_owner[at / 2] / 64, lds_owner[at / 2] % 64);
                    }
    }
}

// ---- 2. and 3.: the LDS buffers, the layer table, and the dataflow beside the per-layer plan ----
// A tensor is named by the layer that wrote it (-1: the planes, -2: nothing yet) and by what it is.
enum Kind { NOTHING, PLANES, STREAM, COPY, MIDDLE };
struct Held {
    Kind kind;
    int by;
};
static bool same(Held a, Held b) { return a.kind == b.kind && a.by == b.by; }

static void check_plan() {
    for (uint32_t blocks = 0; blocks <= 6; blocks++) {
        const uint32_t nl = t64r_layers(blocks);
        CHECK(nl == 1 + 2 * blocks && nl == f16r_layers(blocks) && t64r_blocks(nl) == blocks, "%u blocks: %u layers", blocks, nl);
        Held mem[4] = {{NOTHING, -2}, {NOTHING, -2}, {NOTHING, -2}, {PLANES, -1}};  // the per-layer plan: F16R_BUF_A, _T, _Y, _X0
        Held lds[2] = {{NOTHING, -2}, {PLANES, -1}};                              // the resident plan: buffer 0, buffer 1 (the expanded planes)
        Held sreg = {NOTHING, -2};                                                // and the lane's stream registers
        int copies = 0, counted_layers = 0;
        for (uint32_t l = 0; l < nl; l++) {
            const F16rLayer fl = f16r_layer(l, blocks);
            const T64rLayer rl = t64r_layer(l, blocks);
            CHECK(rl.reads == t64r_reads(l) && rl.writes == t64r_writes(l) && rl.reads != rl.writes && (rl.reads | rl.writes) == 1, "layer %u: one buffer read, the other written", l);
            CHECK(rl.stream == f16r_stream_layer(l) && rl.last == f16r_is_last(l, blocks) && rl.last == (l + 1 == nl), "layer %u: roles", l);
            CHECK(rl.skip == (fl.adds != F16R_NONE) && (!rl.skip || rl.stream), "layer %u: the skip flag", l);
            CHECK(!rl.last || rl.stream, "the last layer is a stream layer");
            // operand: the same tensor
            CHECK(same(lds[rl.reads], mem[fl.reads]), "layer %u reads (%d by %d) from LDS, (%d by %d) per layer", l, lds[rl.reads].kind, lds[rl.reads].by, mem[fl.reads].kind,
                  mem[fl.reads].by);
            // skip: the same tensor, from the registers
            if (rl.skip) CHECK(fl.adds == F16R_S && sreg.kind == STREAM && same(sreg, mem[fl.adds]), "layer %u adds the stream written by layer %d, per layer by %d", l, sreg.by, mem[fl.adds].by);
            // destination
            if (rl.stream) {
                CHECK(fl.writes == F16R_S, "layer %u: a stream layer writes the stream", l);
                sreg = Held{STREAM, (int)l}, mem[fl.writes] = Held{STREAM, (int)l};
                CHECK(rl.last == (fl.writes_copy == F16R_NONE), "layer %u: a copy from every stream layer but the last", l);
                if (!rl.last) {
                    CHECK(rl.writes == T64R_LDS_A && fl.writes_copy == F16R_A, "layer %u: the copy goes to buffer 0", l);
                    CHECK(t64r_layer(l + 1, blocks).reads == rl.writes && !t64r_layer(l + 1, blocks).stream, "layer %u: its copy lands where the next conv1 reads", l);
                    lds[rl.writes] = Held{COPY, (int)l}, mem[fl.writes_copy] = Held{COPY, (int)l};
                    copies++, counted_layers++;
                }
                // (the last layer writes no LDS at all: the buffer keeps what it held)
            } else {
                CHECK(fl.writes == F16R_M && fl.writes_copy == F16R_NONE && rl.writes == T64R_LDS_M && !rl.skip && !rl.last, "layer %u: conv1 writes the middle to buffer 1", l);
                lds[rl.writes] = Held{MIDDLE, (int)l}, mem[fl.writes] = Held{MIDDLE, (int)l};
                counted_layers++;
            }
        }
        CHECK(same(sreg, mem[f16r_head_input()]) && sreg.kind == STREAM && sreg.by == (int)nl - 1, "%u blocks: the heads read the last layer's stream", blocks);
        CHECK(copies == (int)blocks && counted_layers == 2 * (int)blocks, "%u blocks: %d copies, %d counting layers", blocks, copies, counted_layers);
    }
}

int main() {
    check_ownership();
    check_plan();
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("t64r rule ok\n");
    return 0;
}
