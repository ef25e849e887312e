// One layer of conv3x3_wino_f32_kernel (dtype f32w) restated on the CPU with std::fmaf, in exactly the order cattus_amd/csrc/wino_f32_rule.h
// states: U through the device's own builder (weight_layout.h: wino_transform, wino_u_f32) and index, V = B^T d B by wf32_bt down the
// columns then along the rows, every accumulator a chain of fmaf from 0 over wf32_chain_channel's channel order, Z and Y by wf32_at,
// wf32_finish behind them.  Build with -ffp-contract=off.  tests/test_f32w_gpu.py holds the kernel to this program's output bit for bit;
// tests/test_wino_f32_rule.py holds the program to a float64 direct convolution.
//
//   wino_f32_layer_ref BOARDS CIN COUT in.f32 weights.f32 bias.f32 skip.f32|- out.f32
//     in      [BOARDS * 64][CIN] f32 rows (row = board * 64 + y * 8 + x)      weights  folded, [9][COUT][CIN], tap = ky * 3 + kx
//     bias    [COUT]                                                          skip     rows like out, or "-" for a layer without one
//     out     [BOARDS * 64][COUT] f32 rows
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "weight_layout.h"
#include "wino_f32_rule.h"

using namespace cattus;

static std::vector<float> read_floats(const char* path, size_t n) {
    std::vector<float> v(n);
    FILE* f = fopen(path, "rb");
    if (!f || fread(v.data(), 4, n, f) != n || fgetc(f) != EOF) {
        fprintf(stderr, "wino_f32_layer_ref: %s does not hold exactly %zu floats\n", path, n);
        exit(2);
    }
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 9) {
        fprintf(stderr, "usage: wino_f32_layer_ref BOARDS CIN COUT in weights bias skip|- out\n");
        return 2;
    }
    const uint32_t B = (uint32_t)atoi(argv[1]), CIN = (uint32_t)atoi(argv[2]), COUT = (uint32_t)atoi(argv[3]);
    if (B < 1 || CIN < 8 || CIN % 8 || COUT < 1) {
        fprintf(stderr, "wino_f32_layer_ref: boards >= 1, cin a multiple of 8, cout >= 1\n");
        return 2;
    }
    const std::vector<float> in = read_floats(argv[4], (size_t)B * 64 * CIN);
    Folded f;
    f.w = read_floats(argv[5], (size_t)9 * COUT * CIN);
    f.b = read_floats(argv[6], COUT);
    const bool has_skip = std::string(argv[7]) != "-";
    const std::vector<float> skip = has_skip ? read_floats(argv[7], (size_t)B * 64 * COUT) : std::vector<float>();
    const ConvShape s{COUT, CIN, COUT, CIN};
    std::vector<int> shift;  // not used by this dtype: no scale
    const std::vector<float> wu = wino_u_f32(wino_transform(f, s, &shift), s);

    std::vector<float> out((size_t)B * 64 * COUT);
    std::vector<float> V((size_t)16 * CIN);  // [frequency][channel] of one tile
    for (uint32_t b = 0; b < B; b++)
        for (int ty = 0; ty < 4; ty++)
            for (int tx = 0; tx < 4; tx++) {
                for (uint32_t ci = 0; ci < CIN; ci++) {
                    float d[4][4], t[4][4];
                    for (int i = 0; i < 4; i++)
                        for (int j = 0; j < 4; j++) {
                            const int y = 2 * ty - 1 + i, x = 2 * tx - 1 + j;
                            d[i][j] = y >= 0 && y < 8 && x >= 0 && x < 8 ? in[((size_t)b * 64 + y * 8 + x) * CIN + ci] : 0.0f;
                        }
                    for (int j = 0; j < 4; j++) wf32_bt(d[0][j], d[1][j], d[2][j], d[3][j], t[0][j], t[1][j], t[2][j], t[3][j]);
                    for (int i = 0; i < 4; i++) {
                        float x[4];
                        wf32_bt(t[i][0], t[i][1], t[i][2], t[i][3], x[0], x[1], x[2], x[3]);
                        for (int l = 0; l < 4; l++) V[(size_t)(i * 4 + l) * CIN + ci] = x[l];
                    }
                }
                for (uint32_t co = 0; co < COUT; co++) {
                    float m[4][4];
                    for (int fq = 0; fq < 16; fq++) {
                        float acc = 0.0f;
                        for (uint32_t n = 0; n < CIN; n++) {
                            const uint32_t ci = (uint32_t)wf32_chain_channel((int)n);
                            acc = std::fmaf(wu[wino_f32_frag_index((uint32_t)fq, co, ci, CIN)], V[(size_t)fq * CIN + ci], acc);
                        }
                        m[fq >> 2][fq & 3] = acc;
                    }
                    float z[4][2], y[2][2];
                    for (int i = 0; i < 4; i++) wf32_at(m[i][0], m[i][1], m[i][2], m[i][3], z[i][0], z[i][1]);
                    for (int c = 0; c < 2; c++) wf32_at(z[0][c], z[1][c], z[2][c], z[3][c], y[0][c], y[1][c]);
                    for (int r = 0; r < 2; r++)
                        for (int c = 0; c < 2; c++) {
                            const size_t at = ((size_t)b * 64 + (2 * ty + r) * 8 + 2 * tx + c) * COUT + co;
                            out[at] = wf32_finish(y[r][c], f.b[co], has_skip, has_skip ? skip[at] : 0.0f);
                        }
                }
            }
    FILE* o = fopen(argv[8], "wb");
    if (!o || fwrite(out.data(), 4, out.size(), o) != out.size() || fclose(o) != 0) {
        fprintf(stderr, "wino_f32_layer_ref: cannot write %s\n", argv[8]);
        return 2;
    }
    return 0;
}
