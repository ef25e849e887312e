// The Winograd F(4x4, 3x3) form of the split-precision conv (kernels_winof4.hip), as far as it can be wrong without a GPU: the three
// matrices, the f32 transforms in the operation order the kernel runs them in (it calls these functions), the tile geometry on an
// 8x8 board, the activation cap and where an element of U lives.  Plain C++: host and device, no HIP call (tests/test_winof4_rule.py).
//
//   Y = A^T [ (G g G^T) . (B^T d B) ] A   for a 6x6 patch d, a 3x3 kernel g and 4x4 outputs Y: Lavin's matrices on the interpolation
//   points 0, +-1, +-2 and infinity.  36 products per 16 outputs and input channel where F(2x2, 3x3) needs 64 and the direct form 144.
//
// Every 1-D transform below is written in differences and sums whose only multiplications are by 2, 4 and 8: those products are
// exact, so a compiler that contracts a multiply-add into an fma and one that does not give the same bits -- host, device and the
// numpy restatement of the test agree bit for bit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WINOF4_HD __host__ __device__ inline
#else
#define WINOF4_HD inline
#endif

namespace cattus {

constexpr int WINOF4_FREQ = 36;  // frequencies f = 6 i + l of a tile: row i, column l of the 6x6 transformed patch

// clang-format off
constexpr float WINOF4_BT[6][6] = {{4,  0, -5,  0, 1, 0},
                                   {0, -4, -4,  1, 1, 0},
                                   {0,  4, -4, -1, 1, 0},
                                   {0, -2, -1,  2, 1, 0},
                                   {0,  2, -1, -2, 1, 0},
                                   {0,  4,  0, -5, 0, 1}};
constexpr double WINOF4_G[6][3] = {{ 1.0 / 4,   0,        0      },
                                   {-1.0 / 6,  -1.0 / 6, -1.0 / 6},
                                   {-1.0 / 6,   1.0 / 6, -1.0 / 6},
                                   { 1.0 / 24,  1.0 / 12, 1.0 / 6},
                                   { 1.0 / 24, -1.0 / 12, 1.0 / 6},
                                   { 0,         0,        1      }};
constexpr float WINOF4_AT[4][6] = {{1, 1,  1, 1,  1, 0},
                                   {0, 1, -1, 2, -2, 0},
                                   {0, 1,  1, 4,  4, 0},
                                   {0, 1, -1, 8, -8, 1}};
// clang-format on

// ---- the activation cap ----
// A transformed input is sum_ij B^T[i][a] d[a][b] B^T[l][b]: at most (largest absolute row sum of B^T)^2 times the largest |d|.  The
// row sums are 10, 10, 10, 6, 6, 10, so activations capped at 655 where they are written (the kernel's epilogue, the stem's
// CONV_WINOF4_IN) keep every |V| <= 65,500 -- inside the f16 range, and the kernel's transform carries neither clamp nor range check.
constexpr float winof4_abs(float x) { return x < 0 ? -x : x; }
constexpr float winof4_row_sum(int i) {
    float s = 0;
    for (int a = 0; a < 6; a++) s += winof4_abs(WINOF4_BT[i][a]);
    return s;
}
constexpr float winof4_max_row_sum() {
    float m = 0;
    for (int i = 0; i < 6; i++) m = winof4_row_sum(i) > m ? winof4_row_sum(i) : m;
    return m;
}
constexpr float WINOF4_ACT_MAX = 655.0f;
static_assert(winof4_max_row_sum() == 10.0f, "the largest absolute row sum of B^T");
static_assert(winof4_max_row_sum() * winof4_max_row_sum() * WINOF4_ACT_MAX <= 65504.0f, "a transformed input of capped activations stays an f16 number");
static_assert(winof4_max_row_sum() * winof4_max_row_sum() * (WINOF4_ACT_MAX + 1.0f) > 65504.0f, "and the cap is the largest whole number that does");

// ---- the 1-D transforms, f32, in this operation order ----
// t = B^T d:  t0 = 4 (d0 - d2) + (d4 - d2)     t1 = (d3 + d4) - 4 (d1 + d2)     t2 = 4 (d1 - d2) + (d4 - d3)
//             t3 = 2 (d3 - d1) + (d4 - d2)     t4 = (d4 - d2) - 2 (d3 - d1)     t5 = 4 (d1 - d3) + (d5 - d3)
template <class T>
WINOF4_HD void winof4_bt_1d(const T (&d)[6], T (&t)[6]) {
    const T a02 = d[0] - d[2], a42 = d[4] - d[2], s12 = d[1] + d[2], s34 = d[3] + d[4], a12 = d[1] - d[2], a43 = d[4] - d[3];
    const T a31 = d[3] - d[1], a13 = d[1] - d[3], a53 = d[5] - d[3];
    t[0] = 4.0f * a02 + a42;
    t[1] = s34 - 4.0f * s12;
    t[2] = 4.0f * a12 + a43;
    t[3] = 2.0f * a31 + a42;
    t[4] = a42 - 2.0f * a31;
    t[5] = 4.0f * a13 + a53;
}
// y = A^T m:  y0 = ((m1 + m2) + (m3 + m4)) + m0     y1 = (m1 - m2) + 2 (m3 - m4)
//             y2 = (m1 + m2) + 4 (m3 + m4)          y3 = ((m1 - m2) + 8 (m3 - m4)) + m5
template <class T>
WINOF4_HD void winof4_at_1d(const T (&m)[6], T (&y)[4]) {
    const T s12 = m[1] + m[2], s34 = m[3] + m[4], a12 = m[1] - m[2], a34 = m[3] - m[4];
    y[0] = (s12 + s34) + m[0];
    y[1] = a12 + 2.0f * a34;
    y[2] = s12 + 4.0f * s34;
    y[3] = (a12 + 8.0f * a34) + m[5];
}
// ---- the 2-D transforms: down the columns first (rows of the result), then along the rows ----
// V = B^T d B: column b of d through winof4_bt_1d gives column b of T = B^T d; row i of T through winof4_bt_1d gives row i of V.
template <class T>
WINOF4_HD void winof4_input_2d(const T (&d)[6][6], T (&v)[6][6]) {
    T t[6][6];
    for (int b = 0; b < 6; b++) {
        const T col[6] = {d[0][b], d[1][b], d[2][b], d[3][b], d[4][b], d[5][b]};
        T r[6];
        winof4_bt_1d(col, r);
        for (int i = 0; i < 6; i++) t[i][b] = r[i];
    }
    for (int i = 0; i < 6; i++) winof4_bt_1d(t[i], v[i]);
}
// Y = A^T M A: column l of M through winof4_at_1d gives column l of Z = A^T M (4 x 6); row p of Z through it gives row p of Y.
template <class T>
WINOF4_HD void winof4_output_2d(const T (&m)[6][6], T (&y)[4][4]) {
    T z[4][6];
    for (int l = 0; l < 6; l++) {
        const T col[6] = {m[0][l], m[1][l], m[2][l], m[3][l], m[4][l], m[5][l]};
        T r[4];
        winof4_at_1d(col, r);
        for (int p = 0; p < 4; p++) z[p][l] = r[p];
    }
    for (int p = 0; p < 4; p++) winof4_at_1d(z[p], y[p]);
}

// ---- tile geometry on an 8x8 board ----
// A board is 2 x 2 tiles; tile (ty, tx) writes pixels (4 ty .. 4 ty + 3, 4 tx .. 4 tx + 3) and reads the 6 x 6 patch whose pixel (a, b)
// is board pixel (4 ty - 1 + a, 4 tx - 1 + b); a patch pixel off the board reads as zero (the conv's padding).
constexpr int WINOF4_TILES = 4;  // per board
WINOF4_HD int winof4_out_y(int ty, int p) { return 4 * ty + p; }
WINOF4_HD int winof4_out_x(int tx, int q) { return 4 * tx + q; }
WINOF4_HD int winof4_patch_y(int ty, int a) { return 4 * ty - 1 + a; }
WINOF4_HD int winof4_patch_x(int tx, int b) { return 4 * tx - 1 + b; }
WINOF4_HD bool winof4_on_board(int y, int x) { return (unsigned)y < 8u && (unsigned)x < 8u; }

// ---- frequencies over the four waves of a workgroup: wave w holds f = 9 w .. 9 w + 8 ----
constexpr int WINOF4_WAVE_FREQ = 9;
WINOF4_HD int winof4_wave_of(int f) { return f / WINOF4_WAVE_FREQ; }
WINOF4_HD int winof4_wave_slot(int f) { return f % WINOF4_WAVE_FREQ; }

// ---- U in the kernel's order: [cout / 32][k-step x 36 + f][hi | lo][lane][8 f16] ----
// A k-step is 16 input channels; the MFMA's A operand of (cout block, k-step, frequency): lane = 32 (k-half) + cout % 32 holds its
// channels 8 (k-half) .. + 7.  Element index of U (frequency f, output channel co, input channel ci, part 0 = hi / 1 = lo); the
// kernel reads exactly the cout_pad x cin_pad x 36 x 2 elements and nothing behind them.
constexpr size_t WINOF4_STAGE_ELEMS = 2 * 64 * 8;  // one (cout block, k-step, frequency): hi fragment, lo fragment = 2,048 B
WINOF4_HD size_t winof4_frag_index(uint32_t f, uint32_t co, uint32_t ci, uint32_t part, uint32_t cin_pad) {
    const size_t stages_per_block = (size_t)(cin_pad / 16) * WINOF4_FREQ, stage = (size_t)(ci >> 4) * WINOF4_FREQ + f;
    const uint32_t lane = ((ci >> 3) & 1) * 32 + (co & 31);
    return ((((size_t)(co >> 5) * stages_per_block + stage) * 2 + part) * 64 + lane) * 8 + (ci & 7);
}
WINOF4_HD size_t winof4_u_elems(uint32_t cout_pad, uint32_t cin_pad) { return (size_t)WINOF4_FREQ * cout_pad * cin_pad * 2; }

}  // namespace cattus
