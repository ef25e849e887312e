// gfx950 kernels of the Cattus leaf evaluator, part 5: the split-precision 3x3 conv in Winograd F(4x4, 3x3) form (K1f4).
//
// F(2x2, 3x3) (kernels_wino.hip, kernels_wino4.hip) issues 16 products per 2x2 outputs and input channel: 64 per 4x4 outputs.
// F(4x4, 3x3) needs 36: 0.75 MFMA terms per multiply-add instead of 1.333, and 1.78x fewer transformed inputs to split into (hi, lo).
// What it does to the result was measured before this was written (scripts/winograd_gate_f4.py -> profiles/winograd_gate_f4.json).
// The form is opt-in (tower_form WINOGRAD_F4), a FIRST BUILD: correct, one launch per layer, no cross-workgroup synchronisation, no
// hand-placed loads -- winof4_rule.h holds the matrices, the transforms' operation order, the geometry, the cap and the U index.
//
// Between its layers a tower in this form keeps the PLAIN F32 rows [row][channel] of the F(2x2) tower (64 slots per 8x8 board), so
// the stem (direct kernel, CONV_OUT_F32 | CONV_WINOF4_IN), the heads and every observer are the same.  The f16 range: a transformed
// input is a signed sum of 36 activations with weights whose absolute values add up to 100 at most, so activations are capped at
// WINOF4_ACT_MAX = 655 where they are written (this kernel's epilogue, the stem) and counted there; the transform needs no clamp.
//   workgroup = 4 waves = 8 boards (32 tiles of 4x4 outputs) x 32 couts; grid = ceil(bpad / 8) x cout / 32 (256 at batch 256, 256
//       filters); bpad is a multiple of 4: the second four boards of the last board group may lie beyond it and are then neither
//       read nor written
//   wave w holds the nine frequencies 9 w .. 9 w + 8 of the (32 couts x 32 tiles) block: 144 accumulator registers
//   a k-step = 16 input channels:
//     d: the k-step's 16 channels of the 512 pixel rows, global -> registers -> LDS (64-byte rows, the row index XOR-swizzled by the
//         tile so that the tiles of a board read different banks), two buffers: k-step s + 1 is fetched while s is transformed
//     V = B^T d B: thread = (tile, channel pair) reads its 6x6 patch (off-board pixels are zero), transforms it in f32
//         (winof4_input_2d), splits the 36 values into (hi, lo) and writes them to the V image [f][tile][16 ch hi | 16 ch lo | pad]
//     U: [cout / 32][k-step x 36 + f][hi | lo][lane][8 f16] (winof4_frag_index), a wave's 18 fragments requested ahead of the transform
//     27 MFMAs per wave: U_lo V_hi, U_hi V_lo, U_hi V_hi per frequency, three frequencies interleaved
//   LDS: V image 92,160 B + 2 x 32,768 B = 157,696 B
//   epilogue: the 36 accumulators of a (tile, cout) meet through LDS ([f][tile][8 x 4 couts], 16-byte slots XOR-swizzled by the tile:
//       147,456 B over the loop's buffers), thread = (tile, 4 couts): Y = A^T M A (winof4_output_2d), fma(y, 2^-s, bias), + skip, ReLU,
//       cap, 16-byte stores -- eight lanes write a pixel's whole 128 bytes.
#include "kernels.h"
#include "device_common.h"

#include <hip/hip_ext.h>

namespace cattus {

constexpr int F4_VP = 80;                       // V image row: 16 ch hi (32 B) | 16 ch lo (32 B) | 16 B pad
constexpr int F4_VF = 32 * F4_VP;               // one frequency: 32 tiles
constexpr int F4_VIMG = WINOF4_FREQ * F4_VF;    // 92,160 B
constexpr int F4_ROWS = 512;                    // pixel rows of a workgroup: 8 boards x 64 slots
constexpr int F4_DBUF = F4_ROWS * 64;           // a k-step's 16 f32 channels of them: 32,768 B
constexpr int F4_LDS_LOOP = F4_VIMG + 2 * F4_DBUF;
constexpr int F4_LDS_EX = WINOF4_FREQ * 32 * 32 * 4;  // the epilogue's exchange
constexpr int F4_LDS_TOTAL = F4_LDS_LOOP > F4_LDS_EX ? F4_LDS_LOOP : F4_LDS_EX;
static_assert(F4_LDS_TOTAL == 157696 && F4_LDS_TOTAL <= 160 * 1024, "LDS budget");
constexpr int F4_NP = F4_DBUF / 16 / 256;       // 16-byte pieces per thread and k-step: 8

typedef __attribute__((ext_vector_type(2))) float f4_f32x2;
typedef __attribute__((ext_vector_type(2))) _Float16 f4_f16x2;

// Where pixel row r (board * 64 + y * 8 + x) of a chunk buffer lives: 64-byte rows, r's low two bits XORed with (bit 2 of x, bit 2
// of y) -- the four tiles of a board, whose patch pixels lie 4 columns / 4 rows apart (multiples of 256 B), land on four bank groups.
__device__ __forceinline__ int f4_row_slot(int r) { return r ^ (((r >> 2) & 1) | (((r >> 5) & 1) << 1)); }

// The workgroup's barrier between phases that hand LDS contents over: this wave's LDS accesses are complete, then everybody meets.
// __syncthreads() would also wait for the global loads in flight (s_waitcnt vmcnt(0)) -- the next k-step's rows and, behind the
// transform's barrier, U fragments the MFMAs further down do not need yet; the compiler waits for each of those where it is used.
__device__ __forceinline__ void f4_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <bool HAS_RES>
__global__ void __launch_bounds__(256, 1)
    conv3x3_winof4_kernel(const float* __restrict__ in, const _Float16* __restrict__ wu, const float* __restrict__ bias, const float* res,
                          float* out, unsigned* __restrict__ sat, int cin, int cout, int bpad) {
    // res and out may be the same rows (a residual block's output over its skip rows): an element's skip value is read and its
    // result written by one lane, the read first
    typedef _Float16 T;
    typedef Mfma<T>::frag frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;

    const int ncb = cout >> 5;
    const int logical = xcd_remap(blockIdx.x, gridDim.x);  // one XCD: all cout blocks of a range of boards
    const int cb = logical % ncb, cout0 = cb * 32;
    const int board0 = (logical / ncb) * 8;
    const int nboards = min(8, bpad - board0);  // 8, or 4 in the last board group
    const size_t row0 = (size_t)board0 * 64;
    const int nks = cin >> 4;

    char* const vimg = smem;
    char* const dbuf = smem + F4_VIMG;

    // ---- a k-step's rows: piece i of thread t = 16 bytes (idx & 3) of pixel row idx >> 2, idx = 256 i + t ----
    auto load_chunk = [&](f32x4(&regs)[F4_NP], int ks) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < F4_NP; i++) {
            const int idx = i * 256 + tid, r = idx >> 2, piece = idx & 3;
            regs[i] = (r >> 6) < nboards ? *reinterpret_cast<const f32x4*>(in + (row0 + r) * (size_t)cin + ks * 16 + piece * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_chunk = [&](const f32x4(&regs)[F4_NP], int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < F4_NP; i++) {
            const int idx = i * 256 + tid, r = idx >> 2, piece = idx & 3;
            *reinterpret_cast<f32x4*>(dbuf + buf * F4_DBUF + f4_row_slot(r) * 64 + piece * 16) = regs[i];
        }
    };

    // ---- the transform's item: tile tt = 4 board + 2 ty + tx, channel pair chp of the k-step's eight ----
    const int tt = tid >> 3, chp = tid & 7;
    const int tb = tt >> 2, tty = (tt >> 1) & 1, ttx = tt & 1;
    int poff[36];  // byte offset of patch pixel (a, b) inside a chunk buffer, -1 off the board
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = 0; b < 6; b++) {
            const int y = winof4_patch_y(tty, a), x = winof4_patch_x(ttx, b);
            poff[a * 6 + b] = winof4_on_board(y, x) ? f4_row_slot(tb * 64 + y * 8 + x) * 64 + chp * 8 : -1;
        }
    const int vwr = tt * F4_VP + chp * 4;  // the item's hi pair inside a frequency's block (the lo pair 32 B further)
    auto transform = [&](int buf) __attribute__((always_inline)) {
        const char* src = dbuf + buf * F4_DBUF;
        f4_f32x2 d[6][6], v[6][6];
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = 0; b < 6; b++) {
                const int o = poff[a * 6 + b];
                d[a][b] = o >= 0 ? *reinterpret_cast<const f4_f32x2*>(src + o) : f4_f32x2{0.f, 0.f};
            }
        winof4_input_2d(d, v);
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int l = 0; l < 6; l++) {
                // |v| <= 100 x 655 = 65,500: whoever wrote the activations capped them at WINOF4_ACT_MAX
                const f4_f32x2 x = v[i][l];
                const f4_f16x2 hi = __builtin_convertvector(x, f4_f16x2);
                const f4_f16x2 lo = __builtin_convertvector(x - __builtin_convertvector(hi, f4_f32x2), f4_f16x2);  // the difference is exact in f32
                char* q = vimg + (i * 6 + l) * F4_VF + vwr;
                *reinterpret_cast<f4_f16x2*>(q) = hi;
                *reinterpret_cast<f4_f16x2*>(q + 32) = lo;
            }
    };

    f32x16 acc[WINOF4_WAVE_FREQ];
#pragma unroll
    for (int j = 0; j < WINOF4_WAVE_FREQ; j++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[j][e] = 0.0f;

    // this wave's U: stage (k-step s, frequency 9 wave + j) of cout block cb, this lane's 16 bytes of the hi fragment (lo: 512 f16 further)
    const _Float16* const wlane = wu + ((size_t)cb * nks * WINOF4_FREQ + wave * WINOF4_WAVE_FREQ) * WINOF4_STAGE_ELEMS + lane * 8;
    const int vrd = (lane & 31) * F4_VP + (lane >> 5) * 16;  // this lane's V fragment inside a frequency's block: tile, channels 8 h .. 8 h + 7

    {
        f32x4 first[F4_NP];
        load_chunk(first, 0);
        store_chunk(first, 0);
    }
    f4_lds_barrier();
    for (int s = 0; s < nks; s++) {
        // requested ahead of the transform: U of this k-step, the rows of the next
        frag uh[WINOF4_WAVE_FREQ], ul[WINOF4_WAVE_FREQ];
        const _Float16* const wk = wlane + (size_t)s * WINOF4_FREQ * WINOF4_STAGE_ELEMS;
#pragma unroll
        for (int j = 0; j < WINOF4_WAVE_FREQ; j++) {
            uh[j] = *reinterpret_cast<const frag*>(wk + (size_t)j * WINOF4_STAGE_ELEMS);
            ul[j] = *reinterpret_cast<const frag*>(wk + (size_t)j * WINOF4_STAGE_ELEMS + 512);
        }
        f32x4 next[F4_NP];
        const bool more = s + 1 < nks;
        if (more) load_chunk(next, s + 1);
        transform(s & 1);
        // the other buffer was last read by the transform of k-step s - 1: every wave has passed two barriers since
        if (more) store_chunk(next, (s + 1) & 1);
        f4_lds_barrier();  // the V image is complete
#pragma unroll
        for (int j0 = 0; j0 < WINOF4_WAVE_FREQ; j0 += 3) {
            frag vh[3], vl[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const char* p = vimg + (wave * WINOF4_WAVE_FREQ + j0 + j) * F4_VF + vrd;
                vh[j] = *reinterpret_cast<const frag*>(p);
                vl[j] = *reinterpret_cast<const frag*>(p + 32);
            }
            // per accumulator the order of the F(2x2) kernels: U_lo V_hi, U_hi V_lo, U_hi V_hi
#pragma unroll
            for (int j = 0; j < 3; j++) Mfma<T>::mac(ul[j0 + j], vh[j], acc[j0 + j]);
#pragma unroll
            for (int j = 0; j < 3; j++) Mfma<T>::mac(uh[j0 + j], vl[j], acc[j0 + j]);
#pragma unroll
            for (int j = 0; j < 3; j++) Mfma<T>::mac(uh[j0 + j], vh[j], acc[j0 + j]);
        }
        f4_lds_barrier();  // every wave has left the V image (and, behind the last k-step, the loop's LDS altogether)
    }

    // ---- epilogue ----
    // accumulator element e of lane (tile n = lane & 31, half eh): cout 8 (e >> 2) + 4 eh + (e & 3) of tile n -> exchange slot
    // [f][tile][quad (2 g + eh) ^ (tile & 7)] of four couts
    {
        const int n = lane & 31, eh = lane >> 5;
#pragma unroll
        for (int j = 0; j < WINOF4_WAVE_FREQ; j++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int f = wave * WINOF4_WAVE_FREQ + j;
                const f32x4 m4 = {acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]};
                *reinterpret_cast<f32x4*>(smem + ((size_t)((f * 32 + n) * 8 + ((2 * g + eh) ^ (n & 7))) << 4)) = m4;
            }
    }
    f4_lds_barrier();
    const int et = tid >> 3, cq = tid & 7;  // tile, quad of couts: eight lanes cover a pixel's 128 bytes
    const int eb = et >> 2, ety = (et >> 1) & 1, etx = et & 1;
    if (eb >= nboards) return;  // a board beyond bpad: nothing of it is written (no barrier follows)
    f32x4 m[6][6], y[4][4];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int l = 0; l < 6; l++) m[i][l] = *reinterpret_cast<const f32x4*>(smem + ((size_t)(((i * 6 + l) * 32 + et) * 8 + (cq ^ (et & 7))) << 4));
    winof4_output_2d(m, y);
    const f32x4 bias4 = *reinterpret_cast<const f32x4*>(bias + cout0 + cq * 4);
    const f32x4 ds4 = *reinterpret_cast<const f32x4*>(bias + cout + cout0 + cq * 4);
    float vmax = 0.0f;
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const size_t at = (row0 + eb * 64 + winof4_out_y(ety, p) * 8 + winof4_out_x(etx, q)) * (size_t)cout + cout0 + cq * 4;
            f32x4 sk4 = {0.f, 0.f, 0.f, 0.f};
            if (HAS_RES) sk4 = *reinterpret_cast<const f32x4*>(res + at);
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float x = __builtin_fmaf(y[p][q][j], ds4[j], bias4[j]);  // the inverse weight scale is a power of two: the fma rounds once
                if (HAS_RES) x = x + sk4[j];
                x = x > 0.0f ? x : 0.0f;
                v[j] = x < WINOF4_ACT_MAX ? x : WINOF4_ACT_MAX;  // the next layer's transform relies on it
            }
            vmax = fmaxf(fmaxf(vmax, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
            *reinterpret_cast<f32x4*>(out + at) = v;
        }
    if (vmax >= WINOF4_ACT_MAX) atomicAdd(sat, 1u);  // an activation reached the cap somewhere in this thread's share
}

bool winof4_supported(uint32_t bpad, uint32_t cin, uint32_t cout, uint32_t S) {
    return S == 8 && cin >= 128 && cin % 64 == 0 && cout >= 128 && cout % 64 == 0 && bpad >= 4 && bpad % 4 == 0;
}

// Both instances, f(kernel, HAS_RES); either takes F4_LDS_TOTAL bytes of dynamic LDS.
template <class F>
static void for_each_winof4(F&& f) {
    each_bool([&](auto r) { f(&conv3x3_winof4_kernel<decltype(r)::value>, r); });
}

void launch_conv3x3_winof4(const float* in, const void* wu, const float* bias, const float* res, float* out, uint32_t bpad, uint32_t cin,
                           uint32_t cout, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop, unsigned* sat) {
    typedef _Float16 H;
    const dim3 grid(((bpad + 7) / 8) * (cout / 32));
    for_each_winof4([&](auto kernel, auto r) {
        if (r == (res != nullptr))
            hipExtLaunchKernelGGL(kernel, grid, dim3(256), F4_LDS_TOTAL, st, ev_start, ev_stop, 0, in, (const H*)wu, bias, res, out, sat, (int)cin, (int)cout,
                                  (int)bpad);
    });
}

hipError_t prepare_winof4() {
    hipError_t err = hipSuccess;
    for_each_winof4([&](auto kernel, auto) { lds_opt_in(err, kernel, F4_LDS_TOTAL); });
    return err;
}

}  // namespace cattus
