// gfx950 kernels of the Cattus leaf evaluator, part 7: the Winograd F(2x2, 3x3) split conv on a SMALL tile (K1w4s), for short batches.
//
// conv3x3_wino4_kernel / tower_wino4_kernel (kernels_wino4.hip) give a workgroup 4 boards x 64 couts: a batch of 64 leaves is 64
// workgroups on 256 CUs, and a workgroup takes as long however few there are.  This kernel computes THE SAME LAYER, bit for bit, on a
// tile a quarter of that size: 256 workgroups at 64 leaves, 64 at 16.
//   workgroup = 4 waves = 2 boards (32 tiles, 128 pixel rows) x 32 couts; wave q owns frequency ROW q (f = 4 q + l, l = 0..3): four
//       32 x 32 accumulators.  Grid = (bpad / 2) x (cout / 32) behind xcd_remap's map: the cout blocks of a board pair share an XCD.
//   U: K1w's buffer and fragment order ([cout / 32][k-step x 16 + f][hi | lo][lane][8 f16]); a wave loads the 4 stages of its frequency
//       row three k-steps ahead, with ordinary loads into a ring of four k-steps of registers.  Nothing is read past the cout block's
//       last stage.
//   d: 32-channel chunks of the 128 pixel rows, global -> registers -> LDS (4 sixteen-byte pieces per thread), K1w's chunk image; two
//       buffers: chunk c + 2 is fetched during k-step 2 c and stored during k-step 2 c + 2.
//   V = B^T d B: K1w's transform -- a thread takes one (tile, channel pair) per k-step, rows first, then columns, in f32, splits the 16
//       values (hi = f16(v), lo = f16(v - hi)) and writes them into the k-step's V image [f][tile][16 hi | 16 lo | pad]; two images: the
//       transform of k-step s + 1 stands beside the 12 MFMAs of k-step s, one barrier per k-step.
//   epilogue: Z = (row q of M) A per wave, exchanged through LDS (32 KiB over V image 0, XOR-swizzled), Y = A^T Z summed across the waves,
//       * 2^-s + bias, + skip, ReLU, cap, whole-line f32 stores; wave r finishes tile row r of both boards.
// The bit contract with K1w / K1w4: per accumulator the k-steps ascending over the same 16 channels in the same lane assignment, within a
// k-step U_lo V_hi, U_hi V_lo, U_hi V_hi; V, Z and Y combined in K1w's order; fmaf(y, 2^-s, bias), + skip, ReLU, cap.  Which tiles share
// an MFMA does not enter an element's value (tests/test_short_batches_gpu.py).
// A FIRST BUILD: plain loads, no hand-placed waits beside the barriers, no cross-workgroup synchronisation.  wino4s_rule.h holds the
// grid map, the transform's items and every LDS offset (tests/test_wino4s_rule.py runs them on the CPU).
#include "kernels.h"
#include "device_common.h"
#include "wino4s_rule.h"

#include <hip/hip_ext.h>

namespace cattus {

static_assert(W4S_PP == SP, "the chunk image's pixel pitch is the split tower's LDS row pitch");

constexpr int W4S_UD = 4;  // k-steps of U in registers: the one being multiplied and three on their way (4 x 32 registers)

typedef __attribute__((ext_vector_type(2))) float w4s_f32x2;
typedef __attribute__((ext_vector_type(2))) _Float16 w4s_f16x2;

template <bool HAS_RES>
__global__ void __launch_bounds__(W4S_THREADS, 1)
    conv3x3_wino4s_kernel(const float* __restrict__ in, const _Float16* __restrict__ wu, const float* __restrict__ bias,
                          const float* res, float* out, unsigned* __restrict__ sat, int cin, int cout) {
    // res and out may be the same rows: an element's skip value is read and its result written by one lane, the read first
    typedef _Float16 T;
    typedef Mfma<T>::frag frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);  // the wave = the frequency row it owns
    const int lane = tid & 63;

    const int ncb = cout >> 5;
    const int logical = wino4s_logical((int)blockIdx.x, (int)gridDim.x);
    const int cout0 = wino4s_cout_block(logical, ncb) * W4S_COUTS;  // the workgroup's 32 output channels
    const int row0 = wino4s_pair(logical, ncb) * W4S_ROWS;          // first tower row of its two boards

    const int nch = cin >> 5;  // 32-channel chunks
    const int nks = cin >> 4;  // k-steps

    // ---- U: the four stages (k-step s, f = 4 q + l) of this wave, [hi | lo] fragments ----
    const char* wq = reinterpret_cast<const char*>(wu) + ((size_t)(cout0 >> 5) * nks * 16 + 4 * q) * SW_STAGE + lane * 16;
    auto load_u = [&](u32x4(&u)[4][2], int s) __attribute__((always_inline)) {
#pragma unroll
        for (int l = 0; l < 4; l++) {
            const char* p = wq + ((size_t)s * 16 + l) * SW_STAGE;
            u[l][0] = *reinterpret_cast<const u32x4*>(p);
            u[l][1] = *reinterpret_cast<const u32x4*>(p + 1024);
        }
    };
    // ---- activation chunks: global -> registers -> LDS ----
    const float* abase = in + (size_t)row0 * cin + (tid & 7) * 4;
    auto load_chunk = [&](f32x4(&regs)[4], int ch) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; i++) regs[i] = *reinterpret_cast<const f32x4*>(abase + (size_t)wino4s_piece_row(tid, i) * cin + ch * 32);
    };
    auto store_chunk = [&](const f32x4(&regs)[4], int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; i++) *reinterpret_cast<f32x4*>(smem + wino4s_chunk_buffer(buf) + wino4s_piece_dst(tid, i)) = regs[i];
    };
    for (int i = tid; i < 2 * (W4S_ZAREA / 16); i += W4S_THREADS)  // the two zero areas
        reinterpret_cast<f32x4*>(smem + wino4s_chunk_buffer(i / (W4S_ZAREA / 16)) + W4S_DZERO)[i % (W4S_ZAREA / 16)] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- the transform's item ----
    const int tt = wino4s_item_tile(tid), chp = wino4s_item_chp(tid);
    int poff[16];  // the 16 patch pixels' offsets inside a chunk buffer (half 0)
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) poff[i * 4 + j] = wino4s_patch_read(tt, chp, i, j, 0);
    const int vwr = wino4s_v_write(0, tt, chp, 0);
    // V of one k-step: chunk buffer `buf`, half kp of its 32 channels, into V image `img`
    auto transform = [&](int buf, int kp, int img) __attribute__((always_inline)) {
        const char* dsrc = smem + wino4s_chunk_buffer(buf) + kp * 64;
        w4s_f32x2 dd[16];
#pragma unroll
        for (int k = 0; k < 16; k++) dd[k] = *reinterpret_cast<const w4s_f32x2*>(dsrc + poff[k]);
#pragma unroll
        for (int j = 0; j < 4; j++) {  // column j: B^T over the rows
            const w4s_f32x2 d0 = dd[j], d1 = dd[4 + j], d2 = dd[8 + j], d3 = dd[12 + j];
            dd[j] = d0 - d2, dd[4 + j] = d1 + d2, dd[8 + j] = d2 - d1, dd[12 + j] = d1 - d3;
        }
        char* vdst = smem + wino4s_v_image(img) + vwr;
#pragma unroll
        for (int i = 0; i < 4; i++) {  // row i: B over the columns
            const w4s_f32x2 t0 = dd[i * 4], t1 = dd[i * 4 + 1], t2 = dd[i * 4 + 2], t3 = dd[i * 4 + 3];
#pragma unroll
            for (int l = 0; l < 4; l++) {
                const w4s_f32x2 x = l == 0 ? t0 - t2 : l == 1 ? t1 + t2 : l == 2 ? t2 - t1 : t1 - t3;
                // |x| <= 65504: a signed sum of four activations, capped at WINO_ACT_MAX = 65504 / 4 where they were written
                const w4s_f16x2 hi = __builtin_convertvector(x, w4s_f16x2);
                // lo = f16(x - hi): the difference is exact in f32 (hi is x rounded to 11 bits), the conversion rounds it once
                const w4s_f16x2 lo = __builtin_convertvector(x - __builtin_convertvector(hi, w4s_f32x2), w4s_f16x2);
                char* p = vdst + (i * 4 + l) * W4S_VF;
                *reinterpret_cast<w4s_f16x2*>(p) = hi;
                *reinterpret_cast<w4s_f16x2*>(p + 32) = lo;
            }
        }
    };

    f32x16 acc[4];
#pragma unroll
    for (int l = 0; l < 4; l++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[l][e] = 0.0f;

    // ---- prologue: chunks 0 and 1 into their buffers (cin >= 128: at least four chunks), U of the first k-steps, V of k-step 0 ----
    // The U ring: slot s % W4S_UD holds the four stages of k-step s; a k-step's loads go out W4S_UD - 1 k-steps ahead of its MFMAs (one
    // k-step ahead they cost the loop the whole latency of a load, k-step after k-step: the first build's 18 us per 256 -> 256 layer)
    constexpr int UD = W4S_UD;
    u32x4 ring[UD][4][2];
    f32x4 pend[4];
    {
        f32x4 first[4];
        load_chunk(first, 0);
        load_chunk(pend, 1);
#pragma unroll
        for (int d = 0; d < UD - 1; d++) load_u(ring[d], d);  // cin >= 128: at least eight k-steps
        store_chunk(first, 0);
        store_chunk(pend, 1);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    transform(0, 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    const int vrd = wino4s_v_read(4 * q, lane, 0);
    // One k-step s (ring slot SL = s % UD, parity PAR = s & 1, chunk c = s >> 1): the 12 MFMAs on V image PAR; beside them U of k-step
    // s + UD - 1 into the slot k-step s - 1 left, V of k-step s + 1 into the other image, and in the even k-steps the chunk traffic -- chunk
    // c + 1, fetched two k-steps ago, goes into the buffer chunk c - 1 was last read from in k-step 2 c - 2, and chunk c + 2 is fetched.
    // A barrier ends the k-step.
    auto kstep = [&](int s, auto slot_tag) __attribute__((always_inline)) {
        constexpr int SL = decltype(slot_tag)::value, PAR = SL & 1;
        if (s + UD - 1 < nks) load_u(ring[(SL + UD - 1) % UD], s + UD - 1);
        if (PAR == 0) {
            const int c = s >> 1;
            if (c >= 1 && c + 1 < nch) store_chunk(pend, (c + 1) & 1);
            if (c + 2 < nch) load_chunk(pend, c + 2);
        }
        frag vh[4], vl[4];
#pragma unroll
        for (int l = 0; l < 4; l++) {
            vh[l] = *reinterpret_cast<const frag*>(smem + wino4s_v_image(PAR) + vrd + l * W4S_VF);
            vl[l] = *reinterpret_cast<const frag*>(smem + wino4s_v_image(PAR) + vrd + l * W4S_VF + 32);
        }
        if (s + 1 < nks) transform(((s + 1) >> 1) & 1, PAR ^ 1, PAR ^ 1);
#pragma unroll
        for (int l = 0; l < 4; l++) {
            const frag uh = __builtin_bit_cast(frag, ring[SL][l][0]), ul = __builtin_bit_cast(frag, ring[SL][l][1]);
            Mfma<T>::mac(ul, vh[l], acc[l]);
            Mfma<T>::mac(uh, vl[l], acc[l]);
            Mfma<T>::mac(uh, vh[l], acc[l]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };
    static_assert(UD == 4, "the loop below walks the ring's slots by name");
    int s0 = 0;
    for (; s0 + 4 <= nks; s0 += 4) {
        kstep(s0, std::integral_constant<int, 0>{});
        kstep(s0 + 1, std::integral_constant<int, 1>{});
        kstep(s0 + 2, std::integral_constant<int, 2>{});
        kstep(s0 + 3, std::integral_constant<int, 3>{});
    }
    if (s0 < nks) {  // cin % 64 == 32: two k-steps left, in the slots they were fetched into
        kstep(s0, std::integral_constant<int, 0>{});
        kstep(s0 + 1, std::integral_constant<int, 1>{});
    }

    // ---- epilogue ----
    // (the last k-step's barrier: every wave has left the V images, which the exchange lies over)
    const int en = lane & 31, eh = lane >> 5;
    // Z[q][c'] = (row q of M) A: Z[.][0] = M[q][0] + M[q][1] + M[q][2], Z[.][1] = M[q][1] - M[q][2] - M[q][3] (K1w's order), four accumulator
    // elements (couts 8 g + 4 eh ..) at a time
#pragma unroll
    for (int g = 0; g < 4; g++) {
        f32x4 m[4];
#pragma unroll
        for (int l = 0; l < 4; l++)
#pragma unroll
            for (int e = 0; e < 4; e++) m[l][e] = acc[l][g * 4 + e];
        const f32x4 z0 = m[0] + m[1] + m[2], z1 = m[1] - m[2] - m[3];
        *reinterpret_cast<f32x4*>(smem + wino4s_z(q, 0, en, g * 2 + eh)) = z0;
        *reinterpret_cast<f32x4*>(smem + wino4s_z(q, 1, en, g * 2 + eh)) = z1;
    }
    // wave q finishes tile row q of both boards: 32 pixel rows x 32 couts, lane = (pixel k * 8 + (lane >> 3), couts 4 pc .. 4 pc + 3)
    const int pc = lane & 7;
    const f32x4 bias4 = *reinterpret_cast<const f32x4*>(bias + cout0 + pc * 4);
    const f32x4 ds4 = *reinterpret_cast<const f32x4*>(bias + cout + cout0 + pc * 4);
    size_t orow[4];
    f32x4 skip[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        orow[k] = ((size_t)row0 + wino4s_out_row(q, wino4s_out_pixel(lane, k))) * (size_t)cout + cout0 + pc * 4;
        if (HAS_RES) skip[k] = *reinterpret_cast<const f32x4*>(res + orow[k]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    float vmax = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int p = wino4s_out_pixel(lane, k);
        const int rp = k & 1, cp = p & 1;  // output row parity inside the tile (p >> 3 & 1), output column parity
        const int tile = wino4s_out_tile(q, p);
        const f32x4 za = *reinterpret_cast<const f32x4*>(smem + wino4s_z(rp + 0, cp, tile, pc));
        const f32x4 zc = *reinterpret_cast<const f32x4*>(smem + wino4s_z(rp + 1, cp, tile, pc));
        const f32x4 zd = *reinterpret_cast<const f32x4*>(smem + wino4s_z(rp + 2, cp, tile, pc));
        const f32x4 a = rp == 0 ? za + zc + zd : za - zc - zd;  // Y[0] = Z0 + Z1 + Z2, Y[1] = Z1 - Z2 - Z3
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float x = __builtin_fmaf(a[j], ds4[j], bias4[j]);  // the inverse weight scale is a power of two: the fma rounds once
            if (HAS_RES) x = x + skip[k][j];
            x = x > 0.0f ? x : 0.0f;
            v[j] = x < WINO_ACT_MAX ? x : WINO_ACT_MAX;  // the next layer's transform relies on it
        }
        vmax = fmaxf(fmaxf(vmax, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
        *reinterpret_cast<f32x4*>(out + orow[k]) = v;
    }
    if (vmax >= WINO_ACT_MAX) atomicAdd(sat, 1u);  // an activation reached the cap somewhere in this thread's share
}

// Both instances, f(kernel, HAS_RES); either takes W4S_LDS_TOTAL bytes of dynamic LDS.
template <class F>
static void for_each_wino4s(F&& f) {
    each_bool([&](auto r) { f(&conv3x3_wino4s_kernel<decltype(r)::value>, r); });
}

void launch_conv3x3_wino4s(const float* in, const void* wu, const float* bias, const float* res, float* out, uint32_t bpad, uint32_t cin,
                           uint32_t cout, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop, unsigned* sat) {
    typedef _Float16 H;
    const dim3 grid(wino4s_grid(bpad, cout));
    for_each_wino4s([&](auto kernel, auto r) {
        if (r == (res != nullptr))
            hipExtLaunchKernelGGL(kernel, grid, dim3(W4S_THREADS), W4S_LDS_TOTAL, st, ev_start, ev_stop, 0, in, (const H*)wu, bias, res, out, sat, (int)cin,
                                  (int)cout);
    });
}

hipError_t prepare_wino4s() {
    hipError_t err = hipSuccess;
    for_each_wino4s([&](auto kernel, auto) { lds_opt_in(err, kernel, W4S_LDS_TOTAL); });
    return err;
}

}  // namespace cattus
