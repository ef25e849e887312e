// gfx950 kernels of the Cattus leaf evaluator, part 9: the SINGLE-TERM f16 conv in Winograd F(2x2, 3x3) form (K1wh, dtype f16w).
//
// The direct f16 tower (conv3x3_mfma_v2_kernel) rounds the residual stream to f16 at every layer and its LDS port is at peak; the split
// Winograd kernels (K1w ..) pay three MFMA terms per product and a (hi, lo) split of every transformed value.  This kernel runs the
// Winograd form with ONE f16 term: a transformed input is rounded once to f16, U is f16(U 2^s), and the rows between the layers stay
// plain f32 -- 2.25x fewer MFMAs than the direct kernel and a stream that is never rounded to 11 bits.
//   workgroup = 4 waves = 2 boards (32 tiles, 128 pixel rows) x NCB blocks of 32 couts (wino_f16_rule.h: wf16_ncb -- two blocks once
//       that grid still fills the CUs); wave q owns frequency ROW q (f = 4 q + l, l = 0..3) of every cout block: 4 NCB accumulators of
//       32 x 32.  Grid = (bpad / 2) x (cout / 32 NCB) behind xcd_remap's map: the cout groups of a board pair share an XCD.
//   a STEP is one 32-channel chunk = two k-steps of 16 channels, 8 NCB MFMAs per wave between two barriers.
//   U: [cout / 32][k-step x 16 + f][lane][8 f16], 1 KiB per stage; a wave loads the 8 NCB stages of a step two steps ahead, with ordinary
//       loads into a ring of WF16_UD = 3 steps of registers.  Nothing is read past a cout block's last stage.
//   d: 32-channel chunks of the 128 pixel rows, global -> registers -> LDS (4 sixteen-byte pieces per thread), K1w's chunk image; two
//       buffers: chunk c + 3 is fetched during step c and stored during step c + 1, for the transform of step c + 2.
//   V = B^T d B: a thread takes one (tile, channel pair) of each k-half per step, columns first, then rows (wf16_bt), in f32, rounds the
//       16 values ONCE to f16 and writes them into the step's V image [f][tile][k-half 0 | k-half 1 | pad]; two images: the transform of
//       step c + 1 stands beside the MFMAs of step c, one barrier per step.
//   epilogue, one cout block at a time: Z = (row q of M) A per wave, exchanged through LDS (32 KiB over V image 0, XOR-swizzled),
//       Y = A^T Z summed across the waves (wf16_at), fmaf(Y, 2^-s, bias), + skip, ReLU, cap, whole-line f32 stores; wave r finishes tile
//       row r of both boards.
// The arithmetic contract: per accumulator the k-steps ascending, one v_mfma_f32_32x32x16_f16 each; |V| <= 65504 by the cap on the rows,
// so the loop holds no clamp.  Which tiles and which cout blocks share a workgroup does not enter an element's value: a leaf's bits depend
// on the leaf alone (tests/test_f16w_gpu.py).
// A FIRST BUILD: plain loads, no hand-placed waits beside the barriers, no cross-workgroup synchronisation.  wino_f16_rule.h holds the
// grid map, the transform's items, every LDS offset, the U stage offset and the transforms (tests/test_wino_f16_rule.py runs them on
// the CPU).
#include "kernels.h"
#include "device_common.h"
#include "wino_f16_rule.h"

#include <hip/hip_ext.h>

namespace cattus {

typedef __attribute__((ext_vector_type(2))) float wf16_f32x2;
typedef __attribute__((ext_vector_type(2))) _Float16 wf16_f16x2;

template <bool HAS_RES, int NCB>
__global__ void __launch_bounds__(WF16_THREADS, 1)
    conv3x3_wino_f16_kernel(const float* __restrict__ in, const _Float16* __restrict__ wu, const float* __restrict__ bias,
                            const float* res, float* out, unsigned* __restrict__ sat, int cin, int cout) {
    // res and out may be the same rows: an element's skip value is read and its result written by one lane, the read first
    typedef _Float16 T;
    typedef Mfma<T>::frag frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);  // the wave = the frequency row it owns
    const int lane = tid & 63;

    const int ngroups = cout / (32 * NCB);
    const int logical = wf16_logical((int)blockIdx.x, (int)gridDim.x);
    const int cout0 = wf16_cout_group(logical, ngroups) * (32 * NCB);  // the workgroup's first output channel
    const int row0 = wf16_pair(logical, ngroups) * WF16_ROWS;          // first tower row of its two boards

    const int nch = cin >> 5;  // 32-channel chunks = steps
    const int nks = cin >> 4;  // k-steps

    // ---- U: the stages (k-steps 2 c and 2 c + 1, f = 4 q + l) of this wave's cout blocks ----
    const char* wq = reinterpret_cast<const char*>(wu) + lane * 16;
    auto load_u = [&](u32x4(&u)[NCB][2][4], int c) __attribute__((always_inline)) {
#pragma unroll
        for (int cb = 0; cb < NCB; cb++)
#pragma unroll
            for (int kh = 0; kh < 2; kh++)
#pragma unroll
                for (int l = 0; l < 4; l++) u[cb][kh][l] = *reinterpret_cast<const u32x4*>(wq + wf16_u_stage((cout0 >> 5) + cb, nks, 2 * c + kh, 4 * q + l));
    };
    // ---- activation chunks: global -> registers -> LDS ----
    const float* abase = in + (size_t)row0 * cin + (tid & 7) * 4;
    auto load_chunk = [&](f32x4(&regs)[4], int ch) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; i++) regs[i] = *reinterpret_cast<const f32x4*>(abase + (size_t)wf16_piece_row(tid, i) * cin + ch * 32);
    };
    auto store_chunk = [&](const f32x4(&regs)[4], int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; i++) *reinterpret_cast<f32x4*>(smem + wf16_chunk_buffer(buf) + wf16_piece_dst(tid, i)) = regs[i];
    };
    for (int i = tid; i < 2 * (WF16_ZAREA / 16); i += WF16_THREADS)  // the two zero areas
        reinterpret_cast<f32x4*>(smem + wf16_chunk_buffer(i / (WF16_ZAREA / 16)) + WF16_DZERO)[i % (WF16_ZAREA / 16)] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- the transform's items ----
    const int tt = wf16_item_tile(tid), chp = wf16_item_chp(tid);
    int poff[16];  // the 16 patch pixels' offsets inside a chunk buffer (k-half 0)
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) poff[i * 4 + j] = wf16_patch_read(tt, chp, i, j, 0);
    const int vwr = wf16_v_write(0, tt, chp, 0);
    // V of one step: chunk buffer `buf`, both halves of its 32 channels, into V image `img`
    auto transform = [&](int buf, int img) __attribute__((always_inline)) {
#pragma unroll
        for (int kh = 0; kh < 2; kh++) {
            const char* dsrc = smem + wf16_chunk_buffer(buf) + kh * WF16_DHALF;
            wf16_f32x2 dd[16];
#pragma unroll
            for (int k = 0; k < 16; k++) dd[k] = *reinterpret_cast<const wf16_f32x2*>(dsrc + poff[k]);
#pragma unroll
            for (int j = 0; j < 4; j++) {  // column j: B^T over the rows
                const wf16_f32x2 d0 = dd[j], d1 = dd[4 + j], d2 = dd[8 + j], d3 = dd[12 + j];
                wf16_bt(d0, d1, d2, d3, dd[j], dd[4 + j], dd[8 + j], dd[12 + j]);
            }
            char* vdst = smem + wf16_v_image(img) + vwr + kh * WF16_VHALF;
#pragma unroll
            for (int i = 0; i < 4; i++) {  // row i: B over the columns
                wf16_f32x2 x[4];
                wf16_bt(dd[i * 4], dd[i * 4 + 1], dd[i * 4 + 2], dd[i * 4 + 3], x[0], x[1], x[2], x[3]);
                // |x| <= 65504: a signed sum of four activations, capped at WINO_ACT_MAX = 65504 / 4 where they were written; one rounding
#pragma unroll
                for (int l = 0; l < 4; l++) *reinterpret_cast<wf16_f16x2*>(vdst + (i * 4 + l) * WF16_VF) = __builtin_convertvector(x[l], wf16_f16x2);
            }
        }
    };

    f32x16 acc[NCB][4];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++)
#pragma unroll
        for (int l = 0; l < 4; l++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[cb][l][e] = 0.0f;

    // ---- prologue: chunks 0 and 1 into their buffers, chunk 2 on its way (cin >= 128: at least four chunks), U of the first steps, V of
    // step 0 ----  The U ring: slot c % WF16_UD holds the stages of step c; a step's loads go out WF16_UD - 1 steps ahead of its MFMAs.
    constexpr int UD = WF16_UD;
    u32x4 ring[UD][NCB][2][4];
    f32x4 pend[4];
    {
        f32x4 first[4], second[4];
        load_chunk(first, 0);
        load_chunk(second, 1);
#pragma unroll
        for (int d = 0; d < UD - 1; d++) load_u(ring[d], d);
        load_chunk(pend, 2);
        store_chunk(first, 0);
        store_chunk(second, 1);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    transform(0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    const int vrd = wf16_v_read(4 * q, lane, 0);
    // One step c (ring slot SL = c % UD, parity c & 1): the 8 NCB MFMAs on V image c & 1; beside them U of step c + UD - 1 into the slot
    // step c - 1 left, chunk c + 2 (fetched during step c - 1) into the buffer chunk c was last read from in step c - 1, chunk c + 3
    // fetched, and V of step c + 1 out of the other buffer into the other image.  A barrier ends the step.
    auto step = [&](int c, auto slot_tag) __attribute__((always_inline)) {
        constexpr int SL = decltype(slot_tag)::value;
        const int par = c & 1;
        if (c + UD - 1 < nch) load_u(ring[(SL + UD - 1) % UD], c + UD - 1);
        if (c + 2 < nch) store_chunk(pend, par);
        if (c + 3 < nch) load_chunk(pend, c + 3);
        frag v[2][4];
#pragma unroll
        for (int kh = 0; kh < 2; kh++)
#pragma unroll
            for (int l = 0; l < 4; l++) v[kh][l] = *reinterpret_cast<const frag*>(smem + wf16_v_image(par) + vrd + l * WF16_VF + kh * WF16_VHALF);
        if (c + 1 < nch) transform(par ^ 1, par ^ 1);
#pragma unroll
        for (int kh = 0; kh < 2; kh++)  // k ascending: the chunk's first 16 channels, then its second
#pragma unroll
            for (int l = 0; l < 4; l++)
#pragma unroll
                for (int cb = 0; cb < NCB; cb++) Mfma<T>::mac(__builtin_bit_cast(frag, ring[SL][cb][kh][l]), v[kh][l], acc[cb][l]);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };
    static_assert(UD == 3, "the loop below walks the ring's slots by name");
    int c0 = 0;
    for (; c0 + 3 <= nch; c0 += 3) {
        step(c0, std::integral_constant<int, 0>{});
        step(c0 + 1, std::integral_constant<int, 1>{});
        step(c0 + 2, std::integral_constant<int, 2>{});
    }
    if (c0 < nch) step(c0, std::integral_constant<int, 0>{});  // the one or two steps left, in the slots they were fetched into
    if (c0 + 1 < nch) step(c0 + 1, std::integral_constant<int, 1>{});

    // ---- epilogue, cout block by cout block ----
    // (the last step's barrier: every wave has left the V images, which the exchange lies over)
    const int en = lane & 31, eh = lane >> 5;
    const int pc = lane & 7;
    float vmax = 0.0f;
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) {
        // the waves have read the exchange of the block before
        if (cb > 0) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        // Z[q][c'] = (row q of M) A, four accumulator elements (couts 8 g + 4 eh ..) at a time
#pragma unroll
        for (int g = 0; g < 4; g++) {
            f32x4 m[4];
#pragma unroll
            for (int l = 0; l < 4; l++)
#pragma unroll
                for (int e = 0; e < 4; e++) m[l][e] = acc[cb][l][g * 4 + e];
            f32x4 z0, z1;
            wf16_at(m[0], m[1], m[2], m[3], z0, z1);
            *reinterpret_cast<f32x4*>(smem + wf16_z(q, 0, en, g * 2 + eh)) = z0;
            *reinterpret_cast<f32x4*>(smem + wf16_z(q, 1, en, g * 2 + eh)) = z1;
        }
        // wave q finishes tile row q of both boards: 32 pixel rows x 32 couts, lane = (pixel k * 8 + (lane >> 3), couts 4 pc .. 4 pc + 3)
        const int cb0 = cout0 + cb * 32;
        const f32x4 bias4 = *reinterpret_cast<const f32x4*>(bias + cb0 + pc * 4);
        const f32x4 ds4 = *reinterpret_cast<const f32x4*>(bias + cout + cb0 + pc * 4);
        size_t orow[4];
        f32x4 skip[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            orow[k] = ((size_t)row0 + wf16_out_row(q, wf16_out_pixel(lane, k))) * (size_t)cout + cb0 + pc * 4;
            if (HAS_RES) skip[k] = *reinterpret_cast<const f32x4*>(res + orow[k]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int p = wf16_out_pixel(lane, k);
            const int rp = k & 1, cp = p & 1;  // output row parity inside the tile (p >> 3 & 1), output column parity
            const int tile = wf16_out_tile(q, p);
            const f32x4 za = *reinterpret_cast<const f32x4*>(smem + wf16_z(rp + 0, cp, tile, pc));
            const f32x4 zc = *reinterpret_cast<const f32x4*>(smem + wf16_z(rp + 1, cp, tile, pc));
            const f32x4 zd = *reinterpret_cast<const f32x4*>(smem + wf16_z(rp + 2, cp, tile, pc));
            const f32x4 a = rp == 0 ? za + zc + zd : za - zc - zd;  // wf16_at's two rows: Y[0] = Z0 + Z1 + Z2, Y[1] = Z1 - Z2 - Z3
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
    }
    if (vmax >= WINO_ACT_MAX) atomicAdd(sat, 1u);  // an activation reached the cap somewhere in this thread's share
}

// The four instances, f(kernel, HAS_RES, NCB); each takes WF16_LDS_TOTAL bytes of dynamic LDS.
template <class F>
static void for_each_wino_f16(F&& f) {
    each_bool([&](auto r) {
        f(&conv3x3_wino_f16_kernel<decltype(r)::value, 1>, r, 1);
        f(&conv3x3_wino_f16_kernel<decltype(r)::value, 2>, r, 2);
    });
}

bool wino_f16_supported(uint32_t bpad, uint32_t cin, uint32_t cout, uint32_t S) {
    return S == 8 && bpad % WF16_BOARDS == 0 && cin % 64 == 0 && cout % 64 == 0 && cin >= 128 && cout >= 128;
}

void launch_conv3x3_wino_f16(const float* in, const void* wu, const float* bias, const float* res, float* out, uint32_t bpad, uint32_t cin,
                             uint32_t cout, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop, unsigned* sat) {
    typedef _Float16 H;
    if (!wino_f16_supported(bpad, cin, cout, 8)) {
        fprintf(stderr, "cattus: launch_conv3x3_wino_f16: unsupported shape (bpad %u, cin %u, cout %u)\n", bpad, cin, cout);
        abort();
    }
    const int ncb = wf16_ncb(bpad, cout);
    const dim3 grid(wf16_grid(bpad, cout, ncb));
    for_each_wino_f16([&](auto kernel, auto r, int n) {
        if (r == (res != nullptr) && n == ncb)
            hipExtLaunchKernelGGL(kernel, grid, dim3(WF16_THREADS), WF16_LDS_TOTAL, st, ev_start, ev_stop, 0, in, (const H*)wu, bias, res, out, sat, (int)cin,
                                  (int)cout);
    });
}

hipError_t prepare_wino_f16() {
    hipError_t err = hipSuccess;
    for_each_wino_f16([&](auto kernel, auto, int) { lds_opt_in(err, kernel, WF16_LDS_TOTAL); });
    return err;
}

}  // namespace cattus
