// gfx950 kernels of the Cattus leaf evaluator, part 10: the F32-OPERAND conv in Winograd F(2x2, 3x3) form (K1wf, dtype f32w).
//
// The exact f32 tower (conv3x3_mfma_v2_kernel<float>) is bound by its f32 MFMAs: 0.87 of the 157 TF the matrix cores give f32 operands.
// This kernel runs the same operand width in the Winograd form -- 2.25x fewer MFMAs -- on the plain f32 rows the f32 stem writes and
// the f32 heads read: U = f32(G g G^T) without a scale, V = B^T d B in f32, one v_mfma_f32_32x32x2_f32 chain per product, no cap and
// no saturation counter.  K1wh's plan (kernels_wino_f16.hip) with a step of half a chunk:
//   workgroup = 4 waves = 2 boards (32 tiles, 128 pixel rows) x NCB blocks of 32 couts (wino_f32_rule.h: wf32_ncb -- two blocks once
//       that grid still fills the CUs); wave q owns frequency ROW q (f = 4 q + l, l = 0..3) of every cout block: 4 NCB accumulators of
//       32 x 32.  Grid = (bpad / 2) x (cout / 32 NCB) behind xcd_remap's map: the cout groups of a board pair share an XCD.
//   a STEP is 16 channels = two 8-channel groups: 8 NCB Mfma<float>::mac = 32 NCB MFMAs of 64 cycles per wave between two barriers.
//   U: [cout / 32][group x 16 + f][lane][4 f32], 1 KiB per stage; a wave loads the 8 NCB stages of a step one step ahead, with ordinary
//       loads into a ring of WF32_UD = 2 steps of registers.  Nothing is read past a cout block's last stage.
//   d: 32-channel chunks of the 128 pixel rows, global -> registers -> LDS (4 sixteen-byte pieces per thread), K1w's chunk image; two
//       buffers: chunk c + 2 is fetched during step 2 c and stored during step 2 c + 1 over chunk c, whose last transform ran in step 2 c.
//   V = B^T d B: a thread takes one (tile, channel pair) of the step's 16 channels, columns first, then rows (wf32_bt), in f32, and writes
//       the 16 values into the step's V image [f][tile][group 0 | group 1 | pad]; two images: the transform of step s + 1 stands beside
//       the MFMAs of step s, one barrier per step.
//   epilogue, one cout block at a time: Z = (row q of M) A per wave, exchanged through LDS (32 KiB over V image 0, XOR-swizzled),
//       Y = A^T Z summed across the waves (wf32_at's order), wf32_finish (+ bias, + skip, ReLU), whole-line f32 stores; wave r finishes
//       tile row r of both boards.
// The arithmetic contract (wino_f32_rule.h; tests/wino_f32_layer_ref.cpp restates it with std::fmaf and tests/test_f32w_gpu.py holds the
// kernel to it bit for bit): per accumulator the 8-channel groups ascending, Mfma<float>::mac's four MFMAs each.  Which tiles and which
// cout blocks share a workgroup does not enter an element's value: a leaf's bits depend on the leaf alone.
// A FIRST BUILD: plain loads, no hand-placed waits beside the barriers, no cross-workgroup synchronisation.  The next step's transform
// stands in front of the step's MFMAs in program order and the compiler leaves it there (behind a branch of its own), so a wave's
// transform and its MFMAs run one after the other, not interleaved; DESIGN.md, K1wf, says what a second pass would do about it.
#include "kernels.h"
#include "device_common.h"
#include "wino_f32_rule.h"

#include <hip/hip_ext.h>

namespace cattus {

typedef __attribute__((ext_vector_type(2))) float wf32_f32x2;

template <bool HAS_RES, int NCB>
__global__ void __launch_bounds__(WF32_THREADS, 1)
    conv3x3_wino_f32_kernel(const float* __restrict__ in, const float* __restrict__ wu, const float* __restrict__ bias, const float* res, float* out,
                            int cin, int cout) {
    // res and out may be the same rows: an element's skip value is read and its result written by one lane, the read first
    typedef Mfma<float>::frag frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);  // the wave = the frequency row it owns
    const int lane = tid & 63;

    const int ngroups = cout / (32 * NCB);
    const int logical = wf32_logical((int)blockIdx.x, (int)gridDim.x);
    const int cout0 = wf32_cout_group(logical, ngroups) * (32 * NCB);  // the workgroup's first output channel
    const int row0 = wf32_pair(logical, ngroups) * WF32_ROWS;          // first tower row of its two boards

    const int nch = cin >> 5;            // 32-channel chunks
    const int nsteps = cin / WF32_STEP;  // steps of 16 channels: two per chunk (cin % 64 == 0: an even number)
    const int ngr = cin >> 3;            // 8-channel groups

    // ---- U: the stages (groups 2 s and 2 s + 1, f = 4 q + l) of this wave's cout blocks ----
    const char* wq = reinterpret_cast<const char*>(wu) + lane * 16;
    auto load_u = [&](frag(&u)[NCB][2][4], int s) __attribute__((always_inline)) {
#pragma unroll
        for (int cb = 0; cb < NCB; cb++)
#pragma unroll
            for (int gh = 0; gh < 2; gh++)
#pragma unroll
                for (int l = 0; l < 4; l++) u[cb][gh][l] = *reinterpret_cast<const frag*>(wq + wf32_u_stage((cout0 >> 5) + cb, ngr, 2 * s + gh, 4 * q + l));
    };
    // ---- activation chunks: global -> registers -> LDS ----
    const float* abase = in + (size_t)row0 * cin + (tid & 7) * 4;
    auto load_chunk = [&](f32x4(&regs)[4], int ch) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; i++) regs[i] = *reinterpret_cast<const f32x4*>(abase + (size_t)wf32_piece_row(tid, i) * cin + ch * 32);
    };
    auto store_chunk = [&](const f32x4(&regs)[4], int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; i++) *reinterpret_cast<f32x4*>(smem + wf32_chunk_buffer(buf) + wf32_piece_dst(tid, i)) = regs[i];
    };
    for (int i = tid; i < 2 * (WF32_ZAREA / 16); i += WF32_THREADS)  // the two zero areas
        reinterpret_cast<f32x4*>(smem + wf32_chunk_buffer(i / (WF32_ZAREA / 16)) + WF32_DZERO)[i % (WF32_ZAREA / 16)] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- the transform's item ----
    const int tt = wf32_item_tile(tid), chp = wf32_item_chp(tid);
    int poff[16];  // the 16 patch pixels' offsets inside a chunk buffer (half 0)
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) poff[i * 4 + j] = wf32_patch_read(tt, chp, i, j, 0);
    const int vwr = wf32_v_write(0, tt, chp);
    // V of one step: half `half` of the chunk in buffer `buf`, into V image `img`
    auto transform = [&](int buf, int half, int img) __attribute__((always_inline)) {
        const char* dsrc = smem + wf32_chunk_buffer(buf) + half * WF32_DHALF;
        wf32_f32x2 dd[16];
#pragma unroll
        for (int k = 0; k < 16; k++) dd[k] = *reinterpret_cast<const wf32_f32x2*>(dsrc + poff[k]);
#pragma unroll
        for (int j = 0; j < 4; j++) {  // column j: B^T over the rows
            const wf32_f32x2 d0 = dd[j], d1 = dd[4 + j], d2 = dd[8 + j], d3 = dd[12 + j];
            wf32_bt(d0, d1, d2, d3, dd[j], dd[4 + j], dd[8 + j], dd[12 + j]);
        }
        char* vdst = smem + wf32_v_image(img) + vwr;
#pragma unroll
        for (int i = 0; i < 4; i++) {  // row i: B over the columns
            wf32_f32x2 x[4];
            wf32_bt(dd[i * 4], dd[i * 4 + 1], dd[i * 4 + 2], dd[i * 4 + 3], x[0], x[1], x[2], x[3]);
#pragma unroll
            for (int l = 0; l < 4; l++) *reinterpret_cast<wf32_f32x2*>(vdst + (i * 4 + l) * WF32_VF) = x[l];
        }
    };

    f32x16 acc[NCB][4];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++)
#pragma unroll
        for (int l = 0; l < 4; l++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[cb][l][e] = 0.0f;

    // ---- prologue: chunks 0 and 1 into their buffers (cin >= 128: at least four chunks), U of step 0, V of step 0 ----
    // The U ring: slot s % WF32_UD holds the stages of step s; a step's loads go out one step ahead of its MFMAs.
    static_assert(WF32_UD == 2, "the loop below walks the ring's two slots by the step's parity");
    frag ring[WF32_UD][NCB][2][4];
    f32x4 pend[4];
    {
        f32x4 second[4];
        load_chunk(pend, 0);
        load_chunk(second, 1);
        load_u(ring[0], 0);
        store_chunk(pend, 0);
        store_chunk(second, 1);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    transform(0, 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    const int vrd = wf32_v_read(4 * q, lane, 0);
    // One step s of parity PAR = s & 1 (ring slot and V image PAR; chunk c = s >> 1, its half PAR): the 32 NCB MFMAs on V image PAR; beside
    // them U of step s + 1 into the other slot; on an even step chunk c + 2 fetched, on an odd one stored over chunk c (last read by the
    // transform that ran in step s - 1); and V of step s + 1 into the other image.  A barrier ends the step.
    // The guards state one invariant: a step prepares only what a later step consumes.  The layer's last step (s + 1 == nsteps) loads no
    // U and transforms nothing; the steps of the last two chunks (c + 2 >= nch) fetch and store no chunk -- `pend` is written on an even
    // step and stored on the odd step behind it, which has the same c and so the same condition.
    auto step =[&](int s, auto par_tag) __attribute__((always_inline)) {
        constexpr int PAR = decltype(par_tag)::value;
        const int c = s >> 1;
        if (s + 1 < nsteps) load_u(ring[PAR ^ 1], s + 1);
        if constexpr (PAR == 0) {
            if (c + 2 < nch) load_chunk(pend, c + 2);
        } else {
            if (c + 2 < nch) store_chunk(pend, c & 1);
        }
        frag v[2][4];
#pragma unroll
        for (int gh = 0; gh < 2; gh++)
#pragma unroll
            for (int l = 0; l < 4; l++) v[gh][l] = *reinterpret_cast<const frag*>(smem + wf32_v_image(PAR) + vrd + l * WF32_VF + gh * WF32_VGROUP);
        if (s + 1 < nsteps) transform(((s + 1) >> 1) & 1, PAR ^ 1, PAR ^ 1);
#pragma unroll
        for (int gh = 0; gh < 2; gh++)  // the groups ascending: the step's first 8 channels, then its second
#pragma unroll
            for (int l = 0; l < 4; l++)
#pragma unroll
                for (int cb = 0; cb < NCB; cb++) Mfma<float>::mac(ring[PAR][cb][gh][l], v[gh][l], acc[cb][l]);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };
    for (int s = 0; s < nsteps; s += 2) {
        step(s, std::integral_constant<int, 0>{});
        step(s + 1, std::integral_constant<int, 1>{});
    }

    // ---- epilogue, cout block by cout block ----
    // (the last step's barrier: every wave has left the V images, which the exchange lies over)
    const int en = lane & 31, eh = lane >> 5;
    const int pc = lane & 7;
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
            wf32_at(m[0], m[1], m[2], m[3], z0, z1);
            *reinterpret_cast<f32x4*>(smem + wf32_z(q, 0, en, g * 2 + eh)) = z0;
            *reinterpret_cast<f32x4*>(smem + wf32_z(q, 1, en, g * 2 + eh)) = z1;
        }
        // wave q finishes tile row q of both boards: 32 pixel rows x 32 couts, lane = (pixel k * 8 + (lane >> 3), couts 4 pc .. 4 pc + 3)
        const int cb0 = cout0 + cb * 32;
        const f32x4 bias4 = *reinterpret_cast<const f32x4*>(bias + cb0 + pc * 4);
        size_t orow[4];
        f32x4 skip[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            orow[k] = ((size_t)row0 + wf32_out_row(q, wf32_out_pixel(lane, k))) * (size_t)cout + cb0 + pc * 4;
            if (HAS_RES) skip[k] = *reinterpret_cast<const f32x4*>(res + orow[k]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int p = wf32_out_pixel(lane, k);
            const int rp = k & 1, cp = p & 1;  // output row parity inside the tile (p >> 3 & 1), output column parity
            const int tile = wf32_out_tile(q, p);
            const f32x4 za = *reinterpret_cast<const f32x4*>(smem + wf32_z(rp + 0, cp, tile, pc));
            const f32x4 zc = *reinterpret_cast<const f32x4*>(smem + wf32_z(rp + 1, cp, tile, pc));
            const f32x4 zd = *reinterpret_cast<const f32x4*>(smem + wf32_z(rp + 2, cp, tile, pc));
            const f32x4 a = rp == 0 ? za + zc + zd : za - zc - zd;  // wf32_at's two rows: Y[0] = Z0 + Z1 + Z2, Y[1] = Z1 - Z2 - Z3
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = wf32_finish(a[j], bias4[j], HAS_RES, HAS_RES ? skip[k][j] : 0.0f);
            *reinterpret_cast<f32x4*>(out + orow[k]) = v;
        }
    }
}

// The four instances, f(kernel, HAS_RES, NCB); each takes WF32_LDS_TOTAL bytes of dynamic LDS.
template <class F>
static void for_each_wino_f32(F&& f) {
    each_bool([&](auto r) {
        f(&conv3x3_wino_f32_kernel<decltype(r)::value, 1>, r, 1);
        f(&conv3x3_wino_f32_kernel<decltype(r)::value, 2>, r, 2);
    });
}

bool wino_f32_supported(uint32_t bpad, uint32_t cin, uint32_t cout, uint32_t S) {
    return S == 8 && bpad % WF32_BOARDS == 0 && cin % 64 == 0 && cout % 64 == 0 && cin >= 128 && cout >= 128;
}

void launch_conv3x3_wino_f32(const float* in, const void* wu, const float* bias, const float* res, float* out, uint32_t bpad, uint32_t cin,
                             uint32_t cout, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop, unsigned*) {
    if (!wino_f32_supported(bpad, cin, cout, 8)) {
        fprintf(stderr, "cattus: launch_conv3x3_wino_f32: unsupported shape (bpad %u, cin %u, cout %u)\n", bpad, cin, cout);
        abort();
    }
    const int ncb = wf32_ncb(bpad, cout);
    const dim3 grid(wf32_grid(bpad, cout, ncb));
    for_each_wino_f32([&](auto kernel, auto r, int n) {
        if (r == (res != nullptr) && n == ncb)
            hipExtLaunchKernelGGL(kernel, grid, dim3(WF32_THREADS), WF32_LDS_TOTAL, st, ev_start, ev_stop, 0, in, (const float*)wu, bias, res, out, (int)cin,
                                  (int)cout);
    });
}

hipError_t prepare_wino_f32() {
    hipError_t err = hipSuccess;
    for_each_wino_f32([&](auto kernel, auto, int) { lds_opt_in(err, kernel, WF32_LDS_TOTAL); });
    return err;
}

}  // namespace cattus
