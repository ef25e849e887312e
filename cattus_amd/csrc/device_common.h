// Definitions shared by the kernel translation units: vector types, the MFMA wrappers, the fragment-order index, the split
// tower's LDS pitch, tap table and weight-stage constants, the workgroup map over the XCDs, small helpers; and, for their
// host side, what a kernel family's one list of instances is written with.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace cattus {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

#define GLOBAL_PTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

template <typename T>
struct Mfma;

template <>
struct Mfma<__bf16> {
    typedef bf16x8 frag;
    static __device__ __forceinline__ void mac(const frag& a, const frag& b, f32x16& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};

// f16 operands (the split-precision tower: DESIGN.md section 3, K1s): same lane map and cycles as the bf16 form
template <>
struct Mfma<_Float16> {
    typedef f16x8 frag;
    static __device__ __forceinline__ void mac(const frag& a, const frag& b, f32x16& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
};

template <>
struct Mfma<float> {
    typedef f32x4 frag;
    // lane half h holds k = 4h + j in element j: the chain visits k = 0,4,1,5,2,6,3,7 of the 8-group
    static __device__ __forceinline__ void mac(const frag& a, const frag& b, f32x16& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b[3], c, 0, 0, 0);
    }
};

// Element index of (row, k) of a [rows][K] matrix kept in MFMA fragment order (kernels.h, HeadsMfma).
template <typename T>
__host__ __device__ constexpr size_t frag_packed_index(uint32_t row, uint32_t k, uint32_t K) {
    constexpr uint32_t KSTEP = 32 / sizeof(T), HALF = KSTEP / 2;
    return ((((size_t)(row >> 5) * (K / KSTEP) + k / KSTEP) * 2 + (k % KSTEP) / HALF) * 32 + (row & 31)) * HALF + k % HALF;
}

// f32 rows that feed a Winograd layer: capped at WINO_ACT_MAX (kernels.h), values beyond it counted like note_saturation's.
__device__ __forceinline__ void cap_wino_input(float (&y)[8], bool valid, unsigned* sat) {
    const float m = fmaxf(fmaxf(fmaxf(y[0], y[1]), fmaxf(y[2], y[3])), fmaxf(fmaxf(y[4], y[5]), fmaxf(y[6], y[7])));
    if (valid && m > WINO_ACT_MAX) {
        unsigned n = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) n += y[j] > WINO_ACT_MAX ? 1u : 0u;
        atomicAdd(sat, n);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) y[j] = y[j] < WINO_ACT_MAX ? y[j] : WINO_ACT_MAX;
}

// The same for rows that feed a Winograd F(4x4, 3x3) layer: the cap is WINOF4_ACT_MAX (winof4_rule.h).
__device__ __forceinline__ void cap_winof4_input(float (&y)[8], bool valid, unsigned* sat) {
    const float m = fmaxf(fmaxf(fmaxf(y[0], y[1]), fmaxf(y[2], y[3])), fmaxf(fmaxf(y[4], y[5]), fmaxf(y[6], y[7])));
    if (valid && m > WINOF4_ACT_MAX) {
        unsigned n = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) n += y[j] > WINOF4_ACT_MAX ? 1u : 0u;
        atomicAdd(sat, n);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) y[j] = y[j] < WINOF4_ACT_MAX ? y[j] : WINOF4_ACT_MAX;
}

// Off-board taps of the 3x3 kernels read zeros.  One zero ROW behind an image's rows put every such lane of a ds_read_b128 group on
// one bank slot, colliding with whichever lane's real row shares it (a quarter of the conv kernels' LDS cycles were bank conflicts).
// A zero AREA instead, 256-B aligned and read at (the off-board row's own address mod 256), gives the lane the banks its row would
// have had -- the group's addresses stay linear in the pixel index, as conflict-free as on a board without borders.  ZAREA_SP: for
// images of 144-byte rows read as (hi at +0, lo at +64): 255 + 64 + 16 bytes rounded up; 128-byte swizzled rows need 256.
constexpr int ZAREA_SP = 352;

// The f16 towers store activations as f16 and clamp them at 65504 instead of letting them overflow to infinity.  A clamped
// value is a wrong value: it is counted (atomic add on the clamp path only -- a network inside the f16 range never gets
// here) into the evaluator's sticky counter, which cattus_hip_stats reports as `saturated`.
__device__ __forceinline__ void note_saturation(const float (&y)[8], bool valid, unsigned* sat) {
    const float m = fmaxf(fmaxf(fmaxf(y[0], y[1]), fmaxf(y[2], y[3])), fmaxf(fmaxf(y[4], y[5]), fmaxf(y[6], y[7])));
    if (valid && m > 65504.0f) {
        unsigned n = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) n += y[j] > 65504.0f ? 1u : 0u;
        atomicAdd(sat, n);
    }
}

// Logical index of workgroup `block` of a grid of nblk.  Consecutive workgroup ids go round the 8 XCDs; the tiled kernels count
// (row block, cout block) with the cout block fastest, so this map gives every XCD one contiguous range of logical indices: all
// cout blocks of a range of boards run on one XCD and find their shared rows in its L2.  Grids that are no multiple of 8 stay as
// they are.  (I: blockIdx.x's unsigned, or the int of a workgroup that walks several grids.)
template <typename I>
__device__ __forceinline__ int xcd_remap(I block, int nblk) {
    return (nblk & 7) == 0 ? (block & 7) * (nblk >> 3) + (block >> 3) : block;
}

__device__ __forceinline__ void glds16(const char* src, char* lds_dst) {
    __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src), LDS_PTR(lds_dst), 16, 0, 0);
}

template <int N>
__device__ __forceinline__ void wait_vm_barrier() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit count");
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

// ---- split-precision tower (K1s, K1rs): LDS image and weight stages ----
constexpr int SP = 144;                                 // LDS row pitch
constexpr int SW_D = 6;                       // weight stages in flight per consumer wave; divides the 18 stages of a chunk
constexpr int SW_STAGE = 2048;                // bytes per 32-cout block and stage: hi fragment, lo fragment
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// Tap table of a consumer lane on images of SP-byte rows.  rowa[tap][pb]: byte offset, inside an image, of the row that tap reads
// for the lane's pixel pslot0 + pb * 32 + r of the board whose rows start at image row board_row, plus the lane half's 16 bytes;
// the image's zero area (at `zero`, above) for a tap off the board or a pixel slot past it.  Loop-invariant: a step adds the
// image's base, and tap, k-slice and hi / lo fold into ds_read immediates.
template <int NPB>
__device__ __forceinline__ void sp_tap_rows(int (&rowa)[9][NPB], int board_row, int pslot0, int r, int h, int S, int zero) {
#pragma unroll
    for (int pb = 0; pb < NPB; pb++) {
        const int p = pslot0 + pb * 32 + r;
        const int ph = p / S, pw = p - ph * S;
        const bool pvalid = p < S * S;
#pragma unroll
        for (int t9 = 0; t9 < 9; t9++) {
            const int hh = ph + t9 / 3 - 1, ww = pw + t9 % 3 - 1;
            const bool ok = pvalid && (unsigned)hh < (unsigned)S && (unsigned)ww < (unsigned)S;
            const int at = (board_row + hh * S + ww) * SP + h * 16;  // off the board: only its low 8 bits are used
            rowa[t9][pb] = ok ? at : zero + (at & 255);
        }
    }
}

// ---- split-precision tower: the epilogue its per-layer kernels share (K1s, K1s', K1sk) ----
// the 8 couts 8 cg .. 8 cg + 7 of staged pixel row px (kernels.hip, stage_tile: f32 [px][32 CB couts], 16-byte slots XORed with px & 7)
__device__ __forceinline__ void staged_read(float (&v)[8], const char* rowp, int px, int cg) {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(rowp + (((2 * cg) ^ (px & 7)) << 4));
    const f32x4 hi = *reinterpret_cast<const f32x4*>(rowp + (((2 * cg + 1) ^ (px & 7)) << 4));
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = lo[j], v[4 + j] = hi[j];
}

// Rows of `in` / `res` / `out`: 4 bytes per channel, the hi values of cout c at element sp_col(c), the lo values 32 further.
__device__ __forceinline__ int sp_col(int c) { return (c >> 5) * 64 + (c & 31); }

// One pixel row's 8 accumulator sums to its stores: the lane's 8 couts from `col` on of tower row `row`.  Times the inverse weight
// scale plus bias (the accumulator carries the weights' power-of-two scale, so the product is exact and the fused multiply-add
// rounds as a multiply followed by an add would), + skip as hi + lo (exact in f32: lo is at most half an ulp of hi, 22 significant
// bits), ReLU, then either plain f32 rows (flags & CONV_OUT_F32: the tower's last layer, for the head kernels or a Winograd
// tower's stem) or the clamp at 65504 and the split into (hi, lo).  Pixel slots past the board (!valid) stay zero: masked once,
// on the packed vectors.  Stores: non-temporal on the full grid (CB = 2), where a layer's 16.7 MB of output and its 2.4 MB of
// weights do not fit the XCDs' L2 together; plain on the small-grid tile (CB = 1, <= 128 leaves of an 8x8 game), where the output
// stays in the L2 of the XCD whose workgroups read it back as the next layer's input (xcd_remap keeps a row block on one XCD):
// 18.5 us per launch against 19.9 with non-temporal stores at batch 64, no difference at 128.
template <int CB, bool HAS_RES>
__device__ __forceinline__ void finish_f16x2_sums(float (&v)[8], const f32x4 (&ds8)[2], const f32x4 (&bias8)[2], const _Float16 (&resv)[16], bool valid,
                                                  int flags, unsigned* sat, _Float16* out, size_t row, int cout, int col) {
    typedef _Float16 T;
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = __builtin_fmaf(v[j], ds8[j >> 2][j & 3], bias8[j >> 2][j & 3]);
    if (HAS_RES) {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = v[j] + ((float)resv[j] + (float)resv[8 + j]);
    }
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; j++) y[j] = v[j] > 0.0f ? v[j] : 0.0f;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    if (flags & CONV_OUT_F32) {
        if (flags & CONV_WINO_IN) cap_wino_input(y, valid, sat);
        else if (flags & CONV_WINOF4_IN) cap_winof4_input(y, valid, sat);
        float* of = reinterpret_cast<float*>(out) + row * (size_t)cout + col;
        const f32x4 y0 = valid ? *reinterpret_cast<f32x4*>(y) : zero4, y1 = valid ? *reinterpret_cast<f32x4*>(y + 4) : zero4;
        if constexpr (CB == 2) {
            __builtin_nontemporal_store(y0, reinterpret_cast<f32x4*>(of));
            __builtin_nontemporal_store(y1, reinterpret_cast<f32x4*>(of) + 1);
        } else {
            reinterpret_cast<f32x4*>(of)[0] = y0;
            reinterpret_cast<f32x4*>(of)[1] = y1;
        }
    } else {
        const size_t off = row * ((size_t)cout * 2) + sp_col(col);
        T hi[8], lo[8];
        note_saturation(y, valid, sat);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float yc = y[j] < 65504.0f ? y[j] : 65504.0f;  // saturate instead of overflowing to infinity
            hi[j] = (T)yc;
            lo[j] = (T)(yc - (float)hi[j]);
        }
        const f32x4 hi4o = valid ? *reinterpret_cast<f32x4*>(hi) : zero4, lo4o = valid ? *reinterpret_cast<f32x4*>(lo) : zero4;
        if constexpr (CB == 2) {
            __builtin_nontemporal_store(hi4o, reinterpret_cast<f32x4*>(out + off));
            __builtin_nontemporal_store(lo4o, reinterpret_cast<f32x4*>(out + off + 32));
        } else {
            *reinterpret_cast<f32x4*>(out + off) = hi4o;
            *reinterpret_cast<f32x4*>(out + off + 32) = lo4o;
        }
    }
}
// The same from a staged pixel row (stage_tile): K1s and K1s'.
template <int CB, bool HAS_RES>
__device__ __forceinline__ void finish_f16x2(const char* rowp, int px, int cg, const f32x4 (&ds8)[2], const f32x4 (&bias8)[2],
                                             const _Float16 (&resv)[16], bool valid, int flags, unsigned* sat, _Float16* out, size_t row,
                                             int cout, int col) {
    float v[8];
    staged_read(v, rowp, px, cg);
    finish_f16x2_sums<CB, HAS_RES>(v, ds8, bias8, resv, valid, flags, sat, out, row, cout, col);
}

// ---- the value head's tanh (K5, the SIMT value kernels, the dense layers, the short-chain FC pair) ----
// tanh from + - * / fmaf and exponent-bit edits only, so the CPU oracle reproduces it bit for bit.
__device__ __forceinline__ float exp_pos(float x) {
    const float log2e = 1.44269504088896341f;
    const float ln2_hi = 0.693145751953125f;
    const float ln2_lo = 1.42860682030941723e-06f;
    const float nf = __builtin_rintf(x * log2e);
    float rr = __builtin_fmaf(nf, -ln2_hi, x);
    rr = __builtin_fmaf(nf, -ln2_lo, rr);
    float p = 1.0f / 720.0f;
    p = __builtin_fmaf(p, rr, 1.0f / 120.0f);
    p = __builtin_fmaf(p, rr, 1.0f / 24.0f);
    p = __builtin_fmaf(p, rr, 1.0f / 6.0f);
    p = __builtin_fmaf(p, rr, 0.5f);
    p = __builtin_fmaf(p, rr, 1.0f);
    p = __builtin_fmaf(p, rr, 1.0f);
    return __uint_as_float(__float_as_uint(p) + (((uint32_t)(int32_t)nf) << 23));
}

__device__ __forceinline__ float tanh_exact(float x) {
    const float ax = __builtin_fabsf(x);
    float t;
    if (!(ax == ax)) return x;
    if (ax < 0.5f) {
        // odd Taylor series to x^15: the x^15 term is 4.4e-8 at 0.5, 1.5 ulp of the result -- without it the value an ulp below 0.5
        // lay an ulp ABOVE the exp branch's at 0.5 (tanh must not decrease); with it both branches are monotone across the seam
        const float s = ax * ax;
        float p = -929569.0f / 638512875.0f;
        p = __builtin_fmaf(p, s, 21844.0f / 6081075.0f);
        p = __builtin_fmaf(p, s, -1382.0f / 155925.0f);
        p = __builtin_fmaf(p, s, 62.0f / 2835.0f);
        p = __builtin_fmaf(p, s, -17.0f / 315.0f);
        p = __builtin_fmaf(p, s, 2.0f / 15.0f);
        p = __builtin_fmaf(p, s, -1.0f / 3.0f);
        t = __builtin_fmaf(ax * s, p, ax);
    } else if (ax < 10.0f) {
        const float e = exp_pos(2.0f * ax);
        t = 1.0f - 2.0f / (e + 1.0f);
    } else {
        t = 1.0f;
    }
    return x < 0.0f ? -t : t;
}

// ---- the f32 head convs in a resident tower's tail (cattus_hip_fused_heads; head_fuse_rule.h has the LDS plan, the ownership map, the
// chain's order and the hv index) ----
// The operands' way into LDS: the four loader waves, once they have issued and awaited their last weight slab, copy the [32][64] f32 head
// weights to the pitched image at lds_w and the 32 biases to lds_b -- under the consumers' last step, into bytes that are dead behind that
// step's barrier -- and then meet the consumers at the barrier that orders these stores (and the consumers' staged rows) against the chain's
// fragment reads.  t: 0 .. HF_STAGE_THREADS - 1.
__device__ __forceinline__ void hf_stage_operands(const float* head_w, const float* head_b, char* lds_w, char* lds_b, int t) {
    typedef const __attribute__((address_space(1))) f32x4* gf32x4p;
    typedef const __attribute__((address_space(1))) float* gf32p;
    const gf32x4p w = (gf32x4p)head_w;
    const f32x4 v0 = w[t], v1 = w[t + HF_STAGE_THREADS];
    const float bv = ((gf32p)head_b)[t & 31];
    *reinterpret_cast<f32x4*>(lds_w + hf_piece_dst(t)) = v0;
    *reinterpret_cast<f32x4*>(lds_w + hf_piece_dst(t + HF_STAGE_THREADS)) = v1;
    if (t < HF_CHANNELS) *reinterpret_cast<float*>(lds_b + t * 4) = bv;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The chain and its epilogue, behind that barrier: the consumer wave that owns a 32-row tile (hf_tile_of_wave) runs head_conv_tile<float>'s
// eight stages -- all sixteen fragment reads issued ahead of the first MFMA, as there -- and writes acc + bias, ReLU to hv for the rows of
// the pass's n leaves that are pixels of a board and the channels the heads have.  row_frag(row, u, h): LDS byte address of tower row
// `row`'s fragment of stage u for lane half h.  A: the tower's arguments (Tower64Args: n, S, hv, hv_pol, kvp, kpp, vhc, ocn).
template <int CH, class Args, class RowFrag>
__device__ __forceinline__ void hf_head_convs(const char* smem, const HfLds& lds, RowFrag row_frag, int wave, int lane, int row0, uint32_t slots, const Args& A) {
    if (hf_tile_of_wave(CH, wave) < 0) return;
    const int r = lane & 31, h = lane >> 5;
    const int row = hf_own(CH, wave, lane, 0).row;
    f32x4 hb[4];
#pragma unroll
    for (int g = 0; g < 4; g++) hb[g] = *reinterpret_cast<const f32x4*>(smem + lds.b + (8 * g + 4 * h) * 4);
    f32x4 fa[8], fb[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
        fa[u] = *reinterpret_cast<const f32x4*>(smem + lds.w + hf_w_frag(r, u, h));
        fb[u] = *reinterpret_cast<const f32x4*>(smem + row_frag(row, u, h));
    }
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.0f;
#pragma unroll
    for (int u = 0; u < 8; u++) Mfma<float>::mac(fa[u], fb[u], acc);
    const HfHead H{A.S * A.S, A.vhc, A.ocn, A.kvp, A.kpp, A.hv_pol, slots};
    const uint32_t grow = (uint32_t)(row0 + row);
    float* const hv = reinterpret_cast<float*>(A.hv);
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const uint32_t i = (uint32_t)hf_own(CH, wave, lane, e).channel;
        if (!hf_writes(H, A.n, grow, i)) continue;
        const float y = acc[e] + hb[e >> 2][e & 3];
        hv[hf_hv_index(H, grow, i)] = y > 0.0f ? y : 0.0f;
    }
}

// The HEADS instance of a resident tower is entered through this one kernel: Tower::run is the tower's body with the flag on,
// Tower::Args its argument struct, Tower::MIN_WAVES its twin's second launch bound.  (A name of its own: the twins' names keep meaning the
// instances they always meant, in scripts/kernel_regs.py's listing as everywhere.)
template <class Tower>
__global__ void __launch_bounds__(512, Tower::MIN_WAVES) tower_heads_kernel(typename Tower::Args A) {
    Tower::run(A);
}

// ---- host side: a kernel family's instances, listed once ----
// Next to its kernels every templated family has one for_each_* visitor.  It calls f(kernel, ..., template arguments as
// std::integral_constant values) for every instance that exists; an `if constexpr` on the family's rule keeps the other
// combinations from being instantiated.  The family's prepare_* sets the dynamic-LDS opt-in through it and its launcher picks,
// through it, the instance whose arguments equal the launch's run-time key (a scan of at most 18 entries).
template <class F>
void each_bool(F&& f) {
    f(std::false_type{});
    f(std::true_type{});
}
template <int... V, class F>
void each_int(F&& f) {
    (f(std::integral_constant<int, V>{}), ...);
}
// The opt-in for more than 64 KiB of dynamic LDS is a per-device function attribute; `err` keeps the first failure.
template <class K>
void lds_opt_in(hipError_t& err, K* kernel, int bytes) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (err == hipSuccess) err = e;
}

}  // namespace cattus
