// Host side of libcattus_hip.so: the C ABI declared in include/cattus_hip.h.
//
// Replaces NNetwork::run_net + Model::{new,run} (reference: engine/src/net/mod.rs:41-72,
// engine/src/net/model.rs:61-218) and Batcher::apply (engine/src/util/batch.rs:49-177).
// There is deliberately no CPU fallback: without a usable HIP device every entry point fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include <dlfcn.h>

#include "../../include/cattus_hip.h"
#include "../../include/cattus_hip_diag.h"
#include "kernels.h"
#include "weight_layout.h"

// Kernel arguments in device memory: by default the HIP runtime keeps the kernel-argument ring in host memory and the
// command processor fetches every launch's arguments over the host link before the first wave starts (~1.6 us per
// launch, 8 % of a 41-launch bf16 forward pass; profiles/r02_experiments.txt).  HIP_FORCE_DEV_KERNARG=1 moves the ring
// into HBM, but the runtime reads it once, when it initialises, and the variable belongs to the HOST process: this
// library does not touch the environment (a library constructor calling setenv races with the host's threads and
// changes the runtime for every other HIP user).  bench.py, the tests, the Python package (opt-out: CATTUS_NO_ENV_DEFAULTS=1)
// and bin/*_self_player export it; INTEGRATION.md tells a Rust host to do the same.  cattus_hip_create reports the
// setting it found in cattus_hip_runtime_note().
static std::string g_runtime_note;

using namespace cattus;

#define CATTUS_API extern "C" __attribute__((visibility("default")))

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t err__ = (expr);                                                                      \
        if (err__ != hipSuccess)                                                                        \
            return fail(CATTUS_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(err__), __FILE__, __LINE__); \
    } while (0)

constexpr size_t HEADER_BYTES = 64;
constexpr float BN_EPS = 1e-5f;
constexpr uint32_t FC_HIDDEN = 128;

// BatchNorm (eval) folded into the preceding bias-free conv:
//   scale = gamma / sqrtf(var + eps);  w' = w * scale;  b' = beta - mean * scale
// (gamma = 1, beta = 0 where the reference builds BatchNorm2d(affine=False): net_utils.py:14,30,68,78).
// This file is compiled with -ffp-contract=off: the products and the subtraction round separately.  (Folded: weight_layout.h)
Folded fold_conv(const float* w, uint32_t cout, uint32_t cin, uint32_t taps, const float* gamma, const float* beta,
                 const float* mean, const float* var) {
    Folded f;
    f.w.resize((size_t)taps * cout * cin);
    f.b.resize(cout);
    for (uint32_t co = 0; co < cout; co++) {
        const float g = gamma ? gamma[co] : 1.0f;
        const float be = beta ? beta[co] : 0.0f;
        const float scale = g / sqrtf(var[co] + BN_EPS);
        f.b[co] = be - mean[co] * scale;
        for (uint32_t ci = 0; ci < cin; ci++)
            for (uint32_t t = 0; t < taps; t++)
                f.w[((size_t)t * cout + co) * cin + ci] = w[((size_t)co * cin + ci) * taps + t] * scale;
    }
    return f;
}

// The f16 towers' stream shift t >= 0.  An f16x2 epilogue splits an activation y unscaled into hi = f16(y), lo = f16(y - hi): once
// |y| < 2^-3 lo is an f16 subnormal and y keeps an absolute resolution of 2^-25 instead of 22 significant bits.  Weights get a
// power-of-two scale per output channel; the residual stream (the stem output, each block's output) is scaled by the trained
// BatchNorm gamma / beta of the stem and the blocks' _bn2 alone (_bn1 has no affine parameters: the middle activation is unit
// scale).  So the tower carries the stream at 2^t times its size: stem w, b x 2^t, every block's conv1 w x 2^-t, conv2 w, b x 2^t,
// the head convs' w x 2^-t -- exact power-of-two products that the per-channel weight scales absorb, the same function in exact
// arithmetic.  S = median over channels of sqrt(gamma_stem^2 + beta_stem^2 + sum over blocks (gamma_2^2 + beta_2^2)) estimates the
// stream's RMS.  S >= 1/2 keeps t = 0: the weights, and so the bits, of a tower without the shift (every seeded network: S lies in
// [0.9, 2.7), near 1 where the blocks are few).  A smaller S is lifted into [1, 2): t = -floor(log2 S), at most 16; 0 where S is 0
// or not finite.
// One t for the tower leaves the cliff in place channel by channel: a trained network's channels differ in scale, and a channel that
// runs below 2^-3 beside a median of O(1) still stores subnormal lo halves.  The products above are per channel anyway -- channel k is
// an output row of the stem and of every conv2 and an input column of every conv1 and of the head convs -- so channel k is carried at
// 2^t_k, t_k = t + r_k: with s_k the same estimate for channel k alone, r_k = 0 where s_k 2^t >= 1/2 (every seeded channel: s_k >= 0.75,
// the same bits again) and where s_k is 0 (a dead channel) or not finite; a smaller channel is lifted into [1, 2) as S is, t_k at most
// 16.  The rule itself is weight_layout.h's stream_shifts (tests/weight_layout_check.cpp); t is what cattus_hip_stream_shift reports,
// every t_k what cattus_hip_stream_shifts does.
// `ceiling` (weight_layout.h, stream_shifts): the F(4x4, 3x3) tower alone passes one, WINOF4_STREAM_CEILING -- a median far below a few
// channels would carry those past its cap of 655 -- and a channel it holds back has t_k below the t reported here.
std::vector<int> choose_stream_shift(const cattus_net_desc& d, const float* p, int* t, double ceiling) {
    const uint32_t F = d.filters;
    const float* g0 = p + (size_t)F * d.planes * 9;
    const float* b0 = g0 + F;
    const size_t stem = (size_t)F * d.planes * 9 + 4 * F, block = (size_t)2 * F * F * 9 + 6 * F;
    std::vector<double> s(F);
    for (uint32_t c = 0; c < F; c++) s[c] = (double)g0[c] * g0[c] + (double)b0[c] * b0[c];
    for (uint32_t i = 0; i < d.blocks; i++) {
        const float* g2 = p + stem + i * block + (size_t)F * F * 9 + 2 * F + (size_t)F * F * 9;
        const float* b2 = g2 + F;
        for (uint32_t c = 0; c < F; c++) s[c] += (double)g2[c] * g2[c] + (double)b2[c] * b2[c];
    }
    *t = stream_shift_global(s);
    return stream_shifts(s, ceiling);
}

// What cattus_hip_create_calibrated measured on its sample positions (cattus_hip_stream_range of an f32 evaluator of the same blob): per
// stream channel the mean square and the largest |value|.  With it build() takes weight_layout.h's calibrated_stream_shifts in place of
// choose_stream_shift: the estimate above is exact only while every BatchNorm input has unit variance under its running statistics and
// nothing but gamma / beta carries the scale -- a channel whose conv rows, running_mean and beta are all 2^-8 of a unit channel's beside
// an unchanged gamma is the same function with s_k = O(1) and a stream at 2^-8.
struct Calibration { std::vector<double> s2, abs_max; };

// A folded layer whose output channels write the stream, or whose input channels read it, with stream channel k at 2^tk[k] times
// its size (exact: powers of two): writes, output channel k's w, b x 2^tk[k]; reads, input channel k's w x 2^-tk[k]
void shift_folded(Folded& f, uint32_t cin, const std::vector<int>& tk, bool writes) {
    const size_t cout = f.b.size();  // w [taps][cout][cin]
    for (size_t i = 0; i < f.w.size(); i++) f.w[i] = ldexpf(f.w[i], writes ? tk[i / cin % cout] : -tk[i % cin]);
    for (size_t co = 0; writes && co < cout; co++) f.b[co] = ldexpf(f.b[co], tk[co]);
}

// One device allocation that a tower's hot buffers are carved from (the Winograd tower: the transformed weights of all layers and
// the activation buffers).  What a forward pass of chess 20x256 touches -- 168 MB of U, 50 MB of activations -- is most of the 256 MB
// Infinity Cache, which is indexed by physical address: 110 separately allocated 2 MB pages land on its sets unevenly, some sets
// overflow, and the weight stream then comes from HBM in part (the same binary ran a layer in 31 or in 34 us from one process to
// the next, and towers of <= 17 blocks always in 31).  One contiguous block covers the sets evenly.
struct DevArena {
    char* base = nullptr;
    size_t cap = 0, used = 0;
    ~DevArena() {
        if (base) (void)hipFree(base);
    }
    void* take(size_t bytes) {  // nullptr when it does not fit (or there is no arena): the caller allocates on its own
        const size_t at = (used + 4095) & ~(size_t)4095;
        if (!base || at + bytes > cap) return nullptr;
        used = at + bytes;
        return base + at;
    }
};

struct DevBuf {
    void* p = nullptr;
    bool owned = true;  // false: carved from a DevArena, which frees it
    ~DevBuf() {
        if (p && owned) (void)hipFree(p);
    }
    int alloc(size_t bytes, DevArena* arena = nullptr) {
        if (p && owned) (void)hipFree(p);
        p = nullptr, owned = true;
        if (arena && (p = arena->take(bytes ? bytes : 16))) {
            owned = false;
            return CATTUS_OK;
        }
        hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        if (e != hipSuccess) return fail(CATTUS_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return CATTUS_OK;
    }
    int upload(const void* src, size_t bytes, DevArena* arena = nullptr) {
        int rc = alloc(bytes, arena);
        if (rc) return rc;
        HIP_TRY(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
        return CATTUS_OK;
    }
    template <typename T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

struct PinnedBuf {
    void* p = nullptr;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    int alloc(size_t bytes) {
        hipError_t e = hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault);
        if (e != hipSuccess) return fail(CATTUS_E_NOMEM, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return CATTUS_OK;
    }
    template <typename T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

// page-locked host ranges handed out by cattus_hip_host_alloc: start -> length.  Every evaluation probes
// this (three pointers per batch, from several threads), allocation is rare: readers share the lock.
std::shared_mutex g_pin_mu;
std::map<const char*, size_t> g_pinned;
// Optional ROCTx ranges around every batch (CATTUS_ROCTX=1): they show up in `rocprofv3 --marker-trace`.
// The library is looked up at run time so that nothing links against the profiler.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        const char* on = getenv("CATTUS_ROCTX");
        if (!on || on[0] != '1') return;
        for (const char* name : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
            if (void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {
                push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
                pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                if (push && pop) return;
                push = nullptr, pop = nullptr;
            }
        }
    }
};
const Roctx& roctx() {
    static const Roctx r;
    return r;
}
struct RoctxRange {
    bool on;
    RoctxRange(const char* what, uint32_t n) : on(roctx().push != nullptr) {
        if (on) {
            char buf[64];
            snprintf(buf, sizeof buf, "%s n=%u", what, n);
            roctx().push(buf);
        }
    }
    ~RoctxRange() {
        if (on) roctx().pop();
    }
};

bool is_pinned(const void* p) {
    std::shared_lock<std::shared_mutex> lk(g_pin_mu);
    auto it = g_pinned.upper_bound((const char*)p);
    if (it == g_pinned.begin()) return false;
    --it;
    return (const char*)p < it->first + it->second;
}

struct ConvLayer { DevBuf w, b; };  // in the one layout the tower's kernel reads this layer in (upload_conv)

struct ServerBatch {
    uint64_t seq = 0;
    uint32_t count = 0, collected = 0;
    bool sealed = false, running = false, done = false;
    int status = CATTUS_OK;
    std::string error;
    std::chrono::steady_clock::time_point t0;
    std::vector<uint64_t> planes;
    std::vector<float> policy, value;
    std::vector<uint8_t> taken;  // per slot: its ticket has been waited for
    // cattus_hip_submit_legal's leaves (legal_span.h): their lists back to back, the offset table as far as it is closed, and per slot whether it
    // came with a list (slots behind the last one that did are plain).  All three stay empty in a batch of plain leaves.
    std::vector<uint16_t> legal_idx;
    std::vector<uint32_t> legal_off;
    std::vector<uint8_t> kind;
    uint32_t legal_leaves = 0;
    std::vector<float> probs;  // [legal_off[count]], the legal leaves' softmax rows at their lists' places
    bool is_legal(uint32_t slot) const { return slot < kind.size() && kind[slot]; }
};

constexpr int NLANES = CATTUS_HIP_LANES;

struct Lane {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;  // blocking-sync event: the host thread sleeps until the batch is back
    DevBuf d_planes, x0, a, t, y, hv, h1, d_policy, d_value;
    DevBuf d_legal_idx, d_legal_cnt, d_probs;  // legal-move softmax operands, allocated on first use
    uint32_t legal_stride = 0;
    // the leaf server's ragged batches (legal_span.h), allocated for every lane at the first cattus_hip_submit_legal and sized for max_batch lists of
    // 1024: the lists, the offset table [max_batch + 1] and the probabilities on the device and in page-locked memory; rag_probs_ref, the shadow's
    // rows of a verified batch, on the lane's first such batch
    DevBuf rag_idx, rag_off, rag_probs, rag_probs_ref;
    PinnedBuf h_rag_idx, h_rag_off, h_rag_probs;
    // cattus_hip_stream_range, allocated on first use: the range kernel's workgroup partials, and the per-channel accumulators
    // [fpad sums of squares (double) | fpad maxima (float)] that collect over a call's tensors and chunks, ordered by `stream`
    DevBuf range_part_sq, range_part_max, range_acc;
    PinnedBuf h_planes, h_policy, h_value;
    // the Winograd tower in one launch (tower_wino4_kernel): this lane's layer table, hand-off counters and error word, and the
    // page-locked word the error word is copied to behind every such launch
    DevBuf tower_layers, tower_ready;  // tower_ready: [error word, pad to 64 B | a counter per (layer, board group)] -- one memset per batch
    PinnedBuf h_tower_err;
    // cattus_hip_verify, allocated when it is first turned on: a verified batch's [n records | n details] (kernels.h, launch_verify_outputs)
    // on the device and in page-locked memory.  (The batch's planes are on the host either way: in the caller's page-locked buffer or in h_planes.)
    DevBuf d_verify;
    PinnedBuf h_verify;
    // the priors part of it (prior_rule.h), verified cattus_hip_eval_legal batches only: a record per leaf on the device and in page-locked memory
    // (allocated with d_verify), and the shadow's legal-move softmax [max_batch][prior_stride] (allocated on first use, like d_probs)
    DevBuf d_prior, d_probs_ref;
    PinnedBuf h_prior;
    uint32_t prior_stride = 0;
    // cattus_hip_tap / cattus_hip_trace, allocated on first use: one point's f32 [max_batch][channels][S*S], the [points][max_batch] records, and the
    // stream shifts as the kernels read them (only where some channel is shifted)
    DevBuf d_tap, d_trace, d_shifts;
    std::mutex mu;  // held while a batch uses the lane
    ~Lane() {
        if (done) (void)hipEventDestroy(done);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// Which tower an evaluator runs: resolved once, by resolve_plan() in cattus_hip_create, never per batch (a leaf's result must not depend
// on the batch it came in).  Everything that differs between the paths -- what is uploaded, allocated, launched, reported -- reads this.
enum class TowerKind {
    // SimpleTwoHeadedModel (training/cattus_train/net_utils.py:92-121; blob with filters == 0): planes -> f32 tensor -> two dense layers
    // + ReLU -> a dense tanh value head and a dense policy head, all in f32 whatever cfg.dtype says (the net is tiny)
    Simple,
    Generic,     // NCHW f32 SIMT tower: heads wider than one 32-row MFMA tile, or the checker (CATTUS_FORCE_GENERIC=1)
    PerLayer,    // MFMA NHWC tower, one launch per conv layer (any dtype)
    Resident64,  // bf16, <= 64 filters: the whole tower in one launch, activations resident in LDS (tower64_lds_kernel; CATTUS_TOWER64=0: PerLayer)
                 // Act::F16 with this kind: the same launch with the per-layer f16 tower's bits, only for tower_form RESIDENT, never by AUTO
    Resident64Split,  // f16x2, <= 64 filters: the same in split precision (tower64_split_kernel; weights from the register ring)
    // f16x2, 8x8 boards: every layer behind the stem in Winograd F(2x2, 3x3) form, for max_batch > 128 (up to there the direct kernels'
    // small tiles win or tie -- whole step of chess 20x256, direct | Winograd: 0.59 | 0.89 ms at 64 leaves, 0.87 | 0.89 at 96, 0.97 | 0.90 at
    // 128 full and ~0.87 | 0.89 at the ~93 a 128-leaf self-play batch holds; from 129 on the direct form needs a second 128-row tile: 1.45 |
    // 0.93 at 160, 1.53 | 1.01 at 192, 1.77 | 1.25 at 256, scripts/by_batch_forms.py); cattus_eval_config.tower_form forbids / forces it.
    Wino16,  // the 16-frequencies kernel (kernels_wino.hip)
    Wino4,   // the 4-frequencies x 2x2-blocks kernel (kernels_wino4.hip) wherever it covers the shape; same bits (CATTUS_WINO_KERNEL=k16|k4)
    // the same tower with every layer behind the stem in Winograd F(4x4, 3x3) form (kernels_winof4.hip): only for tower_form WINOGRAD_F4,
    // never by AUTO; other bits than the F(2x2) kinds, activations capped at WINOF4_ACT_MAX, always one launch per layer
    WinoF4,
    // dtype f16w (Act::F16 with this kind, and no other kind for that dtype): the stem on the direct f16 kernel, every layer behind it in
    // Winograd F(2x2, 3x3) form with ONE f16 term per product and f32 rows between the layers (kernels_wino_f16.hip); bits of its own,
    // activations capped at WINO_ACT_MAX, always one launch per layer
    WinoF16,
    // dtype f32w (Act::F32 with this kind, and no other kind for that dtype): the stem on the direct f32 kernel with the exact tower's bits,
    // every layer behind it in Winograd F(2x2, 3x3) form with f32 operands on the f32 tower's own rows (kernels_wino_f32.hip); bits of its
    // own, no cap, no stream shift, no saturation counter, always one launch per layer
    WinoF32,
    // f16x2, 64-slot boards, 128 .. SK_MAX_FILTERS filters: the per-layer direct tower with the K walk of every layer behind the stem divided
    // over the waves of a workgroup (kernels_splitk.hip), for batches of a few leaves: only for tower_form DIRECT_SPLITK, never by AUTO; its
    // f32 summation order, and so its bits, are its own; rows in the direct form's layout
    DirectSplitK,
    // dtype f16r (Act::F16 with this kind, and no other kind for that dtype): the per-layer direct f16 tower with the residual stream kept
    // in f32 (K1hr: conv3x3_f16r_kernel for the stem and every conv2, dtype f16's own layer for every conv1; f16r_rule.h has the buffer
    // plan): dtype f16's weights, scales, shifts and coverage, bits of its own from point 2 on, always one launch per layer
    PerLayerStream,
    // dtype f16r_resident (Act::F16 with this kind, and no other kind for that dtype): PerLayerStream's tower of a network with <= 64 filters
    // in one LDS-resident launch (K1hr resident: tower64_stream_kernel; t64r_rule.h) -- the f32 stream in the owning lanes' registers, dtype
    // f16r's weights, scales, shifts, calibration and bits; Resident64's coverage, workgroup shapes and switches; observed on PerLayerStream
    Resident64Stream,
    // dtype f32_resident (Act::F32 with this kind, and no other kind for that dtype): PerLayer's exact f32 tower of a network with <= 64 filters
    // and <= 32 planes in one LDS-resident launch (K1rf: tower64_f32_kernel; t64f_rule.h) -- dtype f32's weights, biases and bits; the resident
    // predicate's coverage with a one-chunk stem; observed on PerLayer; like dtype f32 it is the exact tower and has no shadow
    Resident64F32,
};
struct TowerPlan {
    TowerKind kind = TowerKind::Generic;
    bool w_frag = false;   // f16x2 weights in fragment order for the register-ring kernels (CATTUS_SPLIT_W=0: rows, through the LDS ring)
    bool inplace = false;  // Winograd kinds: a block's output over its own skip rows (CATTUS_WINO_INPLACE=0: a third activation buffer)
    // Wino4: every layer behind the stem as ONE launch (tower_wino4_kernel), one workgroup per CU, several tiles per workgroup and layer where
    // a layer has more tiles than the device has CUs (CATTUS_WINO_PERSIST=0: per-layer launches) -- for the batches one_launch_now() admits
    bool one_launch = false;
    bool tuned() const { return kind != TowerKind::Simple && kind != TowerKind::Generic; }  // the MFMA NHWC towers
    bool resident() const { return kind == TowerKind::Resident64 || kind == TowerKind::Resident64Split || kind == TowerKind::Resident64Stream || kind == TowerKind::Resident64F32; }  // one launch, activations in LDS
    bool f32_stream() const { return kind == TowerKind::PerLayerStream || kind == TowerKind::Resident64Stream; }  // dtype f16r's arithmetic (f16r_rule.h)
    bool wino() const { return kind == TowerKind::Wino16 || kind == TowerKind::Wino4 || kind == TowerKind::WinoF4 || kind == TowerKind::WinoF16 || kind == TowerKind::WinoF32; }  // f32 rows between the layers
};

}  // namespace

struct cattus_eval {
    DevArena arena;  // first member: destroyed last, behind every buffer carved from it
    cattus_net_desc d{};
    cattus_eval_config cfg{};
    TowerPlan plan;
    DevBuf d1w, d1b, d2w, d2b, svw, svb, spw, spb;  // TowerKind::Simple
    bool wait_spin = true;  // host wait for a batch: spinning hipStreamSynchronize, or a blocking event
    Act act = Act::F32;
    uint32_t hw = 0, bpad = 0, cpad0 = 0;
    uint32_t slots = 64;  // pixel slots per board of the tuned tower (kernels.h: tower_slots)
    uint32_t fpad = 0;    // filters as laid out on the device: rounded up to 64 on the tuned path (zero channels)
    DevBuf t64_layers, t64s_bias;  // the resident towers' layer table; Resident64Split: every layer's [biases | inverse scales]
    bool t64s_fuse_heads = true;  // CATTUS_T64S_HEADS=0: the head convs as their own launch on the tower's f32 rows (A/B, the equality test)
    int t64s_depth = 0;           // CATTUS_T64S_SHAPE=1|2: workgroup shape of the resident split tower (kernels.h; 0: by grid size)
    bool pack_separately = false;  // more than 32 planes, or CATTUS_FUSED_STEM=0 (A/B, tests): the plane pack as its own launch in front of the stem
    int t64_force_ch = 0;          // CATTUS_T64_CH=2|4: workgroup shape of the resident tower (A/B runs, the row-split test)
    bool t64f_narrow = true;       // CATTUS_T64F_NARROW=0: the resident f32 tower walks both chunks of a <= 32-filter network too (A/B, the equality test)
    // the one-launch Winograd tower: set when a launch reported a hand-off wait that gave up (CATTUS_WINO_SPIN=<polls>: the budget of a
    // wait) -- that batch is run again on the per-layer launches, and so is every later one
    std::atomic<bool> tower_gave_up{false};
    uint32_t persist_spin = 1u << 18, cus = 0;
    // cattus_eval_config.tail_leaves as it holds on this plan (0 on every plan but Wino4 / Wino16): an unobserved pass of at most this many
    // leaves runs the layers behind the stem on the small-tile kernel (kernels_wino4s.hip), the same bits; tail_batches counts those passes
    uint32_t tail_leaves = 0;
    std::atomic<uint64_t> tail_batches{0};
    // cattus_hip_head_chain as it holds (0 wherever the heads are not the f32 MFMA heads): an unobserved, untimed pass of at most this many leaves runs
    // FC1 + FC2 and the policy FC on head_fc_chain_kernel (kernels_head_chain.hip) instead of head_fc_pair_kernel<float>, the same bits;
    // head_chain_batches counts those passes.  Written with every lane mutex held, read by a pass under its lane's
    std::atomic<uint32_t> head_chain{0};
    std::atomic<uint64_t> head_chain_batches{0};
    // cattus_hip_fused_heads as it holds (0 wherever head_fuse_rule.h's hf_takes says the plan has no HEADS instance): an unobserved, untimed pass
    // launches the resident tower's HEADS instance, which runs the head convs in its tail, and no head conv launch; fused_heads_batches counts
    // those passes.  Written and read as head_chain is.
    std::atomic<uint32_t> fused_heads{0};
    std::atomic<uint64_t> fused_heads_batches{0};
    int splitk_forced = 0;  // CATTUS_SPLITK_WAYS=1|2|4|8: the way count of the split-K direct form (tests and A/B; 0: splitk_rule.h's rule)
    // the f16 towers carry the residual stream at 2^stream_shift times its size, channel k of it at 2^stream_shifts[k] >= that
    // (choose_stream_shift; from cattus_hip_create_calibrated: calibrated_stream_shifts, whose headroom guard can take a channel
    // below the global shift, as the F(4x4) tower's ceiling on the estimate can); CATTUS_STREAM_SHIFT=0: never
    bool stream_shift_on = true;
    int stream_shift = 0;
    std::vector<int> stream_shifts;
    // tile-forcing switches (CATTUS_CONV_CB, CATTUS_CONV_PBW: A/B runs, the tile-equality tests) and the f16 towers' saturation
    // counter: this evaluator's own -- a second evaluator in the process (model1 vs model2) neither re-tiles nor shares them
    ConvOpts conv_opts;
    DevBuf d_saturated;
    bool t64_layer_steps = true;   // CATTUS_T64_LS=0: three barriers per layer in the one-board resident tower
    int device = 0;

    ConvLayer stem;
    std::vector<std::unique_ptr<ConvLayer>> c1, c2;
    // heads: generic path keeps f32 [k][n]-transposed FC weights for the SIMT kernels; the tuned path
    // keeps K-contiguous, zero-padded matrices in the tower element type for the MFMA head GEMMs
    DevBuf head_w, head_b, w1t, b1, w2, b2, wpt, bp;
    uint32_t kvp = 0, kpp = 0;  // padded K of the value / policy FC (tuned path)

    // Two lanes = two independent sets of activation buffers, each with its own stream, so that two
    // host threads can have a batch in flight each: one lane's transfers, launch latency and completion
    // wake-up hide behind the other lane's kernels.  The weights are shared.
    Lane lanes[NLANES];
    std::atomic<unsigned> lane_rr{0};

    std::mutex stat_mu;
    cattus_stats stats{};
    uint64_t stats_tower_fallbacks = 0;  // batches the one-launch tower gave up on (run again on the per-layer launches)

    // cattus_hip_verify: every verify_every-th batch of eval_host (0: none) also runs on `shadow`, a dtype f32 evaluator of the same blob that this
    // one owns (built when verification is first turned on; its lane i is used under this evaluator's lane i mutex and by nobody else), and the two
    // outputs are compared on the device.  verify_every and the shadow change only with every lane mutex held; eval_host reads them holding one
    // (atomic for cattus_hip_verify_stats, which holds none).
    uint64_t blob_hash = 0;  // of the blob this evaluator was created from, which it keeps no host copy of
    size_t blob_bytes = 0;
    std::atomic<uint32_t> verify_every{0};
    std::atomic<uint64_t> verify_ticket{0};  // one per eval_host batch while verification is on: a batch is verified when ticket % verify_every == 0
    cattus_eval* shadow = nullptr;
    struct Verified {  // the sticky record, under stat_mu
        uint64_t batches = 0, leaves = 0, leaves_outside = 0;
        float max_dlogit = 0, logit = 0, logit_ref = 0, max_dvalue = 0, value = 0, value_ref = 0;
        uint32_t move = 0;
        std::vector<uint64_t> worst_planes;  // of the leaf that holds max_dlogit; empty before any leaf was verified
    } verified;
    // the priors part of the sticky record (prior_rule.h; cattus_hip_verify_prior_stats), under stat_mu, and the leaf that holds its max_tv
    PriorStats priors;
    struct WorstPrior {
        std::vector<uint64_t> planes;
        std::vector<uint16_t> legal;  // the leaf's legal list, min(legal_count, legal_stride) entries
        uint32_t top = 0, top_ref = 0;
    } worst_prior;

    // leaf server
    std::mutex srv_mu;
    std::condition_variable srv_cv, done_cv;
    std::deque<std::unique_ptr<ServerBatch>> batches;  // oldest first; back() is collecting unless sealed
    uint64_t next_seq = 1;
    bool flush_req = false, stop = false;
    std::mutex ragged_mu;  // the one-time allocation of the lanes' ragged buffers
    std::atomic<bool> ragged_ready{false};
    std::thread servers[NLANES];  // one per lane: two sealed batches can be on the device together

    ~cattus_eval() {
        {
            std::lock_guard<std::mutex> lk(srv_mu);
            stop = true;
        }
        srv_cv.notify_all();
        done_cv.notify_all();
        for (auto& t : servers)
            if (t.joinable()) t.join();
        delete shadow;
    }
};

namespace {

size_t blob_floats(const cattus_net_desc& d) {
    const size_t hw = (size_t)d.board * d.board, F = d.filters;
    if (F == 0) {  // SimpleTwoHeadedModel: two K x K dense layers, a 1 x K and an M x K head
        const size_t K = (size_t)d.planes * hw;
        return 2 * (K * K + K) + K + 1 + (size_t)d.moves * K + d.moves;
    }
    size_t n = F * d.planes * 9 + 4 * F;
    n += (size_t)d.blocks * (2 * F * F * 9 + 6 * F);
    n += (size_t)d.vhc * F + 2 * (size_t)d.vhc + (size_t)FC_HIDDEN * d.vhc * hw + FC_HIDDEN + FC_HIDDEN + 1;
    n += (size_t)d.phc * F + 2 * (size_t)d.phc + (size_t)d.moves * d.phc * hw + d.moves;
    return n;
}

// 64 bits of the blob, FNV-1a taken over 8-byte words (a trailing partial word zero-padded): how cattus_hip_verify knows the blob it is handed
// for the one the evaluator was created from.  ~10 ms for chess 20x256's 95 MB, once per create.
uint64_t blob_hash64(const void* p, size_t nbytes) {
    uint64_t h = 0xcbf29ce484222325ull ^ nbytes;
    const char* c = static_cast<const char*>(p);
    for (size_t at = 0; at < nbytes; at += 8) {
        uint64_t w = 0;
        memcpy(&w, c + at, std::min<size_t>(8, nbytes - at));
        h = (h ^ w) * 0x100000001b3ull;
    }
    return h;
}

// Launches of the persistent tower never overlap on a device: each waits for the one before it (an event chain per device, process-wide:
// two evaluators -- model1 and model2 of a self-play round -- or the two lanes of one would otherwise share the CUs, neither launch
// would have all its workgroups resident, and each would wait for hand-offs from workgroups the other keeps out).  Other work of the
// lanes (copies, stem, heads) overlaps as before.
std::mutex g_chain_mu;
hipEvent_t g_chain[64] = {};
int chain_persistent_launch(int device, hipStream_t st, const std::function<void()>& launch) {
    std::lock_guard<std::mutex> lk(g_chain_mu);
    hipEvent_t& ev = g_chain[device & 63];
    if (!ev) {
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    } else {
        HIP_TRY(hipStreamWaitEvent(st, ev, 0));
    }
    launch();
    HIP_TRY(hipEventRecord(ev, st));
    return CATTUS_OK;
}

// Upload one folded 3x3 layer in the layout this evaluator's tower reads it in (weight_layout.h): L.w the weights, L.b the biases (f16 towers:
// [biases | inverse scales] of that layout's scaling).  The Winograd kinds run every layer behind the stem on U = G g G^T, kept in the arena.
int upload_conv(cattus_eval* e, ConvLayer& L, const Folded& f, uint32_t cout, uint32_t cin, bool stem = false) {
    auto up = [](DevBuf& buf, const auto& v, DevArena* arena = nullptr) { return buf.upload(v.data(), v.size() * sizeof(v[0]), arena); };
    int rc;
    if (!e->plan.tuned()) return (rc = up(L.b, f.b)) ? rc : up(L.w, f.w);
    const ConvShape s{cout, cin, e->fpad, stem ? e->cpad0 : e->fpad};
    if (e->plan.kind == TowerKind::WinoF4 && !stem) {
        std::vector<int> sh;
        const std::vector<double> U = winof4_transform(f, s, &sh);
        if ((rc = up(L.b, bias_and_scales(f, s, &sh)))) return rc;
        return up(L.w, winof4_u(U, s, sh), &e->arena);
    }
    if (e->plan.wino() && !stem) {
        std::vector<int> sh;  // wino_transform's per-channel scale: the f16 kinds' (WinoF32 takes U unscaled and the biases alone)
        const std::vector<double> U = wino_transform(f, s, &sh);
        const bool f32w = e->plan.kind == TowerKind::WinoF32;
        if ((rc = up(L.b, bias_and_scales(f, s, f32w ? nullptr : &sh)))) return rc;
        if (f32w) return up(L.w, wino_u_f32(U, s), &e->arena);
        if (e->plan.kind == TowerKind::WinoF16) return up(L.w, wino_u_f16(U, s, sh), &e->arena);
        return up(L.w, wino_u(U, s, sh), &e->arena);
    }
    const bool scaled = act_f16_family(e->act);
    const std::vector<int> sh = scaled ? channel_shifts(f, s) : std::vector<int>();
    if ((rc = up(L.b, bias_and_scales(f, s, scaled ? &sh : nullptr)))) return rc;
    if (e->act == Act::F32) return up(L.w, rows_f32(f, s));
    if (e->act == Act::BF16) return up(L.w, rows_bf16(f, s));
    if (e->act == Act::F16) return up(L.w, rows_f16(f, s, sh));
    return e->plan.w_frag ? up(L.w, frag_f16x2(f, s, sh)) : up(L.w, rows_f16x2(f, s, sh));
}

// What a lane has whichever tower runs: its stream and event, a batch's planes, logits and values on the device and in page-locked memory.
int lane_common(cattus_eval* e, Lane& L) {
    const size_t B = e->cfg.max_batch, M = e->d.moves, plane_bytes = B * e->d.planes * e->cfg.plane_words * 8;
    int rc;
    HIP_TRY(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&L.done, hipEventBlockingSync | hipEventDisableTiming));
    if ((rc = L.d_planes.alloc(plane_bytes)) || (rc = L.d_policy.alloc(B * M * 4)) || (rc = L.d_value.alloc(B * 4))) return rc;
    if ((rc = L.h_planes.alloc(plane_bytes)) || (rc = L.h_policy.alloc(B * M * 4)) || (rc = L.h_value.alloc(B * 4))) return rc;
    return CATTUS_OK;
}

// leaf capacity of the tuned heads' activation buffer (HeadsMfma::hv): whole 32-leaf tiles
uint32_t hv_leaves(const cattus_eval* e) { return (e->bpad + 31) / 32 * 32; }

// SimpleTwoHeadedModel: weights transposed to [k][n] (coalesced along n in the dense kernel), buffers for the planes tensor
// and the two hidden layers.
int build_simple(cattus_eval* e, const float* p) {
    const cattus_net_desc& d = e->d;
    const size_t K = (size_t)d.planes * e->hw, M = d.moves, B = e->cfg.max_batch;
    auto upload_t = [&](DevBuf& buf, const float* w, size_t n_out) -> int {
        std::vector<float> t(K * n_out);
        for (size_t n = 0; n < n_out; n++)
            for (size_t k = 0; k < K; k++) t[k * n_out + n] = w[n * K + k];
        return buf.upload(t.data(), t.size() * 4);
    };
    int rc;
    const float *w1 = p, *b1 = w1 + K * K, *w2 = b1 + K, *b2 = w2 + K * K, *vw = b2 + K, *vb = vw + K, *pw = vb + 1, *pb = pw + M * K;  // blob order
    if ((rc = upload_t(e->d1w, w1, K)) || (rc = e->d1b.upload(b1, K * 4)) || (rc = upload_t(e->d2w, w2, K)) || (rc = e->d2b.upload(b2, K * 4)) ||
        (rc = upload_t(e->svw, vw, 1)) || (rc = e->svb.upload(vb, 4)) || (rc = upload_t(e->spw, pw, M)) || (rc = e->spb.upload(pb, M * 4)))
        return rc;
    for (Lane& L : e->lanes)
        if ((rc = lane_common(e, L)) || (rc = L.x0.alloc(B * K * 4)) || (rc = L.a.alloc(B * K * 4)) || (rc = L.t.alloc(B * K * 4))) return rc;
    return CATTUS_OK;
}

int build(cattus_eval* e, const float* p, const Calibration* cal) {
    const cattus_net_desc& d = e->d;
    const TowerPlan& plan = e->plan;
    if (plan.kind == TowerKind::Simple) return build_simple(e, p);
    const uint32_t F = d.filters, hw = e->hw, FP = e->fpad;
    auto take = [&](size_t n) { return (p += n) - n; };  // the next n floats of the blob
    int rc;
    e->stream_shifts.assign(F, 0);
    if (act_f16_family(e->act) && e->stream_shift_on) {
        // (the F(4x4) form's cap is 25x tighter: its headroom is a quarter of that cap, as the default is of the F(2x2) form's)
        const double headroom = plan.kind == TowerKind::WinoF4 ? WINOF4_CAL_HEADROOM : STREAM_CAL_HEADROOM;
        // (the f16w tower's stream is f32: calibrated, it keeps the estimate's shifts and takes the measured guard alone -- weight_layout.h;
        // so does the f16r tower, whose stream is f32 as well: its shifts serve the f16 operand copy, and a seeded net keeps its shifts and bits)
        if (cal && (plan.kind == TowerKind::WinoF16 || plan.f32_stream()))
            e->stream_shifts = calibrated_stream_shifts_f32_stream(choose_stream_shift(d, p, &e->stream_shift, STREAM_NO_CEILING), cal->abs_max, headroom);
        else if (cal) e->stream_shifts = calibrated_stream_shifts(cal->s2, cal->abs_max, headroom), e->stream_shift = stream_shift_global(cal->s2);
        else e->stream_shifts = choose_stream_shift(d, p, &e->stream_shift, plan.kind == TowerKind::WinoF4 ? WINOF4_STREAM_CEILING : STREAM_NO_CEILING);
    }
    const std::vector<int>& tk = e->stream_shifts;
    const bool shifted = std::any_of(tk.begin(), tk.end(), [](int t) { return t != 0; });
    {
        const float* w = take((size_t)F * d.planes * 9);
        const float *g = take(F), *be = take(F), *mu = take(F), *var = take(F);
        Folded f = fold_conv(w, F, d.planes, 9, g, be, mu, var);
        if (shifted) shift_folded(f, d.planes, tk, true);
        if ((rc = upload_conv(e, e->stem, f, F, d.planes, true))) return rc;
    }
    for (uint32_t i = 0; i < d.blocks; i++) {
        e->c1.emplace_back(new ConvLayer);
        e->c2.emplace_back(new ConvLayer);
        const float* w1 = take((size_t)F * F * 9);
        const float *mu1 = take(F), *var1 = take(F);
        Folded f1 = fold_conv(w1, F, F, 9, nullptr, nullptr, mu1, var1);
        if (shifted) shift_folded(f1, F, tk, false);
        if ((rc = upload_conv(e, *e->c1.back(), f1, F, F))) return rc;
        const float* w2 = take((size_t)F * F * 9);
        const float *g2 = take(F), *be2 = take(F), *mu2 = take(F), *var2 = take(F);
        Folded f2 = fold_conv(w2, F, F, 9, g2, be2, mu2, var2);
        if (shifted) shift_folded(f2, F, tk, true);
        if ((rc = upload_conv(e, *e->c2.back(), f2, F, F))) return rc;
    }
    // heads: value rows first, then policy rows, in one [vhc+phc][F] 1x1 conv
    std::vector<float> hw_w((size_t)(d.vhc + d.phc) * F), hw_b(std::max(32u, d.vhc + d.phc), 0.0f);  // bias padded to one 32-row tile
    const float* vw = take((size_t)d.vhc * F);
    const float *vmu = take(d.vhc), *vvar = take(d.vhc);
    Folded fv = fold_conv(vw, d.vhc, F, 1, nullptr, nullptr, vmu, vvar);
    const float* fc1_w = take((size_t)FC_HIDDEN * d.vhc * hw);
    const float* fc1_b = take(FC_HIDDEN);
    const float* fc2_w = take(FC_HIDDEN);
    const float* fc2_b = take(1);
    const float* pw = take((size_t)d.phc * F);
    const float *pmu = take(d.phc), *pvar = take(d.phc);
    Folded fp = fold_conv(pw, d.phc, F, 1, nullptr, nullptr, pmu, pvar);
    const float* pfc_w = take((size_t)d.moves * d.phc * hw);
    const float* pfc_b = take(d.moves);
    if (shifted) shift_folded(fv, F, tk, false), shift_folded(fp, F, tk, false);  // f32 rows on every path that runs an f16 tower (head_act)
    memcpy(hw_w.data(), fv.w.data(), fv.w.size() * 4);
    memcpy(hw_w.data() + fv.w.size(), fp.w.data(), fp.w.size() * 4);
    memcpy(hw_b.data(), fv.b.data(), fv.b.size() * 4);
    memcpy(hw_b.data() + fv.b.size(), fp.b.data(), fp.b.size() * 4);
    const uint32_t kv = d.vhc * hw, kp = d.phc * hw;
    if ((rc = e->head_b.upload(hw_b.data(), hw_b.size() * 4)) || (rc = e->b1.upload(fc1_b, FC_HIDDEN * 4)) || (rc = e->w2.upload(fc2_w, FC_HIDDEN * 4)) ||
        (rc = e->b2.upload(fc2_b, 4)) || (rc = e->bp.upload(pfc_b, d.moves * 4)))
        return rc;
    if (plan.tuned()) {
        // K-contiguous matrices, K padded to 16 with zeros (zero terms do not change an fmaf chain)
        const uint32_t ocn = d.vhc + d.phc;
        e->kvp = (kv + 15) / 16 * 16;
        e->kpp = (kp + 15) / 16 * 16;
        const uint32_t m32 = (d.moves + 31) / 32 * 32;
        std::vector<float> cw((size_t)32 * FP, 0.0f), w1((size_t)FC_HIDDEN * e->kvp, 0.0f), wp((size_t)m32 * e->kpp, 0.0f);
        for (uint32_t oc = 0; oc < ocn; oc++) memcpy(&cw[(size_t)oc * FP], &hw_w[(size_t)oc * F], (size_t)F * 4);
        for (uint32_t j = 0; j < FC_HIDDEN; j++) memcpy(&w1[(size_t)j * e->kvp], &fc1_w[(size_t)j * kv], kv * 4);
        for (uint32_t m = 0; m < d.moves; m++) memcpy(&wp[(size_t)m * e->kpp], &pfc_w[(size_t)m * kp], kp * 4);
        const Act hact = head_act(e->act);  // the split tower's heads run in exact f32 on the last layer's f32 rows
        auto upload_t = [&](DevBuf& buf, const std::vector<float>& v) -> int {
            if (hact == Act::F32) return buf.upload(v.data(), v.size() * 4);
            std::vector<uint16_t> hb(v.size());
            for (size_t i = 0; i < v.size(); i++) hb[i] = f32_to_bf16(v[i]);
            return buf.upload(hb.data(), hb.size() * 2);
        };
        // the FC weights go up in MFMA fragment order (kernels.h, HeadsMfma): a wave's operand of one k-step is one KiB
        auto frag_order = [&](const std::vector<float>& v, uint32_t rows, uint32_t K) {
            const uint32_t kstep = hact == Act::F32 ? 8 : 16, half = kstep / 2;
            std::vector<float> o(v.size());
            for (uint32_t row = 0; row < rows; row++)
                for (uint32_t k = 0; k < K; k++)
                    o[((((size_t)(row >> 5) * (K / kstep) + k / kstep) * 2 + (k % kstep) / half) * 32 + (row & 31)) * half + k % half] =
                        v[(size_t)row * K + k];
            return o;
        };
        if ((rc = upload_t(e->head_w, cw)) || (rc = upload_t(e->w1t, frag_order(w1, FC_HIDDEN, e->kvp))) || (rc = upload_t(e->wpt, frag_order(wp, m32, e->kpp)))) return rc;
    } else {
        std::vector<float> w1t((size_t)kv * FC_HIDDEN), wpt((size_t)kp * d.moves);
        for (uint32_t j = 0; j < FC_HIDDEN; j++)
            for (uint32_t k = 0; k < kv; k++) w1t[(size_t)k * FC_HIDDEN + j] = fc1_w[(size_t)j * kv + k];
        for (uint32_t m = 0; m < d.moves; m++)
            for (uint32_t k = 0; k < kp; k++) wpt[(size_t)k * d.moves + m] = pfc_w[(size_t)m * kp + k];
        if ((rc = e->head_w.upload(hw_w.data(), hw_w.size() * 4)) || (rc = e->w1t.upload(w1t.data(), w1t.size() * 4)) || (rc = e->wpt.upload(wpt.data(), wpt.size() * 4))) return rc;
        e->kvp = kv, e->kpp = kp;
    }

    // the resident towers' layer tables: stem, then (conv1, conv2 + skip) per block
    auto layer_table = [&](auto row) {
        std::vector<decltype(row(e->stem, 0, true))> tl{row(e->stem, 0, true)};
        for (uint32_t i = 0; i < d.blocks; i++) tl.push_back(row(*e->c1[i], 0, false)), tl.push_back(row(*e->c2[i], 1, false));
        return tl;
    };
    if (plan.kind == TowerKind::Resident64) {
        const auto tl = layer_table([](const ConvLayer& c, int res, bool) { return Tower64Layer{c.w.p, c.b.as<float>(), res, 0}; });
        if ((rc = e->t64_layers.upload(tl.data(), tl.size() * sizeof(Tower64Layer)))) return rc;
    }
    if (plan.kind == TowerKind::Resident64Stream) {  // t64r_rule.h's table: the skip flag per layer (the last-layer flag follows from nlayers)
        std::vector<Tower64Layer> tl;
        for (uint32_t l = 0; l < t64r_layers(d.blocks); l++) {
            const ConvLayer& c = l == 0 ? e->stem : (l & 1) ? *e->c1[(l - 1) / 2] : *e->c2[(l - 1) / 2];
            tl.push_back(Tower64Layer{c.w.p, c.b.as<float>(), t64r_layer(l, d.blocks).skip ? 1 : 0, 0});
        }
        if ((rc = e->t64_layers.upload(tl.data(), tl.size() * sizeof(Tower64Layer)))) return rc;
    }
    if (plan.kind == TowerKind::Resident64F32) {  // t64f_rule.h's table: dtype f32's rows and biases, the skip flag per layer
        std::vector<Tower64Layer> tl;
        for (uint32_t l = 0; l < t64f_layers(d.blocks); l++) {
            const ConvLayer& c = l == 0 ? e->stem : (l & 1) ? *e->c1[(l - 1) / 2] : *e->c2[(l - 1) / 2];
            tl.push_back(Tower64Layer{c.w.p, c.b.as<float>(), t64f_layer(l, d.blocks).skip ? 1 : 0, 0});
        }
        if ((rc = e->t64_layers.upload(tl.data(), tl.size() * sizeof(Tower64Layer)))) return rc;
    }
    if (plan.kind == TowerKind::Resident64Split) {
        const auto tl = layer_table([](const ConvLayer& c, int res, bool stem) { return Tower64SplitLayer{c.w.p, c.b.as<float>(), res, stem ? 1 : 2}; });
        if ((rc = e->t64_layers.upload(tl.data(), tl.size() * sizeof(Tower64SplitLayer)))) return rc;
        // every layer's [64 biases | 64 inverse scales] in one table (the kernel copies it to LDS with independent loads)
        if ((rc = e->t64s_bias.alloc(tl.size() * 512))) return rc;
        for (size_t l = 0; l < tl.size(); l++)
            HIP_TRY(hipMemcpy((char*)e->t64s_bias.p + l * 512, tl[l].bias, 512, hipMemcpyDeviceToDevice));
    }

    // activations
    const bool tuned = plan.tuned();
    // bytes per channel of the tower buffers; the f16 towers' last layer writes f32 rows into one of them
    const size_t bpad = e->bpad, esz = tuned ? (act_f16_family(e->act) ? 4 : (size_t)act_bytes(e->act)) : 4;
    const size_t hesz = tuned ? (size_t)act_bytes(head_act(e->act)) : 4;  // element of the head activations
    const size_t slots = tuned ? e->slots : hw;
    for (Lane& L : e->lanes) {
        const size_t act_bytes_ = bpad * slots * FP * esz, hv_bytes = (size_t)(tuned ? hv_leaves(e) : bpad) * (e->kvp + e->kpp) * hesz;
        if ((rc = lane_common(e, L)) || (rc = L.x0.alloc(bpad * slots * e->cpad0 * esz)) || (rc = L.a.alloc(act_bytes_, &e->arena)) ||
            (rc = L.t.alloc(act_bytes_, &e->arena)) || (rc = L.y.alloc(act_bytes_, plan.inplace ? nullptr : &e->arena)) ||  // in place: the Winograd tower does not touch y
            (rc = L.hv.alloc(hv_bytes)) || (rc = L.h1.alloc(bpad * FC_HIDDEN * 4)))
            return rc;
        HIP_TRY(hipMemset(L.hv.p, 0, hv_bytes));  // pad columns (and leaves never written) must read as zero
        if (plan.one_launch) {
            // the lane's layer table: conv1 of a block a -> t, conv2 t -> a over its own skip rows (the per-layer launches' in-place plan)
            std::vector<Wino4TowerLayer> tl;
            float *la = L.a.as<float>(), *lt = L.t.as<float>();
            for (uint32_t i = 0; i < d.blocks; i++) {
                tl.push_back(Wino4TowerLayer{la, e->c1[i]->w.p, e->c1[i]->b.as<float>(), nullptr, lt});
                tl.push_back(Wino4TowerLayer{lt, e->c2[i]->w.p, e->c2[i]->b.as<float>(), la, la});
            }
            if ((rc = L.tower_layers.upload(tl.data(), tl.size() * sizeof(Wino4TowerLayer))) || (rc = L.tower_ready.alloc(64 + (size_t)tl.size() * (bpad / 4) * 4)) ||
                (rc = L.h_tower_err.alloc(4)))
                return rc;
            *L.h_tower_err.as<unsigned>() = 0;
        }
    }
    return CATTUS_OK;
}

struct TowerTimer { std::vector<hipEvent_t> ev; size_t used = 0; };  // event pairs (start, stop) and how many events a pass has taken

// The two decisions about the one-launch Winograd tower that are taken per batch: the sticky demotion after a hand-off wait gave up, and whether
// the grid of a batch of nb boards fits the device.  Both ways of launching give the same bits: a leaf's result still does not depend on its batch.
bool one_launch_now(const cattus_eval* e, uint32_t nb) {
    return e->plan.one_launch && !e->tower_gave_up.load(std::memory_order_relaxed) && wino4_tower_fits(nb, e->fpad, e->cus);
}

// What cattus_hip_stream_range, cattus_hip_tap and cattus_hip_trace hang behind the layers of a pass.  It is called while the pass is being
// enqueued, behind every conv layer of the tower and behind the head convs, with the point (include/cattus_hip.h: 0 the stem, 2i + 1 and 2i + 2
// block i's two convs, the last one the heads), the buffer that layer wrote and where an element lives in it (tap_layout.h); what it enqueues
// on the pass's stream runs before the next layer overwrites anything.  A pass with an observer runs the per-layer form of its plan's
// arithmetic -- the resident towers Forward::per_layer on the same ConvLayer buffers, the one-launch Winograd tower its per-layer launches:
// the same bits (tests/test_tower_plan_gpu.py, tests/test_trace_gpu.py).  Every other call passes none and enqueues what it always did.
using Observer = std::function<int(uint32_t point, const void* buf, const TapSource& src)>;

uint32_t net_points(const cattus_net_desc& d) { return 2 + 2 * d.blocks; }

// One forward pass being enqueued on `st`: n leaves whose planes are at d_planes (nb boards with the tower's padding), logits and values to
// d_policy / d_value.  One function per TowerKind; a tower returns its output rows, or nullptr where it has run the head convs itself.
struct Forward {
    cattus_eval* e;
    Lane& L;
    const uint64_t* d_planes;
    uint32_t n, nb;
    float *d_policy, *d_value;
    hipStream_t st;
    TowerTimer* tt;
    const Observer* obs;  // nullptr on every call but cattus_hip_stream_range, cattus_hip_tap and cattus_hip_trace
    int orc = CATTUS_OK;  // the first failure an observer reported
    const cattus_net_desc& d = e->d;
    const uint32_t w64 = e->cfg.plane_words, S = d.board, F = d.filters, FP = e->fpad;
    float *a = L.a.as<float>(), *t = L.t.as<float>(), *y = L.y.as<float>();

    void seen(uint32_t point, const void* buf, const TapSource& src) {
        if (!obs) return;
        const int rc = (*obs)(point, buf, src);
        if (rc && !orc) orc = rc;
    }
    // where tower layer l (the point of the same number) keeps its output: NCHW on the generic path; on the tuned ones rows in the tower's
    // element type, except that the Winograd tower keeps f32 rows throughout and the f16 towers' last layer writes f32 rows for the heads
    TapSource tower_source(uint32_t l) const {
        TapSource s{};
        s.C = F, s.hw = e->hw, s.slots = e->slots, s.pitch = FP;
        if (!e->plan.tuned()) s.layout = TAP_NCHW_F32;
        else if (e->plan.f32_stream()) return f16r_tap_source(l, F, e->hw, e->slots, FP);
        else if (e->plan.wino()) s.layout = TAP_ROWS_WINO_F32;
        else if (e->act == Act::F32 || (act_f16_family(e->act) && l == 2 * d.blocks)) s.layout = TAP_ROWS_F32;
        else s.layout = e->act == Act::BF16 ? TAP_ROWS_BF16 : e->act == Act::F16 ? TAP_ROWS_F16 : TAP_ROWS_F16X2;
        return s;
    }
    // the head convs' output: [leaf][(vhc + phc) * hw] on the generic path, HeadsMfma::hv's two fragment-ordered matrices on the tuned ones
    TapSource head_source() const {
        TapSource s{};
        s.C = d.vhc + d.phc, s.hw = e->hw, s.layout = TAP_NCHW_F32;
        if (!e->plan.tuned()) return s;
        s.layout = head_act(e->act) == Act::BF16 ? TAP_HV_BF16 : TAP_HV_F32;
        s.vhc = d.vhc, s.kvp = e->kvp, s.kpp = e->kpp, s.hv_pol = hv_leaves(e) * e->kvp;
        return s;
    }

    // with `tt` (a timing pass) each tower launch gets its own (start, stop) event pair stamped by the kernel itself
    hipEvent_t ev() { return tt && tt->used < tt->ev.size() ? tt->ev[tt->used++] : nullptr; }

    // SimpleTwoHeadedModel.forward (net_utils.py:112-121): flatten -> dense + ReLU -> dense + ReLU -> value: dense + tanh,
    // policy: dense + the non-finite scrub of net/mod.rs:56-61
    void simple() {
        const uint32_t K = d.planes * e->hw;
        launch_planes_to_tensor_nchw(d_planes, n, d.planes, w64, S, n, L.x0.as<float>(), st);
        launch_dense(L.x0.as<float>(), K, e->d1w.as<float>(), e->d1b.as<float>(), n, K, K, a, 1, st);
        launch_dense(a, K, e->d2w.as<float>(), e->d2b.as<float>(), n, K, K, t, 1, st);
        launch_dense(t, K, e->svw.as<float>(), e->svb.as<float>(), n, K, 1, d_value, 2, st);
        launch_dense(t, K, e->spw.as<float>(), e->spb.as<float>(), n, K, d.moves, d_policy, 0, st);
    }

    const void* generic() {
        launch_planes_to_tensor_nchw(d_planes, n, d.planes, w64, S, n, L.x0.as<float>(), st);
        auto conv = [&](const ConvLayer& c, const float* in, uint32_t cin, const float* res, float* out) {
            hipEvent_t s0 = ev(), s1 = ev();
            launch_conv3x3_generic(in, c.w.as<float>(), c.b.as<float>(), res, out, n, cin, F, S, st, s0, s1);
        };
        conv(e->stem, L.x0.as<float>(), d.planes, nullptr, a);
        seen(0, a, tower_source(0));
        for (uint32_t i = 0; i < d.blocks; i++) {
            conv(*e->c1[i], a, F, nullptr, t);
            seen(2 * i + 1, t, tower_source(2 * i + 1));
            conv(*e->c2[i], t, F, a, y);
            std::swap(a, y);
            seen(2 * i + 2, a, tower_source(2 * i + 2));
        }
        return a;
    }

    // the arguments the two resident towers share: the network, and the head convs fused on the resident output
    template <class Args>
    void resident_args(Args& ta, bool fuse_heads) {
        ta.planes = d_planes, ta.layers = (decltype(ta.layers))e->t64_layers.p;
        ta.n = n, ta.C = d.planes, ta.w64 = w64, ta.S = S, ta.nlayers = 1 + 2 * d.blocks;
        if (!fuse_heads) return;
        ta.head_w = (decltype(ta.head_w))e->head_w.p, ta.hv = (decltype(ta.hv))L.hv.p;  // bf16 tower: bf16 behind void*; split tower: float*
        ta.head_b = e->head_b.as<float>();
        ta.hv_pol = hv_leaves(e) * e->kvp, ta.kvp = e->kvp, ta.kpp = e->kpp, ta.vhc = d.vhc, ta.ocn = d.vhc + d.phc;
    }

    // cattus_hip_fused_heads on this pass (an observed pass never gets here: it runs the per-layer twin): the HEADS instance of the plan's
    // resident kernel writes hv itself, so the pass fills the head convs' arguments, counts, and hands heads_mfma no tower
    bool fuse_heads_now() {
        if (obs || tt || !e->fused_heads.load(std::memory_order_relaxed)) return false;
        e->fused_heads_batches.fetch_add(1, std::memory_order_relaxed);
        return true;
    }

    // bf16: the head convs fused, nullptr; f16: the tower's output as plain f32 rows in `a` for the f32 head kernels (fused_heads: as bf16)
    // 128-row workgroups; for 64-slot boards one board per workgroup while that leaves no CU with two of them
    int resident64_ch(uint32_t rows) const {
        if (e->t64_force_ch) return e->t64_force_ch == 4 && e->slots == 64 ? 4 : 2;  // A/B runs, the row-split test
        return e->slots == 64 && rows / 64 <= 256 ? 4 : 2;
    }

    const void* resident64() {
        Tower64Args ta{};
        const bool f16 = e->act == Act::F16, fuse = f16 && fuse_heads_now();
        resident_args(ta, !f16 || fuse);
        if (f16) ta.out = fuse ? nullptr : a, ta.sat = e->conv_opts.saturated;
        const uint32_t rows = nb * e->slots;
        hipEvent_t s0 = ev(), s1 = ev();
        launch_tower64(e->act, ta, rows, resident64_ch(rows), e->t64_layer_steps, st, s0, s1);
        return ta.out;  // (bf16: none asked for)
    }

    // dtype f16r_resident: the tower's output, the f32 stream behind the last layer, as plain f32 rows in the stream's buffer for the f32 head kernels
    const void* resident64_stream() {
        void* const buf[3] = {L.a.p, L.t.p, L.y.p};
        Tower64Args ta{};
        const bool fuse = fuse_heads_now();
        resident_args(ta, fuse);
        ta.out = fuse ? nullptr : buf[f16r_head_input()], ta.sat = e->conv_opts.saturated;
        const uint32_t rows = nb * e->slots;
        hipEvent_t s0 = ev(), s1 = ev();
        launch_tower64_stream(ta, rows, resident64_ch(rows), e->t64_layer_steps, st, s0, s1);
        return ta.out;
    }

    // dtype f32_resident: the tower's output as the plain f32 rows the per-layer f32 tower leaves, in `a`, for the f32 head kernels
    const void* resident64_f32() {
        Tower64F32Args ta{};
        ta.planes = d_planes, ta.layers = e->t64_layers.as<Tower64Layer>(), ta.out = a;
        ta.n = n, ta.C = d.planes, ta.w64 = w64, ta.S = S, ta.nlayers = t64f_layers(d.blocks);
        ta.nch = (uint32_t)t64f_hidden_chunks(F, e->t64f_narrow);
        const uint32_t rows = nb * e->slots;
        hipEvent_t s0 = ev(), s1 = ev();
        launch_tower64_f32(ta, rows, t64f_ch(rows / e->slots, e->slots, e->t64_force_ch), st, s0, s1);
        return ta.out;
    }

    // CATTUS_T64S_HEADS=0: the tower's output as plain f32 rows in `a` for the f32 head kernels
    const void* resident64_split() {
        Tower64SplitArgs ta{};
        resident_args(ta, e->t64s_fuse_heads);
        ta.sat = e->conv_opts.saturated, ta.bias_all = e->t64s_bias.as<float>();
        if (!e->t64s_fuse_heads) ta.out = a;
        hipEvent_t s0 = ev(), s1 = ev();
        launch_tower64_split(ta, nb * e->slots, e->t64s_depth, st, s0, s1);
        return ta.out;
    }

    // One direct conv layer of the MFMA tower; `stem`: from the planes (the stem conv expands them itself when they fit one 128-byte
    // chunk -- every game here -- else K0 packs them into x0 first and the stem is an ordinary layer of cpad0 input channels)
    void conv_mfma(const ConvLayer& c, const void* in, const void* res, void* out, int flags, bool stem = false) {
        const bool fused_stem = stem && stem_is_fused(d.planes, e->pack_separately);
        const StemInput stem_in{d_planes, n, d.planes, w64};
        if (stem && !fused_stem) launch_pack_planes_nhwc(e->act, d_planes, n, nb, d.planes, w64, S, e->cpad0, L.x0.p, st);
        hipEvent_t s0 = ev(), s1 = ev();
        launch_conv3x3_mfma(e->act, in, c.w.p, c.b.as<float>(), res, out, nb, stem ? e->cpad0 : FP, FP, S, st, s0, s1, fused_stem ? &stem_in : nullptr,
                            (e->plan.w_frag ? CONV_W_FRAG : 0) | flags, e->conv_opts);
    }

    // Layer l of the per-layer tower -- 0: the stem; 2i + 1: block i's conv1, a -> t; 2i + 2: its conv2 + skip, t -> y, which becomes a --
    // in layer order; returns the buffer it wrote.  (cattus_hip_trace steps the shadow's pass through this, one layer per point.)
    // One layer behind the stem of the split-K direct tower: conv_mfma's arguments, the split-K launcher
    void conv_splitk(const ConvLayer& c, const void* in, const void* res, void* out, int flags) {
        hipEvent_t s0 = ev(), s1 = ev();
        launch_conv3x3_splitk(in, c.w.p, c.b.as<float>(), res, out, nb, FP, FP, S, st, s0, s1, flags, e->splitk_forced, e->conv_opts.saturated);
    }

    const void* per_layer_step(uint32_t l) {
        const int last_flags = act_f16_family(e->act) && l == 2 * d.blocks ? CONV_OUT_F32 : 0;  // the f16 towers hand the f32 head kernels plain f32 rows
        if (l == 0) {
            conv_mfma(e->stem, L.x0.p, nullptr, a, last_flags, true);
            return a;
        }
        const uint32_t i = (l - 1) / 2;
        const bool sk = e->plan.kind == TowerKind::DirectSplitK;
        if (l & 1) {
            if (sk) conv_splitk(*e->c1[i], a, nullptr, t, 0);
            else conv_mfma(*e->c1[i], a, nullptr, t, 0);
            return t;
        }
        if (sk) conv_splitk(*e->c2[i], t, a, y, last_flags);
        else conv_mfma(*e->c2[i], t, a, y, last_flags);
        std::swap(a, y);
        return a;
    }

    const void* per_layer() {
        for (uint32_t l = 0; l <= 2 * d.blocks; l++) seen(l, per_layer_step(l), tower_source(l));
        return a;
    }

    // dtype f16r: layer l of f16r_rule.h's plan -- the stem and every conv2 on the stream kernel (S in f32, updated in place, and its f16
    // operand copy A), every conv1 on dtype f16's layer (A -> M); the buffers' roles never move, so a layer is a function of l alone
    const void* per_layer_stream_step(uint32_t l) {
        void* const buf[4] = {L.a.p, L.t.p, L.y.p, L.x0.p};  // F16R_BUF_A, _T, _Y, _X0
        const F16rLayer fl = f16r_layer(l, d.blocks);
        const ConvLayer& c = l == 0 ? e->stem : (l & 1) ? *e->c1[(l - 1) / 2] : *e->c2[(l - 1) / 2];
        if (!f16r_stream_layer(l)) {
            conv_mfma(c, buf[fl.reads], nullptr, buf[fl.writes], 0);
            return buf[fl.writes];
        }
        const bool stem = l == 0, fused_stem = stem && stem_is_fused(d.planes, e->pack_separately);
        const StemInput stem_in{d_planes, n, d.planes, w64};
        if (stem && !fused_stem) launch_pack_planes_nhwc(e->act, d_planes, n, nb, d.planes, w64, S, e->cpad0, L.x0.p, st);
        hipEvent_t s0 = ev(), s1 = ev();
        launch_conv3x3_f16r(buf[fl.reads], c.w.p, c.b.as<float>(), static_cast<float*>(buf[fl.writes]), fl.adds != F16R_NONE,
                            fl.writes_copy == F16R_NONE ? nullptr : buf[fl.writes_copy], nb, stem ? e->cpad0 : FP, FP, S, st, s0, s1,
                            fused_stem ? &stem_in : nullptr, f16r_is_last(l, d.blocks), e->conv_opts);
        return buf[fl.writes];
    }

    const void* per_layer_stream() {
        for (uint32_t l = 0; l < f16r_layers(d.blocks); l++) seen(l, per_layer_stream_step(l), tower_source(l));
        void* const buf[3] = {L.a.p, L.t.p, L.y.p};
        return buf[f16r_head_input()];
    }

    // Wino16 / Wino4 / WinoF4 / WinoF16 / WinoF32: the stem on the direct kernel (the split one, the f16 one under dtype f16w, the f32 one under f32w),
    // every layer behind it in Winograd form, f32 rows between the layers
    int wino() {
        const bool f4 = e->plan.kind == TowerKind::WinoF4, f32w = e->plan.kind == TowerKind::WinoF32;
        // (the f32 stem takes no flag: conv3x3_mfma_v2_kernel<float> writes plain f32 [row][cout] rows on 64-slot boards, the Winograd form's layout, and reads no flag)
        conv_mfma(e->stem, L.x0.p, nullptr, a, f32w ? 0 : CONV_OUT_F32 | (f4 ? CONV_WINOF4_IN : CONV_WINO_IN), true);
        seen(0, a, tower_source(0));
        const bool tail = !obs && e->tail_leaves && n <= e->tail_leaves;  // a short batch: the small-tile kernel, one launch per layer
        if (tail && !tt) e->tail_batches.fetch_add(1, std::memory_order_relaxed);  // (a timing pass is not a batch)
        if (!obs && !tail && one_launch_now(e, nb)) {
            // every layer behind the stem in ONE launch: counters and error word zeroed ahead of it on the same stream, the error word
            // copied to page-locked memory behind it (eval_host reads it when the batch is back; the device entry points at their next call)
            hipEvent_t s0 = ev(), s1 = ev();
            unsigned* const tower_err = L.tower_ready.as<unsigned>();
            HIP_TRY(hipMemsetAsync(L.tower_ready.p, 0, 64 + (size_t)2 * d.blocks * (nb / 4) * 4, st));
            if (int crc = chain_persistent_launch(e->device, st, [&] {
                    launch_tower_wino4(L.tower_layers.as<Wino4TowerLayer>(), 2 * d.blocks, tower_err + 16, tower_err, e->conv_opts.saturated, nb, FP,
                                       e->persist_spin, e->cus, st, s0, s1);
                }))
                return crc;
            HIP_TRY(hipMemcpyAsync(L.h_tower_err.p, tower_err, 4, hipMemcpyDeviceToHost, st));
            return CATTUS_OK;
        }
        const auto launch = f32w ? launch_conv3x3_wino_f32 : e->plan.kind == TowerKind::WinoF16 ? launch_conv3x3_wino_f16 : f4 ? launch_conv3x3_winof4 : tail ? launch_conv3x3_wino4s : e->plan.kind == TowerKind::Wino4 ? launch_conv3x3_wino4 : launch_conv3x3_wino;
        auto conv = [&](const ConvLayer& c, const float* in, const float* res, float* out) {
            hipEvent_t s0 = ev(), s1 = ev();
            launch(in, c.w.p, c.b.as<float>(), res, out, nb, FP, FP, st, s0, s1, e->conv_opts.saturated);
        };
        for (uint32_t i = 0; i < d.blocks; i++) {
            conv(*e->c1[i], a, nullptr, t);
            seen(2 * i + 1, t, tower_source(2 * i + 1));
            // in place: the block's output over its own skip rows -- the lane that adds a skip element writes that element, behind all its reads:
            // two activation buffers instead of three (33.6 instead of 50 MB per lane of what a pass drags through the Infinity Cache beside 168 MB of U)
            conv(*e->c2[i], t, a, e->plan.inplace ? a : y);
            if (!e->plan.inplace) std::swap(a, y);
            seen(2 * i + 2, a, tower_source(2 * i + 2));
        }
        return CATTUS_OK;
    }

    void heads_mfma(const void* tower) {
        HeadsMfma hd{};
        hd.conv_w = e->head_w.p, hd.conv_b = e->head_b.as<float>(), hd.hv = L.hv.p;
        hd.w1 = e->w1t.p, hd.b1 = e->b1.as<float>(), hd.h1 = L.h1.as<float>();
        hd.wp = e->wpt.p, hd.bp = e->bp.as<float>(), hd.policy = d_policy;
        hd.hw = e->hw, hd.vhc = d.vhc, hd.phc = d.phc, hd.kvp = e->kvp, hd.kpp = e->kpp, hd.M = d.moves;
        hd.w2 = e->w2.as<float>(), hd.b2 = e->b2.as<float>(), hd.value = d_value;
        hd.slots = e->slots, hd.hv_leaves = hv_leaves(e);
        const uint32_t chain_leaves = e->head_chain.load(std::memory_order_relaxed);
        if (!obs && !tt && chain_leaves && n <= chain_leaves) {  // the short-chain form of the f32 FC pair (head_chain_rule.h): the same bits
            e->head_chain_batches.fetch_add(1, std::memory_order_relaxed);
            launch_heads_chain(head_act(e->act), tower, n, FP, hd, st);
        } else {
            launch_heads_mfma(head_act(e->act), tower, n, FP, hd, st);
        }
        seen(net_points(d) - 1, L.hv.p, head_source());
    }

    void heads_generic(const void* tower) {
        const uint32_t hw = e->hw, kv = d.vhc * hw, kp = d.phc * hw;
        TowerView tv;
        tv.x = tower, tv.act = Act::F32, tv.sb = F * hw, tv.sk = hw, tv.sp = 1;
        launch_head_conv1x1(tv, e->head_w.as<float>(), e->head_b.as<float>(), n, F, d.vhc + d.phc, hw, L.hv.as<float>(), st);
        launch_value_fc1(L.hv.as<float>(), kv + kp, e->w1t.as<float>(), e->b1.as<float>(), n, kv, L.h1.as<float>(), st);
        launch_value_fc2_tanh(L.h1.as<float>(), e->w2.as<float>(), e->b2.as<float>(), n, d_value, st);
        launch_policy_fc(L.hv.as<float>(), kv + kp, kv, e->wpt.as<float>(), e->bp.as<float>(), n, kp, d.moves, d_policy, st);
        seen(net_points(d) - 1, L.hv.p, head_source());
    }
};

// boards of a pass of n leaves with the tower's padding: whole workgroups of the conv kernel on the tuned towers
uint32_t padded_boards(const cattus_eval* e, uint32_t n) {
    const uint32_t bpw = e->plan.tuned() ? ROWS_PER_WG / e->slots : 1;
    return (n + bpw - 1) / bpw * bpw;
}

int enqueue_forward(cattus_eval* e, Lane& L, const uint64_t* d_planes, uint32_t n, float* d_policy, float* d_value, hipStream_t st, TowerTimer* tt = nullptr,
                    const Observer* obs = nullptr) {
    Forward f{e, L, d_planes, n, padded_boards(e, n), d_policy, d_value, st, tt, obs};
    // observed: the resident towers' per-layer twin (upload_conv: one layout for both) -- the f32-stream one's is PerLayerStream
    switch (obs && e->plan.resident() ? (e->plan.f32_stream() ? TowerKind::PerLayerStream : TowerKind::PerLayer) : e->plan.kind) {
        case TowerKind::Simple: f.simple(); break;
        case TowerKind::Generic: f.heads_generic(f.generic()); break;
        case TowerKind::PerLayer: f.heads_mfma(f.per_layer()); break;
        case TowerKind::PerLayerStream: f.heads_mfma(f.per_layer_stream()); break;
        case TowerKind::DirectSplitK: f.heads_mfma(f.per_layer()); break;  // the stem through conv_mfma, every layer behind it through conv_splitk
        case TowerKind::Resident64: f.heads_mfma(f.resident64()); break;
        case TowerKind::Resident64Split: f.heads_mfma(f.resident64_split()); break;
        case TowerKind::Resident64Stream: f.heads_mfma(f.resident64_stream()); break;
        case TowerKind::Resident64F32: f.heads_mfma(f.resident64_f32()); break;
        case TowerKind::Wino16:
        case TowerKind::Wino4:
        case TowerKind::WinoF4:
        case TowerKind::WinoF16:
        case TowerKind::WinoF32:
            if (int rc = f.wino()) return rc;
            f.heads_mfma(f.a);
            break;
    }
    if (hipError_t err = hipGetLastError()) return fail(CATTUS_E_DEVICE, "kernel launch failed: %s", hipGetErrorString(err));
    return f.orc;
}

// seconds: of a batch whose wait was measured; nullptr: the counters alone (an asynchronous entry point measures no time).  verified: the batch
// also ran on the shadow tower (cattus_hip_verify) -- the caller did wait for that, so the total has it, but the average is the reference's
// model.run_duration, whose 0.99 weight makes it the last batch: a batch several times as long as its neighbours stays out of it.
void account(cattus_eval* e, uint32_t n, const double* seconds, bool verified = false) {
    std::lock_guard<std::mutex> lk(e->stat_mu);
    cattus_stats& s = e->stats;
    if (seconds) {
        // RunningAverage::set with epsilon 0.99, starting from 0 (reference: engine/src/util/metric.rs:1-20,
        // engine/src/net/mod.rs:36): value = (1 - eps) * value + eps * new
        if (!verified) s.run_seconds_ema = 0.01 * s.run_seconds_ema + 0.99 * *seconds;
        s.run_seconds_total += *seconds;
    }
    s.batches += 1;
    s.positions += n;
    if (n == e->cfg.max_batch) s.full_batches += 1;
}

// True: a one-launch tower on this lane reported that a hand-off wait ran out of its budget (its workgroups were not all resident: somebody else's
// kernels on this device) and finished on rows that were not ready.  Nothing of it is kept; every later batch takes the per-layer launches.
bool take_tower_give_up(cattus_eval* e, Lane& L) {
    if (!L.h_tower_err.p || *L.h_tower_err.as<volatile unsigned>() == 0) return false;
    *L.h_tower_err.as<volatile unsigned>() = 0;
    e->tower_gave_up.store(true, std::memory_order_relaxed);
    std::lock_guard<std::mutex> sl(e->stat_mu);
    e->stats_tower_fallbacks += 1;
    return true;
}

struct LegalArgs {
    const uint16_t* idx;  // [n][stride] policy indices of the legal moves
    const uint16_t* cnt;  // [n]
    uint32_t stride;
    float* probs;  // [n][stride]
    // The ragged form, a batch of the leaf server (legal_span.h): off [n + 1] is set, idx and probs hold off[n] entries back to back, cnt and stride
    // are not read.  kind [n]: 0 marks a plain leaf (an empty span that is no leaf of the prior statistics); logits: some leaf is plain, so the
    // logits come back too, into `policy`.
    const uint32_t* off = nullptr;
    const uint8_t* kind = nullptr;
    bool logits = false;
};

// A lane for one blocking call, locked: a free one if there is one, else queue on one of them in turn.
Lane& take_lane(cattus_eval* e, std::unique_lock<std::mutex>& lk) {
    for (Lane& cand : e->lanes) {
        std::unique_lock<std::mutex> tl(cand.mu, std::try_to_lock);
        if (tl.owns_lock()) {
            lk = std::move(tl);
            return cand;
        }
    }
    Lane& lane = e->lanes[e->lane_rr.fetch_add(1) % NLANES];
    lk = std::unique_lock<std::mutex>(lane.mu);
    return lane;
}

// A verified batch's n records, then its n details (kernels.h, launch_verify_outputs), into the sticky record, in leaf order.  The first
// verified leaf seeds the worst-logit entry, so that there are planes to ask for from then on; after that only a strictly larger difference
// replaces an entry: the first occurrence of a maximum stays.  A NaN |dvalue| (a non-finite value: its leaf is counted outside) replaces nothing.
void fold_verified(cattus_eval* e, const VerifyRecord* rec, uint32_t n, const uint64_t* planes) {
    const size_t words = (size_t)e->d.planes * e->cfg.plane_words;
    const float* detail = reinterpret_cast<const float*>(rec + n);
    std::lock_guard<std::mutex> lk(e->stat_mu);
    cattus_eval::Verified& v = e->verified;
    v.batches += 1;
    for (uint32_t i = 0; i < n; i++) {
        const float* dt = detail + (size_t)i * 4;
        v.leaves_outside += rec[i].flags & VERIFY_LEAF_OUTSIDE;
        if (v.worst_planes.empty() || rec[i].max_dlogit > v.max_dlogit) {
            v.max_dlogit = rec[i].max_dlogit, v.move = rec[i].move, v.logit = dt[0], v.logit_ref = dt[1];
            v.worst_planes.assign(planes + i * words, planes + (i + 1) * words);
        }
        if (rec[i].dvalue > v.max_dvalue) v.max_dvalue = rec[i].dvalue, v.value = dt[2], v.value_ref = dt[3];
    }
    v.leaves += n;
}

// The priors part of a verified batch, beside fold_verified and like it once per batch, in leaf order: the value pairs of every verified leaf
// (from the details of `rec`), and -- for a batch that came with legal moves -- its n prior records; the leaf that now holds max_tv leaves
// its planes, its legal list and both favourites.
void fold_priors(cattus_eval* e, const VerifyRecord* rec, uint32_t n, const uint64_t* planes, const PriorRecord* prior, const LegalArgs* lg) {
    const size_t words = (size_t)e->d.planes * e->cfg.plane_words;
    const float* detail = reinterpret_cast<const float*>(rec + n);
    std::lock_guard<std::mutex> lk(e->stat_mu);
    PriorStats& s = e->priors;
    for (uint32_t i = 0; i < n; i++) prior_fold_value(s, detail[(size_t)i * 4 + 2], detail[(size_t)i * 4 + 3]);
    if (!lg) {
        s.batches_without_legal += 1;
        return;
    }
    s.batches += 1;
    for (uint32_t i = 0; i < n; i++) {
        // a ragged batch (the leaf server's) folds its leaves in slot order with their own lists; its plain leaves fed the value part above
        if (lg->off && !lg->kind[i]) continue;
        if (!prior_fold(s, prior[i])) continue;
        cattus_eval::WorstPrior& w = e->worst_prior;
        w.planes.assign(planes + i * words, planes + (i + 1) * words);
        const uint16_t* list = lg->idx + (lg->off ? (size_t)legal_span(lg->off, i).begin : (size_t)i * lg->stride);
        w.legal.assign(list, list + prior[i].count);
        w.top = prior[i].top_a, w.top_ref = prior[i].top_b;
    }
}

// Blocking host-buffer evaluation; caller holds no lock.  With `lg` the logits stay on the device and
// the per-leaf softmax over the legal moves comes back instead (policy is not written).
int eval_host(cattus_eval* e, const uint64_t* planes, uint32_t n, float* policy, float* value, const LegalArgs* lg = nullptr) {
    const cattus_net_desc& d = e->d;
    std::unique_lock<std::mutex> lk;
    Lane& L = take_lane(e, lk);
    const RoctxRange range(lg ? "cattus_hip_eval_legal" : "cattus_hip_eval", n);
    HIP_TRY(hipSetDevice(e->device));
    const auto t0 = std::chrono::steady_clock::now();
    // cattus_hip_verify: while it is on every batch takes a ticket, and every verify_every-th one -- the first one first -- is checked
    const uint32_t every = e->verify_every.load(std::memory_order_relaxed);
    const bool verify = every && e->verify_ticket.fetch_add(1, std::memory_order_relaxed) % every == 0;
    const size_t pbytes = (size_t)n * d.planes * e->cfg.plane_words * 8;
    // Buffers obtained from cattus_hip_host_alloc are page-locked: DMA straight from / into them.
    // Anything else goes through the evaluator's own pinned staging buffers.
    const bool ragged = lg && lg->off, logits_out = !lg || lg->logits;
    const bool direct = is_pinned(planes) && (!logits_out || is_pinned(policy)) && is_pinned(value);
    const uint32_t rag_total = ragged ? lg->off[n] : 0;
    if (ragged) {
        // lists and offsets through the lane's page-locked staging, whatever the caller's memory is (the server's batches live in vectors)
        if (!L.rag_idx.p) return fail(CATTUS_E_STATE, "ragged batch before the lanes' ragged buffers exist");
        if (rag_total) memcpy(L.h_rag_idx.p, lg->idx, (size_t)rag_total * 2);
        memcpy(L.h_rag_off.p, lg->off, ((size_t)n + 1) * 4);
        if (verify && !L.rag_probs_ref.p)
            if (int arc = L.rag_probs_ref.alloc((size_t)e->cfg.max_batch * LEGAL_CAP * 4)) return arc;
    }
    if (lg && !ragged && (L.legal_stride < lg->stride || !L.d_probs.p)) {
        const size_t B = e->cfg.max_batch;
        int arc;
        if ((arc = L.d_legal_idx.alloc(B * lg->stride * 2)) || (arc = L.d_legal_cnt.alloc(B * 2)) ||
            (arc = L.d_probs.alloc(B * lg->stride * 4)))
            return arc;
        L.legal_stride = lg->stride;
    }
    if (lg && !ragged && verify && (L.prior_stride < lg->stride || !L.d_probs_ref.p)) {
        if (int arc = L.d_probs_ref.alloc((size_t)e->cfg.max_batch * lg->stride * 4)) return arc;
        L.prior_stride = lg->stride;
    }
    const void* src_planes = planes;
    if (!direct) {
        memcpy(L.h_planes.p, planes, pbytes);
        src_planes = L.h_planes.p;
    }
    HIP_TRY(hipMemcpyAsync(L.d_planes.p, src_planes, pbytes, hipMemcpyHostToDevice, L.stream));
    auto copy_out = [&]() -> int {
        if (ragged) {
            // the leaf server's batch: the lists go up, the ragged softmax runs on the logits where they are, and only the probabilities (and the
            // values, below) come back -- plus the logits where some leaf of the batch is a plain one
            const uint32_t* d_off = L.rag_off.as<uint32_t>();
            HIP_TRY(hipMemcpyAsync(L.rag_off.p, L.h_rag_off.p, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, L.stream));
            if (rag_total) HIP_TRY(hipMemcpyAsync(L.rag_idx.p, L.h_rag_idx.p, (size_t)rag_total * 2, hipMemcpyHostToDevice, L.stream));
            launch_legal_softmax_ragged(L.d_policy.as<float>(), d.moves, L.rag_idx.as<uint16_t>(), d_off, n, rag_total, L.rag_probs.as<float>(), L.stream);
            if (verify) {
                // as below: the shadow's logits through the same softmax with the same lists, the two sets of rows compared span by span
                Lane& SL = e->shadow->lanes[&L - e->lanes];
                launch_legal_softmax_ragged(SL.d_policy.as<float>(), d.moves, L.rag_idx.as<uint16_t>(), d_off, n, rag_total, L.rag_probs_ref.as<float>(), L.stream);
                launch_verify_priors(L.rag_probs.as<float>(), L.rag_probs_ref.as<float>(), nullptr, L.d_value.as<float>(), SL.d_value.as<float>(), n, 0,
                                     L.d_prior.as<PriorRecord>(), L.stream, d_off);
                HIP_TRY(hipMemcpyAsync(L.h_prior.p, L.d_prior.p, (size_t)n * sizeof(PriorRecord), hipMemcpyDeviceToHost, L.stream));
            }
            if (rag_total) HIP_TRY(hipMemcpyAsync(L.h_rag_probs.p, L.rag_probs.p, (size_t)rag_total * 4, hipMemcpyDeviceToHost, L.stream));
            if (logits_out) HIP_TRY(hipMemcpyAsync(direct ? (void*)policy : L.h_policy.p, L.d_policy.p, (size_t)n * d.moves * 4, hipMemcpyDeviceToHost, L.stream));
        } else if (lg) {
            HIP_TRY(hipMemcpyAsync(L.d_legal_idx.p, lg->idx, (size_t)n * lg->stride * 2, hipMemcpyHostToDevice, L.stream));
            HIP_TRY(hipMemcpyAsync(L.d_legal_cnt.p, lg->cnt, (size_t)n * 2, hipMemcpyHostToDevice, L.stream));
            if (launch_legal_softmax(L.d_policy.as<float>(), d.moves, L.d_legal_idx.as<uint16_t>(), L.d_legal_cnt.as<uint16_t>(),
                                     lg->stride, n, L.d_probs.as<float>(), L.stream))
                return fail(CATTUS_E_INVALID, "legal stride %u exceeds 1024", lg->stride);
            if (verify) {
                // the priors the exact network would have handed back for the same legal moves, and the two rows compared (prior_rule.h): behind
                // verify_outputs_kernel on this stream, into buffers of their own
                Lane& SL = e->shadow->lanes[&L - e->lanes];
                launch_legal_softmax(SL.d_policy.as<float>(), d.moves, L.d_legal_idx.as<uint16_t>(), L.d_legal_cnt.as<uint16_t>(), lg->stride, n,
                                     L.d_probs_ref.as<float>(), L.stream);
                launch_verify_priors(L.d_probs.as<float>(), L.d_probs_ref.as<float>(), L.d_legal_cnt.as<uint16_t>(), L.d_value.as<float>(),
                                     SL.d_value.as<float>(), n, lg->stride, L.d_prior.as<PriorRecord>(), L.stream);
                HIP_TRY(hipMemcpyAsync(L.h_prior.p, L.d_prior.p, (size_t)n * sizeof(PriorRecord), hipMemcpyDeviceToHost, L.stream));
            }
            HIP_TRY(hipMemcpyAsync(lg->probs, L.d_probs.p, (size_t)n * lg->stride * 4, hipMemcpyDeviceToHost, L.stream));
        } else {
            HIP_TRY(hipMemcpyAsync(direct ? (void*)policy : L.h_policy.p, L.d_policy.p, (size_t)n * d.moves * 4, hipMemcpyDeviceToHost, L.stream));
        }
        HIP_TRY(hipMemcpyAsync(direct ? (void*)value : L.h_value.p, L.d_value.p, (size_t)n * 4, hipMemcpyDeviceToHost, L.stream));
        return CATTUS_OK;
    };
    // Forward + copies + wait.  hipStreamSynchronize spins on the completion signal (lowest latency: +3 % self-play throughput on a 16-CPU
    // share with 8 search threads); CATTUS_HIP_WAIT=block sleeps on a blocking-sync event instead, which frees the core each waiting
    // thread would burn (for hosts short of CPUs).
    auto run_batch = [&]() -> int {
        int rc = enqueue_forward(e, L, L.d_planes.as<uint64_t>(), n, L.d_policy.as<float>(), L.d_value.as<float>(), L.stream);
        if (rc) return rc;
        if (verify) {
            // the same device-resident leaves through the shadow's lane of this index, on this lane's stream, behind the evaluator's own pass:
            // it writes the shadow lane's buffers only, so what the copies below return is what they return without it.  (A batch the one-launch
            // tower gives up on comes through here twice; its second run's records are the ones that are folded.)
            Lane& SL = e->shadow->lanes[&L - e->lanes];
            if ((rc = enqueue_forward(e->shadow, SL, L.d_planes.as<uint64_t>(), n, SL.d_policy.as<float>(), SL.d_value.as<float>(), L.stream))) return rc;
            VerifyRecord* const rec = L.d_verify.as<VerifyRecord>();
            launch_verify_outputs(L.d_policy.as<float>(), SL.d_policy.as<float>(), L.d_value.as<float>(), SL.d_value.as<float>(), n, d.moves, rec,
                                  reinterpret_cast<float*>(rec + n), L.stream);
            HIP_TRY(hipMemcpyAsync(L.h_verify.p, rec, (size_t)n * 2 * sizeof(VerifyRecord), hipMemcpyDeviceToHost, L.stream));
        }
        if ((rc = copy_out())) return rc;
        if (e->wait_spin) {
            HIP_TRY(hipStreamSynchronize(L.stream));
        } else {
            HIP_TRY(hipEventRecord(L.done, L.stream));
            HIP_TRY(hipEventSynchronize(L.done));
        }
        return CATTUS_OK;
    };
    int rc = run_batch();
    if (rc) return rc;
    if (take_tower_give_up(e, L) && (rc = run_batch())) return rc;  // this batch again, from the planes, on the per-layer launches
    if (!direct) {
        if (logits_out) memcpy(policy, L.h_policy.p, (size_t)n * d.moves * 4);
        memcpy(value, L.h_value.p, (size_t)n * 4);
    }
    if (rag_total) memcpy(lg->probs, L.h_rag_probs.p, (size_t)rag_total * 4);
    if (verify) {
        fold_verified(e, L.h_verify.as<VerifyRecord>(), n, static_cast<const uint64_t*>(src_planes));
        fold_priors(e, L.h_verify.as<VerifyRecord>(), n, static_cast<const uint64_t*>(src_planes), L.h_prior.as<PriorRecord>(), lg);
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    account(e, n, &seconds, verify);
    return CATTUS_OK;
}

ServerBatch* new_batch(cattus_eval* e) {
    auto b = std::make_unique<ServerBatch>();
    b->seq = e->next_seq++;
    b->planes.resize((size_t)e->cfg.max_batch * e->d.planes * e->cfg.plane_words);
    e->batches.push_back(std::move(b));
    return e->batches.back().get();
}

void server_loop(cattus_eval* e) {
    std::unique_lock<std::mutex> lk(e->srv_mu);
    for (;;) {
        // pick the oldest batch that is sealed and not yet run; seal the collecting one on deadline/flush
        ServerBatch* run = nullptr;
        for (auto& b : e->batches)
            if (b->sealed && !b->done && !b->running) {
                run = b.get();
                break;
            }
        if (!run && !e->batches.empty()) {
            ServerBatch* cur = e->batches.back().get();
            if (!cur->sealed && !cur->running && cur->count > 0) {
                const auto deadline = cur->t0 + std::chrono::microseconds(e->cfg.flush_us);
                if (e->flush_req || std::chrono::steady_clock::now() >= deadline) {
                    cur->sealed = true;
                    run = cur;
                } else if (!e->stop) {
                    e->srv_cv.wait_until(lk, deadline);
                    continue;
                }
            }
        }
        if (!run) {
            e->flush_req = false;
            if (e->stop) return;
            e->srv_cv.wait(lk);
            continue;
        }
        run->running = true;
        const uint32_t n = run->count;
        // a batch with lists runs the ragged softmax on the device; where all its leaves carry one, no logits come back at all
        const bool ragged = run->legal_leaves > 0, logits = run->legal_leaves < n;
        if (logits) run->policy.resize((size_t)n * e->d.moves);
        run->value.resize(n);
        run->taken.assign(n, 0);
        LegalArgs lg{};
        if (ragged) {
            legal_close(run->legal_off, n);
            run->kind.resize(n, 0);
            run->probs.resize(run->legal_off[n]);
            lg.idx = run->legal_idx.data(), lg.probs = run->probs.data(), lg.off = run->legal_off.data(), lg.kind = run->kind.data(), lg.logits = logits;
        }
        lk.unlock();
        const int rc = eval_host(e, run->planes.data(), n, logits ? run->policy.data() : nullptr, run->value.data(), ragged ? &lg : nullptr);
        std::string err = rc ? g_last_error : std::string();
        lk.lock();
        run->status = rc;
        run->error = err;
        run->done = true;
        e->done_cv.notify_all();
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------ ABI

CATTUS_API const char* cattus_hip_last_error(void) { return g_last_error.c_str(); }
CATTUS_API const char* cattus_hip_version(void) { return "cattus_hip 0.2 (gfx950)"; }
CATTUS_API const char* cattus_hip_runtime_note(void) { return g_runtime_note.c_str(); }

CATTUS_API const char* cattus_hip_tower_kernel(const cattus_eval* e) {
    if (!e) return "";
    switch (e->plan.kind) {
        case TowerKind::Simple: return "policy_fc_kernel";
        case TowerKind::Generic: return "conv3x3_generic_kernel";
        case TowerKind::Resident64: return "tower64_lds_kernel";
        case TowerKind::Resident64Split: return "tower64_split_kernel";
        case TowerKind::Resident64Stream: return "tower64_stream_kernel";
        case TowerKind::Resident64F32: return "tower64_f32_kernel";
        case TowerKind::Wino16: return "conv3x3_wino_kernel";
        case TowerKind::Wino4: return one_launch_now(e, e->bpad) ? "tower_wino4_kernel" : "conv3x3_wino4_kernel";
        case TowerKind::WinoF4: return "conv3x3_winof4_kernel";
        case TowerKind::WinoF16: return "conv3x3_wino_f16_kernel";
        case TowerKind::WinoF32: return "conv3x3_wino_f32_kernel";
        case TowerKind::DirectSplitK: return "conv3x3_splitk_kernel";
        case TowerKind::PerLayerStream: return "conv3x3_f16r_kernel";
        case TowerKind::PerLayer: break;
    }
    return e->act != Act::F16S ? "conv3x3_mfma_v2_kernel" : e->plan.w_frag ? "conv3x3_splitw_kernel" : "conv3x3_split_kernel";
}

CATTUS_API int cattus_hip_tail_leaves(const cattus_eval* e, uint32_t* effective) {
    if (!e || !effective) return fail(CATTUS_E_INVALID, "NULL argument");
    *effective = e->tail_leaves;
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_splitk_plan(const cattus_eval* e, uint32_t* ways, uint32_t* bounds) {
    if (!e || !ways) return fail(CATTUS_E_INVALID, "NULL argument");
    if (e->plan.kind != TowerKind::DirectSplitK) return fail(CATTUS_E_UNSUPPORTED, "splitk_plan: the evaluator does not run tower_form DIRECT_SPLITK");
    const int chunks = (int)e->fpad / 32, w = splitk_ways(chunks, e->splitk_forced);
    *ways = (uint32_t)w;
    for (int i = 0; bounds && i <= w; i++) bounds[i] = (uint32_t)splitk_bound(chunks, w, i);
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_tail_batches(cattus_eval* e, uint64_t* batches) {
    if (!e || !batches) return fail(CATTUS_E_INVALID, "NULL argument");
    *batches = e->tail_batches.load(std::memory_order_relaxed);
    return CATTUS_OK;
}

// the f32 MFMA heads: a tuned tower (Forward::heads_mfma) whose head kernels run in f32, within what one workgroup of the chain form keeps in LDS
static bool heads_are_f32_mfma(const cattus_eval* e) {
    return e->plan.tuned() && head_act(e->act) == Act::F32 && hc_lds_bytes(2, e->kvp, e->kpp) <= HC_LDS_MAX;
}

CATTUS_API int cattus_hip_head_chain(cattus_eval* e, uint32_t leaves) {
    if (!e) return fail(CATTUS_E_INVALID, "NULL argument");
    if (leaves > e->cfg.max_batch) return fail(CATTUS_E_INVALID, "head_chain: %u leaves is more than max_batch %u", leaves, e->cfg.max_batch);
    std::unique_lock<std::mutex> held[NLANES];  // every lane, in lane order: batches in flight finish first, none starts meanwhile
    for (int i = 0; i < NLANES; i++) held[i] = std::unique_lock<std::mutex>(e->lanes[i].mu);
    e->head_chain = heads_are_f32_mfma(e) ? leaves : 0;
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_head_chain_leaves(const cattus_eval* e, uint32_t* effective) {
    if (!e || !effective) return fail(CATTUS_E_INVALID, "NULL argument");
    *effective = e->head_chain.load(std::memory_order_relaxed);
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_head_chain_batches(cattus_eval* e, uint64_t* batches) {
    if (!e || !batches) return fail(CATTUS_E_INVALID, "NULL argument");
    *batches = e->head_chain_batches.load(std::memory_order_relaxed);
    return CATTUS_OK;
}

// head_fuse_rule.h's name for this evaluator's tower plan
static HfPlan fused_heads_plan(const cattus_eval* e) {
    switch (e->plan.kind) {
        case TowerKind::Resident64: return e->act == Act::F16 ? HfPlan::Resident64F16 : HfPlan::Resident64Bf16;
        case TowerKind::Resident64Split: return HfPlan::Resident64Split;
        case TowerKind::Resident64Stream: return HfPlan::Resident64Stream;
        case TowerKind::Resident64F32: return HfPlan::Resident64F32;
        default: return HfPlan::Other;
    }
}

CATTUS_API int cattus_hip_fused_heads(cattus_eval* e, uint32_t on) {
    if (!e) return fail(CATTUS_E_INVALID, "NULL argument");
    std::unique_lock<std::mutex> held[NLANES];  // every lane, in lane order: batches in flight finish first, none starts meanwhile
    for (int i = 0; i < NLANES; i++) held[i] = std::unique_lock<std::mutex>(e->lanes[i].mu);
    e->fused_heads = on && hf_takes(fused_heads_plan(e)) ? 1 : 0;
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_fused_heads_effective(const cattus_eval* e, uint32_t* effective) {
    if (!e || !effective) return fail(CATTUS_E_INVALID, "NULL argument");
    *effective = e->fused_heads.load(std::memory_order_relaxed);
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_fused_heads_batches(cattus_eval* e, uint64_t* batches) {
    if (!e || !batches) return fail(CATTUS_E_INVALID, "NULL argument");
    *batches = e->fused_heads_batches.load(std::memory_order_relaxed);
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_stream_shift(const cattus_eval* e) { return e ? e->stream_shift : 0; }

CATTUS_API int cattus_hip_stream_shifts(const cattus_eval* e, int* out, uint32_t n) {
    if (!e || (n && !out)) return fail(CATTUS_E_INVALID, "NULL argument");
    if (n != e->stream_shifts.size()) return fail(CATTUS_E_INVALID, "stream_shifts: %u entries asked for, the tower has %zu channels", n, e->stream_shifts.size());
    std::copy(e->stream_shifts.begin(), e->stream_shifts.end(), out);
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_stem_input(const cattus_eval* e, uint32_t* channels, uint32_t* packed) {
    if (!e) return fail(CATTUS_E_INVALID, "NULL argument");
    if (channels) *channels = e->cpad0;
    // the towers that go through Forward::conv_mfma; the resident ones expand the planes in their one launch
    if (packed) *packed = (e->plan.kind == TowerKind::PerLayer || e->plan.kind == TowerKind::PerLayerStream || e->plan.kind == TowerKind::DirectSplitK || e->plan.wino()) && !stem_is_fused(e->d.planes, e->pack_separately);
    return CATTUS_OK;
}

namespace {

// Diagnostic switches of cattus_hip_create_diag (include/cattus_hip_diag.h): "KEY=VALUE;KEY=VALUE".  cattus_hip_create passes none,
// and the library reads no A/B switch from the environment: what a host links is one code path per configuration.
struct Switches {
    std::map<std::string, std::string> kv;
    int parse(const char* text) {
        if (!text) return CATTUS_OK;
        static const char* const known[] = {"CATTUS_CONV_CB", "CATTUS_CONV_PBW", "CATTUS_FUSED_STEM", "CATTUS_T64_CH", "CATTUS_T64_LS", "CATTUS_SPLIT_W",
                                            "CATTUS_T64S_HEADS", "CATTUS_T64S_SHAPE", "CATTUS_TOWER64", "CATTUS_FORCE_GENERIC", "CATTUS_WINO_INPLACE",
                                            "CATTUS_ARENA", "CATTUS_WINO_KERNEL", "CATTUS_WINO_PERSIST", "CATTUS_WINO_SPIN", "CATTUS_STREAM_SHIFT", "CATTUS_SPLITK_WAYS", "CATTUS_T64F_NARROW"};
        const std::string s(text);
        size_t at = 0;
        while (at < s.size()) {
            size_t end = s.find(';', at);
            if (end == std::string::npos) end = s.size();
            const std::string item = s.substr(at, end - at);
            at = end + 1;
            if (item.empty()) continue;
            const size_t eq = item.find('=');
            if (eq == std::string::npos || eq == 0) return fail(CATTUS_E_INVALID, "diagnostic switch '%s' is not KEY=VALUE", item.c_str());
            const std::string key = item.substr(0, eq);
            bool ok = false;
            for (const char* k : known) ok = ok || key == k;
            if (!ok) return fail(CATTUS_E_INVALID, "unknown diagnostic switch '%s'", key.c_str());
            kv[key] = item.substr(eq + 1);
        }
        return CATTUS_OK;
    }
    const char* get(const char* key) const {
        auto it = kv.find(key);
        return it == kv.end() ? nullptr : it->second.c_str();
    }
    bool starts(const char* key, char c) const { return get(key) && get(key)[0] == c; }  // the switch is given and its value begins with c
    int number(const char* key) const { return get(key) ? atoi(get(key)) : 0; }          // 0 when the switch is not given
};

// Which tower runs, from the network, the configuration, the switches and the tuned towers' padding (bpad boards, fpad filters, cpad0 stem
// input channels).  The form is part of the configuration: AUTO = Winograd for max_batch > 128 where a kernel covers the shape; WINOGRAD
// where none does is refused.  The resident kinds and the Winograd kinds cannot both hold -- the resident kinds need fpad == 64,
// wino_supported needs cout % 128 == 0 and wino4_supported cout >= 128 -- so the order of the cases below decides nothing between them.
int resolve_plan(const cattus_net_desc& d, const cattus_eval_config& cfg, const Switches& sw, Act act, uint32_t bpad, uint32_t fpad, uint32_t cpad0,
                 TowerPlan* plan) {
    // The MFMA tower covers every board up to 11x11 and any filter count (channels are padded to 64 with zeros);
    // the two 1x1 head convs share one 32-row MFMA tile.  Wider heads take the generic f32 path (one thread
    // per output, same arithmetic order), which otherwise serves as a checker only (CATTUS_FORCE_GENERIC=1).
    const bool simple = d.filters == 0, tuned = !simple && d.vhc + d.phc <= 32 && !sw.starts("CATTUS_FORCE_GENERIC", '1');
    // the LDS-resident bf16 / f16 tower's coverage (tower64_lds_kernel, tower64_stream_kernel): at most 64 padded filters, planes it expands itself
    const bool resident = tuned && fpad == 64 && !sw.starts("CATTUS_TOWER64", '0');
    const bool resident64 = resident && cpad0 == 64;
    if (!tuned && act != Act::F32 && cfg.dtype != CATTUS_DTYPE_F16R_RESIDENT)  // (f16r_resident refuses below, under its own name)
        return fail(CATTUS_E_UNSUPPORTED, "bf16 / f16 / f16x2 need the MFMA tower: value + policy head channels <= 32 (got %u + %u)", d.vhc, d.phc);
    // dtype f16w: the single-term f16 Winograd tower and nothing else -- AUTO and WINOGRAD both mean it, every other form and every
    // shape it does not cover is refused (never other bits under this name); a SimpleTwoHeadedModel runs in f32 as under every dtype
    if (cfg.dtype == CATTUS_DTYPE_F16W && !simple) {
        if (cfg.tower_form != CATTUS_TOWER_AUTO && cfg.tower_form != CATTUS_TOWER_WINOGRAD)
            return fail(CATTUS_E_UNSUPPORTED, "dtype f16w is the Winograd F(2x2, 3x3) form: tower_form AUTO or WINOGRAD (got %u)", cfg.tower_form);
        if (!(d.blocks > 0 && wino_f16_supported(bpad, fpad, fpad, d.board)))
            return fail(CATTUS_E_UNSUPPORTED, "dtype f16w needs an 8x8 board, at least one residual block and a multiple of 64 filters (at least 128)");
        *plan = TowerPlan();
        plan->kind = TowerKind::WinoF16;
        plan->inplace = !sw.starts("CATTUS_WINO_INPLACE", '0');
        return CATTUS_OK;
    }
    // dtype f32w: the f32-operand Winograd tower and nothing else, by the same rule
    if (cfg.dtype == CATTUS_DTYPE_F32W && !simple) {
        if (cfg.tower_form != CATTUS_TOWER_AUTO && cfg.tower_form != CATTUS_TOWER_WINOGRAD)
            return fail(CATTUS_E_UNSUPPORTED, "dtype f32w is the Winograd F(2x2, 3x3) form: tower_form AUTO or WINOGRAD (got %u)", cfg.tower_form);
        if (!(tuned && d.blocks > 0 && wino_f32_supported(bpad, fpad, fpad, d.board)))
            return fail(CATTUS_E_UNSUPPORTED,
                        "dtype f32w needs an 8x8 board, at least one residual block, a multiple of 64 filters (at least 128) and value + policy head channels <= 32");
        *plan = TowerPlan();
        plan->kind = TowerKind::WinoF32;
        plan->inplace = !sw.starts("CATTUS_WINO_INPLACE", '0');
        return CATTUS_OK;
    }
    // dtype f16r: the per-layer direct f16 tower with an f32 residual stream and nothing else -- every shape dtype f16 runs on the MFMA
    // per-layer tower (wider heads were refused above: the generic path is f32); AUTO means it, the forms 1-4 are ignored (they name forms of the
    // f16x2 tower; dtype f16 ignores DIRECT alike), RESIDENT is refused (the one-launch form of this tower is a dtype of its own, f16r_resident, below), tail_leaves is ignored
    if (cfg.dtype == CATTUS_DTYPE_F16R && !simple) {
        if (cfg.tower_form == CATTUS_TOWER_RESIDENT)
            return fail(CATTUS_E_UNSUPPORTED, "dtype f16r is the per-layer tower (tower_form AUTO): its one-launch LDS-resident form is dtype f16r_resident");
        *plan = TowerPlan();
        plan->kind = TowerKind::PerLayerStream;
        return CATTUS_OK;
    }
    // dtype f16r_resident: dtype f16r's arithmetic, bit for bit, as a demand for the one-launch LDS-resident form and nothing else -- exactly the
    // evaluators on which dtype f16 accepts tower_form RESIDENT (`resident64` above: one predicate for both); AUTO and RESIDENT both mean it, the
    // forms 1-4 are ignored as under f16r, tail_leaves is ignored; anything the form does not cover is refused, never other bits under this name
    if (cfg.dtype == CATTUS_DTYPE_F16R_RESIDENT && !simple) {
        if (!resident64)
            return fail(CATTUS_E_UNSUPPORTED, "dtype f16r_resident is dtype f16r in the one-launch LDS-resident form: at most 64 filters, at most 64 planes, value + policy head channels <= 32 "
                                              "(and no CATTUS_TOWER64=0); dtype f16r runs every other shape per layer");
        *plan = TowerPlan();
        plan->kind = TowerKind::Resident64Stream;
        return CATTUS_OK;
    }
    // dtype f32_resident: dtype f32's arithmetic, bit for bit, as a demand for the one-launch LDS-resident form and nothing else -- wherever the
    // resident predicate above holds and the stem's input is one 128-byte chunk of f32 (at most 32 planes); AUTO and RESIDENT both mean it, the
    // forms 1-4 are ignored as under f32, tail_leaves is ignored; anything the form does not cover is refused, never other bits under this name
    if (cfg.dtype == CATTUS_DTYPE_F32_RESIDENT && !simple) {
        if (!(resident && cpad0 == 32))
            return fail(CATTUS_E_UNSUPPORTED, "dtype f32_resident is dtype f32 in the one-launch LDS-resident form: at most 64 filters, at most 32 planes, value + policy head channels <= 32 "
                                              "(and no CATTUS_TOWER64=0); dtype f32 runs every other shape per layer");
        *plan = TowerPlan();
        plan->kind = TowerKind::Resident64F32;
        return CATTUS_OK;
    }
    // the 4-frequency kernel wherever it covers the layer shape (filters a multiple of 64), else the 16-frequency one (128)
    const char* wk = sw.get("CATTUS_WINO_KERNEL");
    if (wk && strcmp(wk, "k16") != 0 && strcmp(wk, "k4") != 0) return fail(CATTUS_E_INVALID, "CATTUS_WINO_KERNEL is k16 or k4");
    const bool k4 = wk ? strcmp(wk, "k4") == 0 : wino4_supported(bpad, fpad, fpad, d.board);
    const bool wino_covers = tuned && act == Act::F16S && d.blocks > 0 && (k4 ? wino4_supported : wino_supported)(bpad, fpad, fpad, d.board);
    if (cfg.tower_form == CATTUS_TOWER_WINOGRAD && !wino_covers)
        return fail(CATTUS_E_UNSUPPORTED, "tower_form WINOGRAD needs dtype f16x2, an 8x8 board, at least one residual block and a multiple of 64 filters");
    // WINOGRAD_F4: the F(4x4, 3x3) form, only when asked for; the coverage of WINOGRAD
    const bool winof4_covers = tuned && act == Act::F16S && d.blocks > 0 && winof4_supported(bpad, fpad, fpad, d.board);
    if (cfg.tower_form == CATTUS_TOWER_WINOGRAD_F4 && !winof4_covers)
        return fail(CATTUS_E_UNSUPPORTED, "tower_form WINOGRAD_F4 needs dtype f16x2, an 8x8 board, at least one residual block and a multiple of 64 filters (at least 128)");
    TowerPlan& p = *plan = TowerPlan();
    p.w_frag = tuned && act == Act::F16S && !sw.starts("CATTUS_SPLIT_W", '0');
    // DIRECT_SPLITK: the split-K direct form, only when asked for, whatever max_batch is
    if (cfg.tower_form == CATTUS_TOWER_DIRECT_SPLITK) {
        const char* const needs = "tower_form DIRECT_SPLITK needs dtype f16x2 with fragment-order weights, a board of edge <= 8, at least one residual block and a multiple of 64 filters, 128 to 512";
        if (!(tuned && act == Act::F16S && p.w_frag && d.blocks > 0 && tower_slots(d.board) == 64 && splitk_supported(fpad, fpad, d.board)))
            return fail(CATTUS_E_UNSUPPORTED, "%s", needs);
        if (const char* wv = sw.get("CATTUS_SPLITK_WAYS"))
            if (strcmp(wv, "1") != 0 && strcmp(wv, "2") != 0 && strcmp(wv, "4") != 0 && strcmp(wv, "8") != 0) return fail(CATTUS_E_INVALID, "CATTUS_SPLITK_WAYS is 1, 2, 4 or 8");
        p.kind = TowerKind::DirectSplitK;
        return CATTUS_OK;
    }
    const bool resident64_split = resident && cpad0 == 32 && p.w_frag && 1 + 2 * d.blocks <= (uint32_t)T64S_MAX_LAYERS;
    // RESIDENT: the one-launch LDS-resident tower, a demand: what AUTO gives bf16 and f16x2 on these shapes, and for f16 -- only when asked
    // for -- bf16's kernel on bf16's shapes with the per-layer f16 tower's bits; a SimpleTwoHeadedModel runs in f32 as under every form
    if (cfg.tower_form == CATTUS_TOWER_RESIDENT && !simple) {
        if (!((resident64 && (act == Act::BF16 || act == Act::F16)) || (resident64_split && act == Act::F16S)))
            return fail(CATTUS_E_UNSUPPORTED, "tower_form RESIDENT needs dtype bf16, f16 or f16x2, value + policy head channels <= 32 and at most 64 filters (and no CATTUS_TOWER64=0)");
        p.kind = act == Act::F16S ? TowerKind::Resident64Split : TowerKind::Resident64;
        return CATTUS_OK;
    }
    if (!tuned) p.kind = simple ? TowerKind::Simple : TowerKind::Generic;
    else if (cfg.tower_form == CATTUS_TOWER_WINOGRAD_F4) {
        p.kind = TowerKind::WinoF4;
        p.inplace = !sw.starts("CATTUS_WINO_INPLACE", '0');  // never one launch for the tower
    } else if (wino_covers && (cfg.tower_form == CATTUS_TOWER_WINOGRAD || (cfg.tower_form == CATTUS_TOWER_AUTO && cfg.max_batch > 128))) {
        p.kind = k4 ? TowerKind::Wino4 : TowerKind::Wino16;
        p.inplace = !sw.starts("CATTUS_WINO_INPLACE", '0');
        p.one_launch = k4 && p.inplace && !sw.starts("CATTUS_WINO_PERSIST", '0');
    } else if (resident64 && act == Act::BF16) p.kind = TowerKind::Resident64;
    else if (resident64_split && act == Act::F16S) p.kind = TowerKind::Resident64Split;
    else p.kind = TowerKind::PerLayer;
    return CATTUS_OK;
}

// the lengths cattus_eval_config has had: up to flush_us, with tower_form, with tail_leaves
bool config_size_known(uint32_t size) {
    return size == offsetof(cattus_eval_config, tower_form) || size == offsetof(cattus_eval_config, tail_leaves) || size == sizeof(cattus_eval_config);
}

int create_impl(const void* weights, size_t nbytes, const cattus_eval_config* cfg_in, const char* switches, cattus_eval** out, const Calibration* cal = nullptr) {
    if (!out) return fail(CATTUS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!weights || !cfg_in) return fail(CATTUS_E_INVALID, "weights/cfg is NULL");
    // struct_size versions the configuration: 24 bytes = the fields up to flush_us (tower_form = AUTO), 28 = with tower_form (tail_leaves = 0),
    // 32 = with tail_leaves
    cattus_eval_config cfg_copy{};
    if (!config_size_known(cfg_in->struct_size)) return fail(CATTUS_E_INVALID, "cfg.struct_size mismatch");
    memcpy(&cfg_copy, cfg_in, cfg_in->struct_size);
    cfg_copy.struct_size = sizeof(cattus_eval_config);
    const cattus_eval_config* cfg = &cfg_copy;
    if (cfg->tower_form > CATTUS_TOWER_RESIDENT) return fail(CATTUS_E_INVALID, "unknown tower_form %u", cfg->tower_form);
    if (cfg->tail_leaves > cfg->max_batch) return fail(CATTUS_E_INVALID, "tail_leaves %u is more than max_batch %u", cfg->tail_leaves, cfg->max_batch);
    Switches sw;
    if (int src = sw.parse(switches)) return src;
    if (nbytes < HEADER_BYTES || memcmp(weights, "CATTUSW1", 8) != 0) return fail(CATTUS_E_INVALID, "not a cattus weight blob");
    uint32_t h[9];
    memcpy(h, (const char*)weights + 8, sizeof h);
    if (h[0] != 1 || h[8] != FC_HIDDEN) return fail(CATTUS_E_INVALID, "unsupported blob version %u / hidden %u", h[0], h[8]);
    cattus_net_desc d{h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8]};
    const bool simple = d.filters == 0;  // SimpleTwoHeadedModel: no conv tower (cattus_amd/weights.py)
    if (d.board < 1 || d.board > 11 || !d.planes || !d.moves || (!simple && (!d.vhc || !d.phc)) || (simple && (d.blocks || d.vhc || d.phc)))
        return fail(CATTUS_E_INVALID, "bad network shape in blob header");
    if (simple && (size_t)d.planes * d.board * d.board > 2048) return fail(CATTUS_E_UNSUPPORTED, "SimpleTwoHeadedModel wider than 2048 features");
    if (nbytes != HEADER_BYTES + 4 * blob_floats(d)) return fail(CATTUS_E_INVALID, "blob size %zu does not match its header", nbytes);
    if (cfg->max_batch < 1 || cfg->max_batch > (1u << 20)) return fail(CATTUS_E_INVALID, "max_batch out of range");
    if ((uint64_t)cfg->plane_words * 64 < (uint64_t)d.board * d.board || cfg->plane_words > 2)
        return fail(CATTUS_E_INVALID, "plane_words %u cannot hold a %ux%u board", cfg->plane_words, d.board, d.board);
    if (d.planes * cfg->plane_words > 128) return fail(CATTUS_E_UNSUPPORTED, "more than 128 plane words per leaf");
    if (cfg->dtype != CATTUS_DTYPE_F32 && cfg->dtype != CATTUS_DTYPE_BF16 && cfg->dtype != CATTUS_DTYPE_F16X2 && cfg->dtype != CATTUS_DTYPE_F16 &&
        cfg->dtype != CATTUS_DTYPE_F16W && cfg->dtype != CATTUS_DTYPE_F32W && cfg->dtype != CATTUS_DTYPE_F16R && cfg->dtype != CATTUS_DTYPE_F16R_RESIDENT &&
        cfg->dtype != CATTUS_DTYPE_F32_RESIDENT)  // (8 is unassigned)
        return fail(CATTUS_E_INVALID, "unknown dtype %u", cfg->dtype);
    if (!simple && (size_t)d.phc * d.board * d.board * 8 * 4 > 64 * 1024) return fail(CATTUS_E_UNSUPPORTED, "policy head too wide for the FC kernel");

    int ndev = 0;
    hipError_t herr = hipGetDeviceCount(&ndev);
    if (herr != hipSuccess || ndev <= 0)
        return fail(CATTUS_E_DEVICE, "no HIP device available (%s); this library has no CPU path", hipGetErrorString(herr));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(CATTUS_E_INVALID, "device %d out of range (%d devices)", cfg->device, ndev);
    HIP_TRY(hipSetDevice(cfg->device));
    {
        // the tower kernels' dynamic-LDS opt-in: once per device, before anything can be launched on it
        static std::mutex prep_mu;
        static uint64_t prepared = 0;
        std::lock_guard<std::mutex> lk(prep_mu);
        const uint64_t bit = 1ull << (cfg->device & 63);
        if (!(prepared & bit)) {
            const hipError_t perr = prepare_device();
            if (perr != hipSuccess) return fail(CATTUS_E_DEVICE, "hipFuncSetAttribute failed: %s", hipGetErrorString(perr));
            prepared |= bit;
        }
    }
    // every environment switch is read here, once per evaluator: nothing on the evaluation path calls getenv
    {
        static std::mutex note_mu;
        std::lock_guard<std::mutex> lk(note_mu);
        const char* ka = getenv("HIP_FORCE_DEV_KERNARG");
        g_runtime_note = ka && ka[0] == '1' ? "HIP_FORCE_DEV_KERNARG=1: kernel arguments in device memory"
                                            : "HIP_FORCE_DEV_KERNARG is not 1: kernel arguments travel over the host link (about +8 % per batch); "
                                              "export HIP_FORCE_DEV_KERNARG=1 before the process initialises HIP";
    }
    const char* wait_mode = getenv("CATTUS_HIP_WAIT");  // operational, not A/B: how the host thread waits for a batch

    std::unique_ptr<cattus_eval> e(new (std::nothrow) cattus_eval);
    if (!e) return fail(CATTUS_E_NOMEM, "out of memory");
    e->d = d, e->cfg = *cfg;
    e->blob_hash = blob_hash64(weights, nbytes), e->blob_bytes = nbytes;
    if (e->cfg.flush_us == 0) e->cfg.flush_us = 200;
    e->device = cfg->device;
    e->wait_spin = !(wait_mode && strcmp(wait_mode, "block") == 0);
    e->pack_separately = d.planes > 32 || sw.starts("CATTUS_FUSED_STEM", '0');
    e->t64_force_ch = sw.number("CATTUS_T64_CH");
    e->t64f_narrow = !sw.starts("CATTUS_T64F_NARROW", '0');
    e->t64_layer_steps = !(sw.get("CATTUS_T64_LS") && sw.number("CATTUS_T64_LS") == 0);
    e->stream_shift_on = !sw.starts("CATTUS_STREAM_SHIFT", '0');
    e->t64s_fuse_heads = !sw.starts("CATTUS_T64S_HEADS", '0');
    e->t64s_depth = sw.number("CATTUS_T64S_SHAPE");
    e->conv_opts.cb = sw.number("CATTUS_CONV_CB");
    e->conv_opts.pbw = sw.number("CATTUS_CONV_PBW");
    e->splitk_forced = sw.number("CATTUS_SPLITK_WAYS");
    e->hw = d.board * d.board;
    e->act = simple ? Act::F32
             : cfg->dtype == CATTUS_DTYPE_BF16 ? Act::BF16
             : cfg->dtype == CATTUS_DTYPE_F16X2 ? Act::F16S
             : cfg->dtype == CATTUS_DTYPE_F16 || cfg->dtype == CATTUS_DTYPE_F16W || cfg->dtype == CATTUS_DTYPE_F16R || cfg->dtype == CATTUS_DTYPE_F16R_RESIDENT ? Act::F16  // f16w: the direct f16 stem, f16r / f16r_resident: f16 operands; resolve_plan chooses their towers
                                              : Act::F32;  // f32w and f32_resident too: dtype f32's operands and rows; resolve_plan chooses their towers
    // the tuned towers' layout: whole workgroups of boards, filters in whole 64-channel groups (zero channels), the planes in whole
    // 128-byte rows; the other towers pad nothing
    e->slots = tower_slots(d.board);
    const uint32_t bpw = ROWS_PER_WG / e->slots;
    e->bpad = (cfg->max_batch + bpw - 1) / bpw * bpw;
    e->cpad0 = stem_cin_pad(d.planes, (uint32_t)act_kc(e->act), e->act == Act::F16S, e->pack_separately);
    e->fpad = (d.filters + COUT_PER_WG - 1) / COUT_PER_WG * COUT_PER_WG;
    if (int prc = resolve_plan(d, *cfg, sw, e->act, e->bpad, e->fpad, e->cpad0, &e->plan)) return prc;
    if (!e->plan.tuned()) e->bpad = cfg->max_batch, e->fpad = d.filters, e->cpad0 = d.planes;
    // short batches on the small-tile kernel: only where the plan is the F(2x2) Winograd tower (the kernel computes that tower's bits and no
    // other's) and the kernel covers the layer shape; everywhere else the field is ignored
    if ((e->plan.kind == TowerKind::Wino4 || e->plan.kind == TowerKind::Wino16) && wino4_supported(e->bpad, e->fpad, e->fpad, d.board)) e->tail_leaves = cfg->tail_leaves;
    if (act_f16_family(e->act)) {
        if (int src = e->d_saturated.alloc(sizeof(unsigned))) return src;
        HIP_TRY(hipMemset(e->d_saturated.p, 0, sizeof(unsigned)));
        e->conv_opts.saturated = e->d_saturated.as<unsigned>();
    }
    if (const char* ws = sw.get("CATTUS_WINO_SPIN")) e->persist_spin = (uint32_t)std::max(1L, atol(ws));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
    e->cus = (uint32_t)prop.multiProcessorCount;
    if (e->plan.wino() && !sw.starts("CATTUS_ARENA", '0')) {  // CATTUS_ARENA=0: every buffer its own allocation (A/B runs)
        // the Winograd tower's hot set in one block: U of every layer, then the lanes' activation buffers (DevArena)
        auto page = [](size_t b) { return (b + 4095) & ~(size_t)4095; };
        const size_t FPz = e->fpad;
        const size_t u_bytes = page(e->plan.kind == TowerKind::WinoF4    ? winof4_u_elems(e->fpad, e->fpad) * 2
                                    : e->plan.kind == TowerKind::WinoF16 ? wino_f16_u_elems(e->fpad, e->fpad) * 2
                                    : e->plan.kind == TowerKind::WinoF32 ? wino_f32_u_elems(e->fpad, e->fpad) * 4
                                                                         : ((size_t)16 * FPz * FPz * 2 + (size_t)WINO_RING_STAGES * 1024) * 2);
        const size_t act_bytes_ = page((size_t)e->bpad * e->slots * FPz * 4);
        const size_t want = 2 * (size_t)d.blocks * u_bytes + (size_t)NLANES * (e->plan.inplace ? 2 : 3) * act_bytes_ + (1u << 20);
        void* base = nullptr;
        if (hipMalloc(&base, want) == hipSuccess) e->arena.base = (char*)base, e->arena.cap = want;
        else (void)hipGetLastError();  // no room for one block: separate allocations, as before
    }
    if (int rc = build(e.get(), reinterpret_cast<const float*>((const char*)weights + HEADER_BYTES), cal)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    {
        std::lock_guard<std::mutex> lk(e->srv_mu);
        new_batch(e.get());
    }
    for (auto& t : e->servers) t = std::thread(server_loop, e.get());
    *out = e.release();
    return CATTUS_OK;
}

}  // namespace

CATTUS_API int cattus_hip_create(const void* weights, size_t nbytes, const cattus_eval_config* cfg, cattus_eval** out) {
    return create_impl(weights, nbytes, cfg, nullptr, out);
}

CATTUS_API int cattus_hip_create_diag(const void* weights, size_t nbytes, const cattus_eval_config* cfg, const char* switches, cattus_eval** out) {
    return create_impl(weights, nbytes, cfg, switches, out);
}

CATTUS_API void cattus_hip_destroy(cattus_eval* e) { delete e; }

CATTUS_API int cattus_hip_stream_range(cattus_eval* e, const uint64_t* planes, uint32_t n, cattus_channel_range* out, uint32_t channels) {
    if (!e || !planes || !out) return fail(CATTUS_E_INVALID, "NULL argument");
    if (e->act != Act::F32 || e->plan.kind != TowerKind::PerLayer)
        return fail(CATTUS_E_UNSUPPORTED, "stream_range measures on the exact f32 tower: a dtype f32 evaluator on the MFMA per-layer tower");
    const cattus_net_desc& d = e->d;
    if (channels != d.filters) return fail(CATTUS_E_INVALID, "stream_range: %u entries asked for, the tower has %u channels", channels, d.filters);
    if (n < 1) return fail(CATTUS_E_INVALID, "stream_range needs at least one leaf");
    std::unique_lock<std::mutex> lk;
    Lane& L = take_lane(e, lk);
    HIP_TRY(hipSetDevice(e->device));
    const size_t FP = e->fpad, acc_bytes = FP * (sizeof(double) + sizeof(float));
    if (!L.range_acc.p) {
        const size_t parts = stream_range_parts(e->bpad, d.board);
        int rc;
        if ((rc = L.range_part_sq.alloc(parts * FP * sizeof(double))) || (rc = L.range_part_max.alloc(parts * FP * sizeof(float))) || (rc = L.range_acc.alloc(acc_bytes)))
            return rc;
    }
    HIP_TRY(hipMemsetAsync(L.range_acc.p, 0, acc_bytes, L.stream));
    const size_t leaf_words = (size_t)d.planes * e->cfg.plane_words;
    uint32_t m = 0;  // leaves of the chunk being enqueued
    // the f32 tower's stream tensors (the even points: plain f32 rows) into the lane's range accumulators
    const Observer range = [&](uint32_t point, const void* buf, const TapSource&) {
        double* const acc_sq = L.range_acc.as<double>();
        if (point % 2 == 0)
            launch_stream_range(static_cast<const float*>(buf), padded_boards(e, m), m, d.board, (uint32_t)FP, L.range_part_sq.as<double>(), L.range_part_max.as<float>(),
                                acc_sq, reinterpret_cast<float*>(acc_sq + FP), L.stream);
        return CATTUS_OK;
    };
    for (uint32_t at = 0; at < n; at += e->cfg.max_batch) {  // the staging buffer is free again once the chunk is through
        m = std::min(n - at, e->cfg.max_batch);
        memcpy(L.h_planes.p, planes + at * leaf_words, m * leaf_words * 8);
        HIP_TRY(hipMemcpyAsync(L.d_planes.p, L.h_planes.p, m * leaf_words * 8, hipMemcpyHostToDevice, L.stream));
        if (int rc = enqueue_forward(e, L, L.d_planes.as<uint64_t>(), m, L.d_policy.as<float>(), L.d_value.as<float>(), L.stream, nullptr, &range)) return rc;
        HIP_TRY(hipStreamSynchronize(L.stream));
    }
    std::vector<double> sq(FP);
    std::vector<float> mx(FP);
    HIP_TRY(hipMemcpy(sq.data(), L.range_acc.p, FP * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mx.data(), (const char*)L.range_acc.p + FP * sizeof(double), FP * sizeof(float), hipMemcpyDeviceToHost));
    const double count = (double)n * e->hw * (1 + d.blocks);  // values per channel: leaves x pixels x stream tensors
    for (uint32_t k = 0; k < channels; k++) out[k] = cattus_channel_range{(float)std::sqrt(sq[k] / count), mx[k]};
    return CATTUS_OK;
}

namespace {

int create_calibrated_impl(const void* weights, size_t nbytes, const cattus_eval_config* cfg, const char* switches, const uint64_t* planes, uint32_t n,
                           cattus_eval** out) {
    if (!out) return fail(CATTUS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!weights || !cfg || !planes) return fail(CATTUS_E_INVALID, "weights/cfg/planes is NULL");
    if (n < 1) return fail(CATTUS_E_INVALID, "calibration needs at least one leaf");
    if (!config_size_known(cfg->struct_size)) return fail(CATTUS_E_INVALID, "cfg.struct_size mismatch");
    uint32_t filters = 0;  // 0: SimpleTwoHeadedModel (or no blob at all, which create_impl refuses)
    if (nbytes >= HEADER_BYTES) memcpy(&filters, (const char*)weights + 8 + 5 * 4, 4);
    // only the f16 towers shift their stream: everything else is cattus_hip_create
    if ((cfg->dtype != CATTUS_DTYPE_F16X2 && cfg->dtype != CATTUS_DTYPE_F16 && cfg->dtype != CATTUS_DTYPE_F16W && cfg->dtype != CATTUS_DTYPE_F16R && cfg->dtype != CATTUS_DTYPE_F16R_RESIDENT) || filters == 0) return create_impl(weights, nbytes, cfg, switches, out);
    cattus_eval_config mcfg{};
    mcfg.struct_size = sizeof mcfg, mcfg.device = cfg->device, mcfg.max_batch = std::min(n, 256u), mcfg.plane_words = cfg->plane_words;
    mcfg.dtype = CATTUS_DTYPE_F32, mcfg.flush_us = cfg->flush_us, mcfg.tower_form = CATTUS_TOWER_AUTO;
    cattus_eval* measure = nullptr;
    if (int rc = create_impl(weights, nbytes, &mcfg, nullptr, &measure)) return rc;
    std::vector<cattus_channel_range> range(filters);
    const int rrc = cattus_hip_stream_range(measure, planes, n, range.data(), filters);
    cattus_hip_destroy(measure);
    if (rrc) return rrc;
    Calibration cal;
    for (const cattus_channel_range& r : range) cal.s2.push_back((double)r.rms * r.rms), cal.abs_max.push_back(r.abs_max);
    return create_impl(weights, nbytes, cfg, switches, out, &cal);
}

}  // namespace

CATTUS_API int cattus_hip_create_calibrated(const void* weights, size_t nbytes, const cattus_eval_config* cfg, const uint64_t* planes, uint32_t n,
                                            cattus_eval** out) {
    return create_calibrated_impl(weights, nbytes, cfg, nullptr, planes, n, out);
}

CATTUS_API int cattus_hip_create_calibrated_diag(const void* weights, size_t nbytes, const cattus_eval_config* cfg, const char* switches,
                                                 const uint64_t* planes, uint32_t n, cattus_eval** out) {
    return create_calibrated_impl(weights, nbytes, cfg, switches, planes, n, out);
}

CATTUS_API int cattus_hip_desc(const cattus_eval* e, cattus_net_desc* out) {
    if (!e || !out) return fail(CATTUS_E_INVALID, "NULL argument");
    *out = e->d;
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_eval(cattus_eval* e, const uint64_t* planes, uint32_t n, float* policy, float* value) {
    if (!e || !planes || !policy || !value) return fail(CATTUS_E_INVALID, "NULL argument");
    // planes_to_tensor asserts 1 <= n <= batch_size (engine/src/net/mod.rs:122-127)
    if (n < 1 || n > e->cfg.max_batch) return fail(CATTUS_E_INVALID, "invalid sample len %u, 1..=%u", n, e->cfg.max_batch);
    return eval_host(e, planes, n, policy, value);
}

CATTUS_API int cattus_hip_eval_legal(cattus_eval* e, const uint64_t* planes, uint32_t n, const uint16_t* legal_idx,
                                     const uint16_t* legal_count, uint32_t legal_stride, float* probs, float* value) {
    if (!e || !planes || !legal_idx || !legal_count || !probs || !value) return fail(CATTUS_E_INVALID, "NULL argument");
    if (n < 1 || n > e->cfg.max_batch) return fail(CATTUS_E_INVALID, "invalid sample len %u, 1..=%u", n, e->cfg.max_batch);
    if (legal_stride < 1 || legal_stride > 1024) return fail(CATTUS_E_INVALID, "legal_stride %u outside 1..=1024", legal_stride);
    for (uint32_t i = 0; i < n; i++) {
        if (legal_count[i] > legal_stride) return fail(CATTUS_E_INVALID, "leaf %u: %u legal moves > stride %u", i, legal_count[i], legal_stride);
        for (uint32_t k = 0; k < legal_count[i]; k++)
            if (legal_idx[(size_t)i * legal_stride + k] >= e->d.moves)
                return fail(CATTUS_E_INVALID, "leaf %u: policy index %u >= %u", i, legal_idx[(size_t)i * legal_stride + k], e->d.moves);
    }
    const LegalArgs lg{legal_idx, legal_count, legal_stride, probs};
    return eval_host(e, planes, n, nullptr, value, &lg);
}

CATTUS_API int cattus_hip_eval_device(cattus_eval* e, const uint64_t* d_planes, uint32_t n, float* d_policy, float* d_value,
                                      void* stream) {
    return cattus_hip_eval_device_lane(e, 0, d_planes, n, d_policy, d_value, stream);
}

CATTUS_API int cattus_hip_eval_device_lane(cattus_eval* e, uint32_t lane, const uint64_t* d_planes, uint32_t n, float* d_policy,
                                           float* d_value, void* stream) {
    if (!e || !d_planes || !d_policy || !d_value) return fail(CATTUS_E_INVALID, "NULL argument");
    if (n < 1 || n > e->cfg.max_batch) return fail(CATTUS_E_INVALID, "invalid sample len %u, 1..=%u", n, e->cfg.max_batch);
    if (lane >= NLANES) return fail(CATTUS_E_INVALID, "lane %u out of range (%d lanes)", lane, NLANES);
    Lane& L = e->lanes[lane];
    std::lock_guard<std::mutex> lk(L.mu);
    HIP_TRY(hipSetDevice(e->device));
    if (take_tower_give_up(e, L))  // this entry point is asynchronous: what an earlier call's one-launch tower reported is seen here, at the next call
        return fail(CATTUS_E_DEVICE, "an earlier batch on lane %u ran the tower as one launch and a hand-off wait in it gave up (the device was shared): that batch's "
                                     "outputs are invalid; this evaluator uses the per-layer launches from now on", lane);
    hipStream_t st = (hipStream_t)stream;  // as HIP itself: NULL is the legacy default stream, not a private one
    int rc = enqueue_forward(e, L, d_planes, n, d_policy, d_value, st);
    if (rc) return rc;
    account(e, n, nullptr);
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_lane_stream(cattus_eval* e, uint32_t lane, void** stream) {
    if (!e || !stream) return fail(CATTUS_E_INVALID, "NULL argument");
    if (lane >= NLANES) return fail(CATTUS_E_INVALID, "lane %u out of range (%d lanes)", lane, NLANES);
    *stream = (void*)e->lanes[lane].stream;
    return CATTUS_OK;
}

// One leaf into the collecting batch.  list: NULL for cattus_hip_submit, else the leaf's legal_count policy indices (already checked), appended to
// the batch's ragged table (legal_span.h).
static int submit_leaf(cattus_eval* e, const uint64_t* planes_one, const uint16_t* list, uint32_t legal_count, uint64_t* ticket) {
    const size_t words = (size_t)e->d.planes * e->cfg.plane_words;
    std::unique_lock<std::mutex> lk(e->srv_mu);
    if (e->stop) return fail(CATTUS_E_STATE, "evaluator is shutting down");
    // the deque can be empty: a deadline-sealed batch may already have been collected and erased
    ServerBatch* cur = e->batches.empty() ? nullptr : e->batches.back().get();
    if (!cur || cur->sealed) cur = new_batch(e);
    const uint32_t slot = cur->count++;
    if (slot == 0) cur->t0 = std::chrono::steady_clock::now();
    memcpy(cur->planes.data() + slot * words, planes_one, words * 8);
    if (list) {
        legal_append(cur->legal_idx, cur->legal_off, slot, list, legal_count);
        cur->kind.resize(slot, 0);
        cur->kind.push_back(1);
        cur->legal_leaves += 1;
    }
    *ticket = (cur->seq << 32) | slot;
    const bool full = cur->count == e->cfg.max_batch;
    if (full) {
        cur->sealed = true;
        new_batch(e);
    }
    lk.unlock();
    if (full || slot == 0) e->srv_cv.notify_all();
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_submit(cattus_eval* e, const uint64_t* planes_one, uint64_t* ticket) {
    if (!e || !planes_one || !ticket) return fail(CATTUS_E_INVALID, "NULL argument");
    return submit_leaf(e, planes_one, nullptr, 0, ticket);
}

// The lanes' ragged buffers (Lane::rag_*), once per evaluator, at its first cattus_hip_submit_legal: each lane is taken in turn, so the call waits
// for the batch in flight on it.  An evaluator that never submits a list allocates none of this.
static int ragged_buffers(cattus_eval* e) {
    if (e->ragged_ready.load(std::memory_order_acquire)) return CATTUS_OK;
    std::lock_guard<std::mutex> once(e->ragged_mu);
    if (e->ragged_ready.load(std::memory_order_relaxed)) return CATTUS_OK;
    HIP_TRY(hipSetDevice(e->device));
    const size_t B = e->cfg.max_batch, entries = B * LEGAL_CAP;
    for (Lane& L : e->lanes) {
        std::lock_guard<std::mutex> lk(L.mu);
        int rc = CATTUS_OK;
        if ((!L.rag_idx.p && (rc = L.rag_idx.alloc(entries * 2))) || (!L.rag_off.p && (rc = L.rag_off.alloc((B + 1) * 4))) ||
            (!L.rag_probs.p && (rc = L.rag_probs.alloc(entries * 4))) || (!L.h_rag_idx.p && (rc = L.h_rag_idx.alloc(entries * 2))) ||
            (!L.h_rag_off.p && (rc = L.h_rag_off.alloc((B + 1) * 4))) || (!L.h_rag_probs.p && (rc = L.h_rag_probs.alloc(entries * 4))))
            return rc;
    }
    e->ragged_ready.store(true, std::memory_order_release);
    return CATTUS_OK;
}

static const char* legal_fault_text(LegalFault f) {
    return f == LEGAL_TOO_LONG ? "more than 1024 legal moves" : f == LEGAL_BAD_INDEX ? "a policy index outside the network's moves" : "offsets do not ascend from 0";
}

CATTUS_API int cattus_hip_submit_legal(cattus_eval* e, const uint64_t* planes_one, const uint16_t* legal_idx, uint32_t legal_count, uint64_t* ticket) {
    if (!e || !planes_one || !ticket || (!legal_idx && legal_count)) return fail(CATTUS_E_INVALID, "NULL argument");
    uint32_t at = 0;
    if (const LegalFault f = legal_list_check(legal_idx, legal_count, e->d.moves, &at))
        return fail(CATTUS_E_INVALID, "legal list of %u entries: %s (position %u, moves %u)", legal_count, legal_fault_text(f), at, e->d.moves);
    if (int rc = ragged_buffers(e)) return rc;
    static const uint16_t none = 0;  // a list of no entries still is one: the leaf is a legal leaf with an empty span
    return submit_leaf(e, planes_one, legal_idx ? legal_idx : &none, legal_count, ticket);
}

// cattus_hip_wait (legal == false: policy receives the logits) and cattus_hip_wait_legal (legal == true: probs receives the leaf's legal_count
// probabilities).  A ticket of the other kind is refused before anything is waited for or marked: the right call can still claim it.
static int wait_leaf(cattus_eval* e, uint64_t ticket, bool legal, float* out, float* value) {
    const uint64_t seq = ticket >> 32;
    const uint32_t slot = (uint32_t)ticket;
    std::unique_lock<std::mutex> lk(e->srv_mu);
    for (;;) {
        ServerBatch* b = nullptr;
        for (auto& x : e->batches)
            if (x->seq == seq) {
                b = x.get();
                break;
            }
        if (!b || slot >= b->count) return fail(CATTUS_E_STATE, "unknown or already collected ticket %llu", (unsigned long long)ticket);
        if (b->is_legal(slot) != legal)
            return fail(CATTUS_E_INVALID, "ticket %llu is a %s: claim it with %s", (unsigned long long)ticket,
                        legal ? "cattus_hip_submit ticket" : "cattus_hip_submit_legal ticket", legal ? "cattus_hip_wait" : "cattus_hip_wait_legal");
        if (b->done) {
            // a ticket is single-use whether its batch succeeded or not: the last waiter through erases the batch
            if (slot >= b->taken.size() || b->taken[slot]) return fail(CATTUS_E_STATE, "ticket %llu was already collected", (unsigned long long)ticket);
            if (legal && !out && b->status == CATTUS_OK && legal_span(b->legal_off.data(), slot).count)
                return fail(CATTUS_E_INVALID, "NULL probs for a leaf with legal moves");
            b->taken[slot] = 1;
            const int status = b->status;
            if (status != CATTUS_OK) {
                g_last_error = b->error;
            } else {
                if (legal) {
                    const LegalSpan sp = legal_span(b->legal_off.data(), slot);
                    if (sp.count) memcpy(out, b->probs.data() + sp.begin, (size_t)sp.count * 4);
                } else {
                    memcpy(out, b->policy.data() + (size_t)slot * e->d.moves, (size_t)e->d.moves * 4);
                }
                *value = b->value[slot];
            }
            if (++b->collected == b->count) {
                for (auto it = e->batches.begin(); it != e->batches.end(); ++it)
                    if (it->get() == b) {
                        e->batches.erase(it);
                        break;
                    }
            }
            return status;
        }
        if (e->stop) return fail(CATTUS_E_STATE, "evaluator is shutting down");
        e->done_cv.wait(lk);
    }
}

CATTUS_API int cattus_hip_wait(cattus_eval* e, uint64_t ticket, float* policy, float* value) {
    if (!e || !policy || !value) return fail(CATTUS_E_INVALID, "NULL argument");
    return wait_leaf(e, ticket, false, policy, value);
}

CATTUS_API int cattus_hip_wait_legal(cattus_eval* e, uint64_t ticket, float* probs, float* value) {
    if (!e || !value) return fail(CATTUS_E_INVALID, "NULL argument");  // probs may be NULL for a leaf without a legal move
    return wait_leaf(e, ticket, true, probs, value);
}

CATTUS_API int cattus_hip_apply_legal(cattus_eval* e, const uint64_t* planes, uint32_t n, const uint16_t* legal_idx, const uint32_t* legal_off, float* probs,
                                      float* value) {
    if (!e || !planes || !legal_off || !value) return fail(CATTUS_E_INVALID, "NULL argument");
    // the whole table is checked before the first leaf is queued: a refused call leaves nothing behind
    uint32_t at = 0;
    if (const LegalFault f = legal_offsets_check(legal_off, n, &at)) return fail(CATTUS_E_INVALID, "legal_off: %s (leaf %u)", legal_fault_text(f), at);
    const uint32_t total = legal_off[n];
    if (total && (!legal_idx || !probs)) return fail(CATTUS_E_INVALID, "NULL argument");
    for (uint32_t k = 0; k < total; k++)
        if (legal_idx[k] >= e->d.moves)
            return fail(CATTUS_E_INVALID, "leaf %u: policy index %u >= %u", legal_owner(legal_off, n, k), legal_idx[k], e->d.moves);
    const size_t words = (size_t)e->d.planes * e->cfg.plane_words;
    std::vector<uint64_t> tickets(n);
    int rc = CATTUS_OK;
    uint32_t submitted = 0;
    for (; submitted < n; submitted++) {
        const LegalSpan sp = legal_span(legal_off, submitted);
        if ((rc = cattus_hip_submit_legal(e, planes + submitted * words, legal_idx + sp.begin, sp.count, &tickets[submitted]))) break;
    }
    // as cattus_hip_apply: every submitted ticket is collected, also after a failure
    for (uint32_t i = 0; i < submitted; i++) {
        const int wrc = cattus_hip_wait_legal(e, tickets[i], probs + legal_off[i], value + i);
        if (wrc && !rc) rc = wrc;
    }
    return rc;
}

CATTUS_API int cattus_hip_apply(cattus_eval* e, const uint64_t* planes, uint32_t n, float* policy, float* value) {
    if (!e || !planes || !policy || !value) return fail(CATTUS_E_INVALID, "NULL argument");
    const size_t words = (size_t)e->d.planes * e->cfg.plane_words;
    std::vector<uint64_t> tickets(n);
    int rc = CATTUS_OK;
    uint32_t submitted = 0;
    for (; submitted < n; submitted++)
        if ((rc = cattus_hip_submit(e, planes + submitted * words, &tickets[submitted]))) break;
    // every submitted ticket is collected, also after a failure, so that no batch stays behind
    for (uint32_t i = 0; i < submitted; i++) {
        const int wrc = cattus_hip_wait(e, tickets[i], policy + (size_t)i * e->d.moves, value + i);
        if (wrc && !rc) rc = wrc;
    }
    return rc;
}

CATTUS_API int cattus_hip_flush(cattus_eval* e) {
    if (!e) return fail(CATTUS_E_INVALID, "NULL argument");
    {
        std::lock_guard<std::mutex> lk(e->srv_mu);
        e->flush_req = true;
    }
    e->srv_cv.notify_all();
    return CATTUS_OK;
}

CATTUS_API void* cattus_hip_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) {
        fail(CATTUS_E_NOMEM, "hipHostMalloc(%zu) failed", bytes);
        return nullptr;
    }
    std::unique_lock<std::shared_mutex> lk(g_pin_mu);
    g_pinned[(const char*)p] = bytes ? bytes : 16;
    return p;
}

CATTUS_API void cattus_hip_host_free(void* p) {
    if (!p) return;
    {
        std::unique_lock<std::shared_mutex> lk(g_pin_mu);
        g_pinned.erase((const char*)p);
    }
    (void)hipHostFree(p);
}

CATTUS_API int cattus_hip_stats(cattus_eval* e, cattus_stats* out) {
    if (!e || !out) return fail(CATTUS_E_INVALID, "NULL argument");
    unsigned sat = 0;
    if (e->d_saturated.p) {  // a 4-byte read of the sticky device counter (batches still in flight may add to it later)
        HIP_TRY(hipSetDevice(e->device));
        HIP_TRY(hipMemcpy(&sat, e->d_saturated.p, sizeof sat, hipMemcpyDeviceToHost));
    }
    std::lock_guard<std::mutex> lk(e->stat_mu);
    e->stats.saturated = sat;
    *out = e->stats;
    return CATTUS_OK;
}

namespace {

// Act::F32 is the exact tower under dtype f32; dtype f32w runs the same Act on a tower of its own bits, which has a shadow like any other
bool exact_f32(const cattus_eval* e) { return e->act == Act::F32 && e->plan.kind != TowerKind::WinoF32; }

// What cattus_hip_verify and cattus_hip_trace ask before anything else: is there an exact tower to hold this evaluator to, and is `weights`
// the blob it was created from (the evaluator keeps no host copy of it)?
int shadow_args(const cattus_eval* e, const void* weights, size_t nbytes, const char* what) {
    if (e->plan.kind == TowerKind::Simple) return fail(CATTUS_E_UNSUPPORTED, "a SimpleTwoHeadedModel runs in f32 whatever its dtype: there is nothing to %s it against", what);
    if (exact_f32(e)) return fail(CATTUS_E_UNSUPPORTED, "a dtype f32 evaluator is the exact tower: its shadow would be itself");
    if (nbytes != e->blob_bytes || blob_hash64(weights, nbytes) != e->blob_hash)
        return fail(CATTUS_E_INVALID, "%s: this is not the weight blob the evaluator was created from", what);
    return CATTUS_OK;
}

// The shadow: a dtype f32 evaluator of the same blob on the same device with the same max_batch and plane_words, no switches, that `e` owns.
// Built by whichever of verify and trace comes first; the caller holds every lane mutex (shadow_args passed).
int ensure_shadow(cattus_eval* e, const void* weights, size_t nbytes) {
    if (e->shadow) return CATTUS_OK;
    HIP_TRY(hipSetDevice(e->device));
    cattus_eval_config scfg = e->cfg;
    scfg.dtype = CATTUS_DTYPE_F32, scfg.tower_form = CATTUS_TOWER_AUTO, scfg.tail_leaves = 0;
    return create_impl(weights, nbytes, &scfg, nullptr, &e->shadow);  // CATTUS_E_NOMEM where it does not fit
}

}  // namespace

CATTUS_API int cattus_hip_verify(cattus_eval* e, const void* weights, size_t nbytes, uint32_t every) {
    if (!e || !weights) return fail(CATTUS_E_INVALID, "NULL argument");
    if (int rc = shadow_args(e, weights, nbytes, "verify")) return rc;
    std::unique_lock<std::mutex> held[NLANES];  // every lane, in lane order: batches in flight finish first, none starts meanwhile
    for (int i = 0; i < NLANES; i++) held[i] = std::unique_lock<std::mutex>(e->lanes[i].mu);
    if (every) {
        if (int rc = ensure_shadow(e, weights, nbytes)) return rc;
        const size_t bytes = (size_t)e->cfg.max_batch * 2 * sizeof(VerifyRecord);
        for (Lane& L : e->lanes) {  // (a shadow that trace built first, or one kept from an attempt that ran out of memory here, stays: the evaluator owns it)
            int rc = CATTUS_OK;
            if (!L.d_verify.p) rc = L.d_verify.alloc(bytes);
            if (!rc && !L.h_verify.p) rc = L.h_verify.alloc(bytes);
            if (!rc && !L.d_prior.p) rc = L.d_prior.alloc((size_t)e->cfg.max_batch * sizeof(PriorRecord));
            if (!rc && !L.h_prior.p) rc = L.h_prior.alloc((size_t)e->cfg.max_batch * sizeof(PriorRecord));
            if (rc) return rc;
        }
    }
    e->verify_every = every;  // 0: off -- the record and the shadow stay, and turning it on again goes on counting
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_points(const cattus_eval* e, uint32_t* points) {
    if (!e || !points) return fail(CATTUS_E_INVALID, "NULL argument");
    if (e->plan.kind == TowerKind::Simple) return fail(CATTUS_E_UNSUPPORTED, "a SimpleTwoHeadedModel has no conv layers to observe");
    *points = net_points(e->d);
    return CATTUS_OK;
}

namespace {

// The stream shifts as the observation kernels read them, on lane L; NULL where no channel is shifted (f32, bf16, every seeded network).
int lane_shifts(cattus_eval* e, Lane& L, const int** out) {
    *out = nullptr;
    const std::vector<int>& tk = e->stream_shifts;
    if (std::none_of(tk.begin(), tk.end(), [](int t) { return t != 0; })) return CATTUS_OK;
    if (!L.d_shifts.p)
        if (int rc = L.d_shifts.upload(tk.data(), tk.size() * sizeof(int))) return rc;
    *out = L.d_shifts.as<int>();
    return CATTUS_OK;
}

// n host leaves onto lane L and through the per-layer twin with `obs` behind its layers, enqueued and not waited for.  Not a batch: nothing
// is counted and no verify ticket is taken (the kernels' own `saturated` counter counts what this pass clamps, as it does for any pass).
int enqueue_observed(cattus_eval* e, Lane& L, const uint64_t* planes, uint32_t n, const Observer& obs) {
    const size_t pbytes = (size_t)n * e->d.planes * e->cfg.plane_words * 8;
    memcpy(L.h_planes.p, planes, pbytes);
    HIP_TRY(hipMemcpyAsync(L.d_planes.p, L.h_planes.p, pbytes, hipMemcpyHostToDevice, L.stream));
    return enqueue_forward(e, L, L.d_planes.as<uint64_t>(), n, L.d_policy.as<float>(), L.d_value.as<float>(), L.stream, nullptr, &obs);
}

// `result` (bytes from d_result) and the pass's own outputs back to the host; returns with the lane's stream drained.
int collect_observed(cattus_eval* e, Lane& L, uint32_t n, void* result, const void* d_result, size_t bytes, float* policy, float* value) {
    HIP_TRY(hipMemcpyAsync(result, d_result, bytes, hipMemcpyDeviceToHost, L.stream));
    if (policy) HIP_TRY(hipMemcpyAsync(L.h_policy.p, L.d_policy.p, (size_t)n * e->d.moves * 4, hipMemcpyDeviceToHost, L.stream));
    if (value) HIP_TRY(hipMemcpyAsync(L.h_value.p, L.d_value.p, (size_t)n * 4, hipMemcpyDeviceToHost, L.stream));
    HIP_TRY(hipStreamSynchronize(L.stream));
    if (policy) memcpy(policy, L.h_policy.p, (size_t)n * e->d.moves * 4);
    if (value) memcpy(value, L.h_value.p, (size_t)n * 4);
    return CATTUS_OK;
}

}  // namespace

CATTUS_API int cattus_hip_tap(cattus_eval* e, const uint64_t* planes, uint32_t n, uint32_t point, float* out, float* policy, float* value) {
    if (!e || !planes || !out) return fail(CATTUS_E_INVALID, "NULL argument");
    if (e->plan.kind == TowerKind::Simple) return fail(CATTUS_E_UNSUPPORTED, "a SimpleTwoHeadedModel has no conv layers to tap");
    const cattus_net_desc& d = e->d;
    const uint32_t P = net_points(d), ocn = d.vhc + d.phc;
    if (n < 1 || n > e->cfg.max_batch) return fail(CATTUS_E_INVALID, "invalid sample len %u, 1..=%u", n, e->cfg.max_batch);
    if (point >= P) return fail(CATTUS_E_INVALID, "tap: point %u, the network has points 0..=%u", point, P - 1);
    std::unique_lock<std::mutex> lk;
    Lane& L = take_lane(e, lk);
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if (!L.d_tap.p && (rc = L.d_tap.alloc((size_t)e->cfg.max_batch * std::max(d.filters, ocn) * e->hw * 4))) return rc;
    const int* shifts = nullptr;
    if ((rc = lane_shifts(e, L, &shifts))) return rc;
    size_t bytes = 0;
    const Observer tap = [&](uint32_t at, const void* buf, const TapSource& src) {
        if (at != point) return CATTUS_OK;
        // the residual stream (the even points) is what the f16 towers carry at 2^t_k; the middle activations and the heads are at 2^0
        launch_tap(buf, src, at % 2 == 0 ? shifts : nullptr, n, L.d_tap.as<float>(), L.stream);
        bytes = (size_t)n * src.C * src.hw * 4;
        return CATTUS_OK;
    };
    if ((rc = enqueue_observed(e, L, planes, n, tap))) return rc;
    if (!bytes) return fail(CATTUS_E_STATE, "tap: the pass never reached point %u", point);
    return collect_observed(e, L, n, out, L.d_tap.p, bytes, policy, value);
}

CATTUS_API int cattus_hip_trace(cattus_eval* e, const void* weights, size_t nbytes, const uint64_t* planes, uint32_t n, cattus_trace_record* out, uint32_t points,
                                float* policy, float* value) {
    static_assert(sizeof(cattus_trace_record) == sizeof(TraceRecord) && offsetof(cattus_trace_record, rms_diff) == offsetof(TraceRecord, rms_diff) &&
                      offsetof(cattus_trace_record, flags) == offsetof(TraceRecord, flags),
                  "the kernel's record is the header's");
    if (!e || !weights || !planes || !out) return fail(CATTUS_E_INVALID, "NULL argument");
    if (int rc = shadow_args(e, weights, nbytes, "trace")) return rc;
    const cattus_net_desc& d = e->d;
    const uint32_t P = net_points(d);
    if (points != P) return fail(CATTUS_E_INVALID, "trace: records for %u points asked for, the network has %u", points, P);
    if (n < 1 || n > e->cfg.max_batch) return fail(CATTUS_E_INVALID, "invalid sample len %u, 1..=%u", n, e->cfg.max_batch);
    {
        std::unique_lock<std::mutex> held[NLANES];  // as cattus_hip_verify: the shadow changes only with every lane mutex held
        for (int i = 0; i < NLANES; i++) held[i] = std::unique_lock<std::mutex>(e->lanes[i].mu);
        if (int rc = ensure_shadow(e, weights, nbytes)) return rc;
    }
    cattus_eval* const sh = e->shadow;  // never replaced once built
    if (sh->plan.kind != TowerKind::PerLayer || sh->slots != e->slots) return fail(CATTUS_E_UNSUPPORTED, "trace: the f32 shadow of this network is not a per-layer MFMA tower");
    std::unique_lock<std::mutex> lk;
    Lane& L = take_lane(e, lk);
    Lane& SL = sh->lanes[&L - e->lanes];  // used under this evaluator's lane mutex and by nobody else, as in a verified batch
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if (!L.d_trace.p && (rc = L.d_trace.alloc((size_t)P * e->cfg.max_batch * sizeof(TraceRecord)))) return rc;
    const int* shifts = nullptr;
    if ((rc = lane_shifts(e, L, &shifts))) return rc;
    // The shadow's f32 per-layer pass on the same device-resident leaves, advanced one layer per point of the evaluator's pass, on the same
    // stream: behind layer l of both the compare kernel reads the two buffers before either pass overwrites them.  Nothing grows with the
    // number of points but the records.
    Forward sf{sh, SL, L.d_planes.as<uint64_t>(), n, padded_boards(sh, n), SL.d_policy.as<float>(), SL.d_value.as<float>(), L.stream, nullptr, nullptr};
    const Observer lockstep = [&](uint32_t at, const void* buf, const TapSource& src) {
        TraceRecord* const rec = L.d_trace.as<TraceRecord>() + (size_t)at * n;
        if (at + 1 < P) {
            const void* ref = sf.per_layer_step(at);
            launch_trace_compare(buf, src, at % 2 == 0 ? shifts : nullptr, ref, sf.tower_source(at), n, rec, L.stream);
        } else {
            sf.heads_mfma(sf.a);
            launch_trace_compare(buf, src, nullptr, SL.hv.p, sf.head_source(), n, rec, L.stream);
        }
        return CATTUS_OK;
    };
    if ((rc = enqueue_observed(e, L, planes, n, lockstep))) return rc;
    return collect_observed(e, L, n, out, L.d_trace.p, (size_t)P * n * sizeof(TraceRecord), policy, value);
}

CATTUS_API int cattus_hip_verify_stats(cattus_eval* e, cattus_verify_stats* out) {
    if (!e || !out) return fail(CATTUS_E_INVALID, "NULL argument");
    if (out->struct_size != sizeof(cattus_verify_stats)) return fail(CATTUS_E_INVALID, "cattus_verify_stats.struct_size mismatch");
    const uint32_t every = e->verify_every.load(std::memory_order_relaxed);
    std::lock_guard<std::mutex> lk(e->stat_mu);
    const cattus_eval::Verified& v = e->verified;
    *out = cattus_verify_stats{(uint32_t)sizeof(cattus_verify_stats), every, v.batches, v.leaves, v.leaves_outside, v.max_dlogit, v.logit, v.logit_ref, v.move,
                               v.max_dvalue, v.value, v.value_ref, 0};
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_verify_worst_planes(cattus_eval* e, uint64_t* planes) {
    if (!e || !planes) return fail(CATTUS_E_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(e->stat_mu);
    if (e->verified.worst_planes.empty()) return fail(CATTUS_E_STATE, "no leaf has been verified yet");
    std::copy(e->verified.worst_planes.begin(), e->verified.worst_planes.end(), planes);
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_verify_prior_stats(cattus_eval* e, cattus_prior_stats* out) {
    if (!e || !out) return fail(CATTUS_E_INVALID, "NULL argument");
    if (out->struct_size != sizeof(cattus_prior_stats)) return fail(CATTUS_E_INVALID, "cattus_prior_stats.struct_size mismatch");
    if (e->plan.kind == TowerKind::Simple || exact_f32(e))
        return fail(CATTUS_E_UNSUPPORTED, "a dtype f32 evaluator and a SimpleTwoHeadedModel have no shadow to compare priors with");
    std::lock_guard<std::mutex> lk(e->stat_mu);
    const PriorStats& s = e->priors;
    *out = cattus_prior_stats{};
    out->struct_size = (uint32_t)sizeof(cattus_prior_stats);
    out->batches = s.batches, out->batches_without_legal = s.batches_without_legal, out->leaves = s.leaves, out->top1_flips = s.top1_flips;
    out->nonfinite = s.nonfinite, out->empty = s.empty, out->sum_tv = s.sum_tv, out->sum_regret = s.sum_regret;
    out->max_tv = s.max_tv, out->max_regret = s.max_regret, out->value_leaves = s.value_leaves, out->sum_dvalue = s.sum_dvalue;
    static_assert(sizeof(out->tv_hist) == sizeof(s.tv_hist), "eight buckets on both sides");
    memcpy(out->tv_hist, s.tv_hist, sizeof(s.tv_hist));
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_verify_worst_prior(cattus_eval* e, uint64_t* planes, uint16_t* legal_idx, uint32_t cap, uint32_t* legal_count, uint32_t* top,
                                             uint32_t* top_ref) {
    if (!e || !planes || !legal_idx || !legal_count || !top || !top_ref) return fail(CATTUS_E_INVALID, "NULL argument");
    if (e->plan.kind == TowerKind::Simple || exact_f32(e))
        return fail(CATTUS_E_UNSUPPORTED, "a dtype f32 evaluator and a SimpleTwoHeadedModel have no shadow to compare priors with");
    std::lock_guard<std::mutex> lk(e->stat_mu);
    const cattus_eval::WorstPrior& w = e->worst_prior;
    if (!e->priors.seeded) return fail(CATTUS_E_STATE, "no leaf's priors have been compared yet");
    if (cap < w.legal.size()) return fail(CATTUS_E_INVALID, "verify_worst_prior: the leaf has %zu legal moves, cap is %u", w.legal.size(), cap);
    std::copy(w.planes.begin(), w.planes.end(), planes);
    std::copy(w.legal.begin(), w.legal.end(), legal_idx);
    *legal_count = (uint32_t)w.legal.size(), *top = w.top, *top_ref = w.top_ref;
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_compare_priors(int device, const float* probs_a, const float* probs_b, const uint16_t* legal_count, uint32_t n, uint32_t L,
                                         const float* value_a, const float* value_b, void* records) {
    if (!probs_a || !probs_b || !legal_count || !value_a || !value_b || !records) return fail(CATTUS_E_INVALID, "NULL argument");
    if (n < 1 || L < 1 || L > 1024 || n > (1u << 20)) return fail(CATTUS_E_INVALID, "compare_priors: %u leaves of stride %u", n, L);
    int ndev = 0;
    hipError_t herr = hipGetDeviceCount(&ndev);
    if (herr != hipSuccess || device < 0 || device >= ndev)
        return fail(CATTUS_E_DEVICE, "no usable HIP device %d (%s); this library has no CPU path", device, hipGetErrorString(herr));
    HIP_TRY(hipSetDevice(device));
    DevBuf pa, pb, cnt, va, vb, rec;
    int rc;
    const size_t pbytes = (size_t)n * L * 4;
    if ((rc = pa.upload(probs_a, pbytes)) || (rc = pb.upload(probs_b, pbytes)) || (rc = cnt.upload(legal_count, (size_t)n * 2)) ||
        (rc = va.upload(value_a, (size_t)n * 4)) || (rc = vb.upload(value_b, (size_t)n * 4)) || (rc = rec.alloc((size_t)n * sizeof(PriorRecord))))
        return rc;
    launch_verify_priors(pa.as<float>(), pb.as<float>(), cnt.as<uint16_t>(), va.as<float>(), vb.as<float>(), n, L, rec.as<PriorRecord>(), nullptr);
    if (hipError_t err = hipGetLastError()) return fail(CATTUS_E_DEVICE, "kernel launch failed: %s", hipGetErrorString(err));
    HIP_TRY(hipMemcpy(records, rec.p, (size_t)n * sizeof(PriorRecord), hipMemcpyDeviceToHost));
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_compare_outputs(int device, const float* policy_a, const float* policy_b, const float* value_a, const float* value_b, uint32_t n,
                                          uint32_t moves, void* records) {
    if (!policy_a || !policy_b || !value_a || !value_b || !records) return fail(CATTUS_E_INVALID, "NULL argument");
    if (n < 1 || moves < 1 || (uint64_t)n * moves > (1ull << 30)) return fail(CATTUS_E_INVALID, "compare_outputs: %u leaves of %u moves", n, moves);
    int ndev = 0;
    hipError_t herr = hipGetDeviceCount(&ndev);
    if (herr != hipSuccess || device < 0 || device >= ndev)
        return fail(CATTUS_E_DEVICE, "no usable HIP device %d (%s); this library has no CPU path", device, hipGetErrorString(herr));
    HIP_TRY(hipSetDevice(device));
    DevBuf pa, pb, va, vb, rec;
    int rc;
    const size_t pbytes = (size_t)n * moves * 4;
    if ((rc = pa.upload(policy_a, pbytes)) || (rc = pb.upload(policy_b, pbytes)) || (rc = va.upload(value_a, (size_t)n * 4)) || (rc = vb.upload(value_b, (size_t)n * 4)) ||
        (rc = rec.alloc((size_t)n * sizeof(VerifyRecord))))
        return rc;
    launch_verify_outputs(pa.as<float>(), pb.as<float>(), va.as<float>(), vb.as<float>(), n, moves, rec.as<VerifyRecord>(), nullptr, nullptr);
    if (hipError_t err = hipGetLastError()) return fail(CATTUS_E_DEVICE, "kernel launch failed: %s", hipGetErrorString(err));
    HIP_TRY(hipMemcpy(records, rec.p, (size_t)n * sizeof(VerifyRecord), hipMemcpyDeviceToHost));
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_time_tower(cattus_eval* e, uint32_t n, uint32_t reps, float* avg_launch_us, uint32_t* launches) {
    if (!e || !avg_launch_us || !launches) return fail(CATTUS_E_INVALID, "NULL argument");
    if (n < 1 || n > e->cfg.max_batch || reps < 1) return fail(CATTUS_E_INVALID, "bad n/reps");
    if (e->plan.kind == TowerKind::Simple) return fail(CATTUS_E_UNSUPPORTED, "a SimpleTwoHeadedModel has no conv tower to time");
    Lane& L = e->lanes[0];
    std::lock_guard<std::mutex> lk(L.mu);
    HIP_TRY(hipSetDevice(e->device));
    // (the one-launch Winograd tower is reported per LAYER: its duration + the stem's over 1 + 2 blocks, so that a caller's
    // flops-per-launch arithmetic does not change with how the layers are launched)
    const uint32_t per_fwd = e->plan.resident() ? 1 : 1 + 2 * e->d.blocks;
    TowerTimer tt;
    tt.ev.resize((size_t)2 * per_fwd);
    for (auto& ev : tt.ev) HIP_TRY(hipEventCreate(&ev));
    HIP_TRY(hipMemsetAsync(L.d_planes.p, 0x5a, (size_t)n * e->d.planes * e->cfg.plane_words * 8, L.stream));
    double total_ms = 0;
    int rc = CATTUS_OK;
    for (uint32_t rep = 0; rep < reps + 1 && rc == CATTUS_OK; rep++) {  // first pass is warm-up
        tt.used = 0;
        rc = enqueue_forward(e, L, L.d_planes.as<uint64_t>(), n, L.d_policy.as<float>(), L.d_value.as<float>(), L.stream, &tt);
        if (rc) break;
        hipError_t err = hipStreamSynchronize(L.stream);
        if (err != hipSuccess) {
            rc = fail(CATTUS_E_DEVICE, "hipStreamSynchronize: %s", hipGetErrorString(err));
            break;
        }
        if (rep == 0) continue;
        for (size_t i = 0; i + 1 < tt.used; i += 2) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, tt.ev[i], tt.ev[i + 1]);
            total_ms += ms;
        }
    }
    for (auto& ev : tt.ev) (void)hipEventDestroy(ev);
    if (rc) return rc;
    *launches = per_fwd;
    *avg_launch_us = (float)(total_ms * 1000.0 / ((double)reps * per_fwd));
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_mfma_sustained(cattus_eval* e, double seconds, double* tflops) {
    if (!e || !tflops) return fail(CATTUS_E_INVALID, "NULL argument");
    if (!(seconds > 0) || seconds > 30) return fail(CATTUS_E_INVALID, "seconds out of range");
    Lane& L = e->lanes[0];
    std::lock_guard<std::mutex> lk(L.mu);
    HIP_TRY(hipSetDevice(e->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, e->device));
    const int cus = prop.multiProcessorCount;
    DevBuf out;
    int rc = out.alloc((size_t)cus * 256 * 4);
    if (rc) return rc;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    // launches of ~50 us (the length of a conv layer), groups of 50, until `seconds` have passed: the last group's rate
    const int iters = e->act == Act::F32 ? 480 : 640, reps = 50;
    double rate = 0, elapsed = 0;
    while (elapsed < seconds) {
        double flop = 0;
        (void)hipEventRecord(e0, L.stream);
        for (int r = 0; r < reps; r++) flop += launch_mfma_sustain(e->act, cus, iters, out.as<float>(), L.stream);
        (void)hipEventRecord(e1, L.stream);
        const hipError_t err = hipEventSynchronize(e1);
        if (err != hipSuccess) {
            (void)hipEventDestroy(e0), (void)hipEventDestroy(e1);
            return fail(CATTUS_E_DEVICE, "hipEventSynchronize: %s", hipGetErrorString(err));
        }
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        elapsed += ms * 1e-3;
        rate = flop / (ms * 1e-3) / 1e12;
    }
    (void)hipEventDestroy(e0), (void)hipEventDestroy(e1);
    *tflops = rate;
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_planes_to_tensor_device(const uint64_t* d_planes, uint32_t n, uint32_t C, uint32_t plane_words,
                                                  uint32_t S, uint32_t batch, float* d_out, void* stream) {
    if (!d_planes || !d_out) return fail(CATTUS_E_INVALID, "NULL argument");
    if (n < 1 || n > batch) return fail(CATTUS_E_INVALID, "invalid sample len %u, 1..=%u", n, batch);
    if (S < 1 || S > 11 || plane_words * 64 < S * S || !C) return fail(CATTUS_E_INVALID, "bad plane geometry");
    launch_planes_to_tensor_nchw(d_planes, n, C, plane_words, S, batch, d_out, (hipStream_t)stream);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(CATTUS_E_DEVICE, "kernel launch failed: %s", hipGetErrorString(err));
    return CATTUS_OK;
}

CATTUS_API int cattus_hip_planes_to_tensor(int device, const uint64_t* planes, uint32_t n, uint32_t C, uint32_t plane_words,
                                           uint32_t S, uint32_t batch, float* out) {
    if (!planes || !out) return fail(CATTUS_E_INVALID, "NULL argument");
    if (n < 1 || n > batch) return fail(CATTUS_E_INVALID, "invalid sample len %u, 1..=%u", n, batch);
    if (S < 1 || S > 11 || plane_words * 64 < S * S || !C) return fail(CATTUS_E_INVALID, "bad plane geometry");
    int ndev = 0;
    hipError_t herr = hipGetDeviceCount(&ndev);
    if (herr != hipSuccess || device < 0 || device >= ndev)
        return fail(CATTUS_E_DEVICE, "no usable HIP device %d (%s); this library has no CPU path", device, hipGetErrorString(herr));
    HIP_TRY(hipSetDevice(device));
    DevBuf dp, dout;
    int rc;
    const size_t pbytes = (size_t)n * C * plane_words * 8, obytes = (size_t)batch * C * S * S * 4;
    if ((rc = dp.upload(planes, pbytes))) return rc;
    if ((rc = dout.alloc(obytes))) return rc;
    rc = cattus_hip_planes_to_tensor_device(dp.as<uint64_t>(), n, C, plane_words, S, batch, dout.as<float>(), nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out, dout.p, obytes, hipMemcpyDeviceToHost));
    return CATTUS_OK;
}
