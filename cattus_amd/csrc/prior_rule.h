// The prior rule of cattus_hip_verify: how far are the priors and the value a search receives from this evaluator from the ones the exact
// network would have handed it for the same legal moves?  Pure functions for the host and the device alike -- no HIP call, nothing of the
// evaluator -- so that every edge can be checked without a GPU (tests/test_prior_rule.py) and the kernel (kernels.hip,
// verify_priors_kernel), the host restatement and the evaluator's fold say the same thing.  verify_rule.h holds the logits to a bar; this
// file sets none: it measures, in the quantities a PUCT search consumes.
//
// One leaf: pa[0..L) this evaluator's probs row as cattus_hip_eval_legal returns it, pb[0..L) legal_softmax_kernel on the shadow's logits
// with the same legal list, c = min(legal_count, L).  Its record, 32 bytes:
//   tv       float(0.5 * sum_k |double(pa[k]) - double(pb[k])|) over k < c, summed as a wave sums it: lane l of 64 takes k = l, l + 64, ...
//            ascending in double (prior_lane_sum), the 64 partials are combined by the xor butterfly 32, 16, .., 1
//            (new[l] = old[l] + old[l ^ off]) and lane 0 is taken (prior_tv_close): the same bytes on a CPU
//   top_a, top_b   position in the legal list of the largest pa / pb, the lowest on ties (verify_take_max's order-free combine); a NaN
//            takes no part, and a row without a comparable entry reports 0
//   regret   pb[top_b] - pb[top_a]: the prior mass the exact network's favourite loses; exactly 0 when the favourites agree, >= 0 otherwise
//   max_dp, k_max  the largest float(|double(pa[k]) - double(pb[k])|) and the lowest k that holds it (NaN differences take no part; 0 at 0
//            where none is positive)
//   count    c
//   flags    bit 0 a non-finite probability on either side (tv and regret are then the one quiet NaN 0x7fc00000), bit 1 c == 0,
//            bit 2 legal_count > L, bit 3 a non-finite value on either side
//   dvalue   verify_rule.h's dvalue of the two values
// A leaf with bit 0 or bit 1 set is counted (nonfinite / empty) and enters no sum, maximum or histogram (prior_fold).
#pragma once
#include "verify_rule.h"

namespace cattus {

struct PriorRecord {
    float tv;
    uint32_t top_a, top_b;
    float regret, max_dp;
    uint32_t k_max;
    uint16_t count, flags;
    float dvalue;
};
static_assert(sizeof(PriorRecord) == 32, "a record is two 16-byte stores");
constexpr uint16_t PRIOR_NONFINITE = 1, PRIOR_EMPTY = 2, PRIOR_TRUNCATED = 4, PRIOR_VALUE_NONFINITE = 8;
constexpr uint32_t PRIOR_LANES = 64;

CATTUS_HD inline float prior_qnan() {
    const uint32_t qnan = 0x7fc00000u;
    float f;
    memcpy(&f, &qnan, 4);
    return f;
}

// Lane `lane`'s share of sum_k |pa[k] - pb[k]|: k = lane, lane + 64, ... ascending, in double.
CATTUS_HD inline double prior_lane_sum(const float* pa, const float* pb, uint32_t c, uint32_t lane) {
    double s = 0.0;
    for (uint32_t k = lane; k < c; k += PRIOR_LANES) s += fabs((double)pa[k] - (double)pb[k]);
    return s;
}
// One step of the butterfly, and what lane 0 makes of its result.
CATTUS_HD inline double prior_combine(double mine, double other) { return mine + other; }
CATTUS_HD inline float prior_tv_close(double total) { return (float)(0.5 * total); }

// What one lane gathers of a leaf: the two favourites, the largest difference, whether anything was non-finite.  Every member combines
// order-free, so a wave may split the moves among its lanes in any way.
struct PriorPartial {
    float a = -INFINITY, b = -INFINITY, d = 0.0f;
    uint32_t ia = 0xffffffffu, ib = 0xffffffffu, id = 0xffffffffu;
    bool nonfinite = false;
};
CATTUS_HD inline void prior_take(PriorPartial& p, float a, float b, uint32_t k) {
    verify_take_max(a, k, p.a, p.ia);
    verify_take_max(b, k, p.b, p.ib);
    verify_take_max(verify_dlogit(a, b), k, p.d, p.id);
    p.nonfinite = p.nonfinite || !verify_finite(a) || !verify_finite(b);
}
CATTUS_HD inline void prior_merge(PriorPartial& p, const PriorPartial& o) {
    verify_take_max(o.a, o.ia, p.a, p.ia);
    verify_take_max(o.b, o.ib, p.b, p.ib);
    verify_take_max(o.d, o.id, p.d, p.id);
    p.nonfinite = p.nonfinite || o.nonfinite;
}

// Closes a leaf: p merged over all its moves, total the butterfly's sum, pb the shadow's row (read at the two favourites).
CATTUS_HD inline PriorRecord prior_record(const PriorPartial& p, double total, const float* pb, uint32_t legal_count, uint32_t L, float value_a,
                                          float value_b) {
    const uint32_t c = legal_count < L ? legal_count : L;
    PriorRecord r;
    r.top_a = p.ia == 0xffffffffu ? 0u : p.ia;
    r.top_b = p.ib == 0xffffffffu ? 0u : p.ib;
    r.max_dp = p.d;
    r.k_max = p.d > 0.0f ? p.id : 0u;
    r.count = (uint16_t)c;
    r.flags = (uint16_t)((p.nonfinite ? PRIOR_NONFINITE : 0) | (c == 0 ? PRIOR_EMPTY : 0) | (legal_count > L ? PRIOR_TRUNCATED : 0) |
                         (!verify_finite(value_a) || !verify_finite(value_b) ? PRIOR_VALUE_NONFINITE : 0));
    r.tv = p.nonfinite ? prior_qnan() : prior_tv_close(total);
    r.regret = p.nonfinite ? prior_qnan() : c == 0 ? 0.0f : pb[r.top_b] - pb[r.top_a];
    r.dvalue = verify_dvalue(value_a, value_b);
    return r;
}

// The whole rule on one leaf on the host: the wave's 64 lanes one after the other, then its butterfly.
inline PriorRecord prior_leaf(const float* pa, const float* pb, uint32_t legal_count, uint32_t L, float value_a, float value_b) {
    const uint32_t c = legal_count < L ? legal_count : L;
    double part[PRIOR_LANES], next[PRIOR_LANES];
    PriorPartial all;
    for (uint32_t lane = 0; lane < PRIOR_LANES; lane++) {
        PriorPartial p;
        for (uint32_t k = lane; k < c; k += PRIOR_LANES) prior_take(p, pa[k], pb[k], k);
        prior_merge(all, p);
        part[lane] = prior_lane_sum(pa, pb, c, lane);
    }
    for (uint32_t off = PRIOR_LANES / 2; off; off >>= 1) {
        for (uint32_t lane = 0; lane < PRIOR_LANES; lane++) next[lane] = prior_combine(part[lane], part[lane ^ off]);
        memcpy(part, next, sizeof part);
    }
    return prior_record(all, part[0], pb, legal_count, L, value_a, value_b);
}

// ---- the sticky record (host) ----
// tv histogram: upper edges 1e-7, 1e-6, .., 1e-1, +inf; a leaf goes to the first bucket whose edge exceeds its tv.
constexpr int PRIOR_BUCKETS = 8;
inline int prior_bucket(float tv) {
    static const double edge[PRIOR_BUCKETS - 1] = {1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1};
    int b = 0;
    while (b < PRIOR_BUCKETS - 1 && !((double)tv < edge[b])) b++;
    return b;
}

struct PriorStats {
    uint64_t batches = 0, batches_without_legal = 0, leaves = 0, top1_flips = 0, nonfinite = 0, empty = 0;
    double sum_tv = 0.0, sum_regret = 0.0;
    float max_tv = 0.0f, max_regret = 0.0f;
    uint64_t tv_hist[PRIOR_BUCKETS] = {};
    uint64_t value_leaves = 0;
    double sum_dvalue = 0.0;
    bool seeded = false;  // a leaf holds max_tv: the first one that entered the sums, then every strictly larger one
};

// One compared leaf into the record.  True: this leaf now holds max_tv (the caller keeps its planes, legal list and favourites).
inline bool prior_fold(PriorStats& s, const PriorRecord& r) {
    s.leaves += 1;
    if (r.flags & PRIOR_NONFINITE) return s.nonfinite += 1, false;
    if (r.flags & PRIOR_EMPTY) return s.empty += 1, false;
    s.top1_flips += r.top_a != r.top_b;
    s.sum_tv += (double)r.tv;
    s.sum_regret += (double)r.regret;
    s.tv_hist[prior_bucket(r.tv)] += 1;
    if (r.regret > s.max_regret) s.max_regret = r.regret;
    if (s.seeded && !(r.tv > s.max_tv)) return false;
    s.max_tv = r.tv, s.seeded = true;
    return true;
}

// One verified leaf's value pair, of either path: finite pairs only.
inline void prior_fold_value(PriorStats& s, float value_a, float value_b) {
    if (!verify_finite(value_a) || !verify_finite(value_b)) return;
    s.value_leaves += 1;
    s.sum_dvalue += (double)verify_dvalue(value_a, value_b);
}

}  // namespace cattus
