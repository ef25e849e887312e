// The comparison rule of cattus_hip_verify: when does an evaluator's output for a leaf count as the f32 shadow tower's?  Pure functions
// of two floats, for the host and the device alike -- no HIP call, nothing of the evaluator -- so that every edge can be checked without a
// GPU (tests/test_verify_rule.py) and the kernel (kernels.hip, verify_outputs_kernel) and the host fold say the same thing.
//
// The bar is the reference's own "same net, another runtime" tolerance (training/tests/test_net_output.py:28-33; tests/helpers.py,
// REF_POLICY_RTOL / REF_POLICY_ATOL / REF_VALUE_REL / REF_VALUE_ABS), with b the shadow.  All arithmetic in double: the difference of two
// floats is exact there, and so is every product below up to one rounding that both sides of this file's users make alike.
//   logit   inside when |a - b| <= 1e-6 + 1e-3 |b|                       (numpy.isclose)
//   value   inside when |a - b| <= max(1e-5 max(|a|, |b|), 1e-6)         (math.isclose)
//   a non-finite operand is outside, two equal infinities included: only finite pairs are judged
//   two scrubbed logits (both f32::MIN, net/mod.rs:56-61) are finite and equal: difference 0, inside
//   leaf    outside when its value is outside or any of its logits is
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define CATTUS_HD __host__ __device__
#else
#define CATTUS_HD
#endif

namespace cattus {

constexpr double VERIFY_POLICY_RTOL = 1e-3, VERIFY_POLICY_ATOL = 1e-6;
constexpr double VERIFY_VALUE_REL = 1e-5, VERIFY_VALUE_ABS = 1e-6;

CATTUS_HD inline bool verify_finite(float x) { return fabs((double)x) <= 3.4028234663852886e+38; }  // false for NaN

// |a - b| as a float: what a record carries.  inf where one operand is infinite (or the difference exceeds the float range), NaN where one
// is NaN or both are infinities of one sign.
CATTUS_HD inline float verify_dlogit(float a, float b) { return (float)fabs((double)a - (double)b); }

CATTUS_HD inline bool verify_logit_inside(float a, float b) {
    if (!verify_finite(a) || !verify_finite(b)) return false;
    return fabs((double)a - (double)b) <= VERIFY_POLICY_ATOL + VERIFY_POLICY_RTOL * fabs((double)b);
}

CATTUS_HD inline bool verify_value_inside(float a, float b) {
    if (!verify_finite(a) || !verify_finite(b)) return false;
    const double fa = fabs((double)a), fb = fabs((double)b), rel = VERIFY_VALUE_REL * (fa > fb ? fa : fb);
    return fabs((double)a - (double)b) <= (rel > VERIFY_VALUE_ABS ? rel : VERIFY_VALUE_ABS);
}

// One leaf's verdict, 16 bytes.  max_dlogit: the largest verify_dlogit over the leaf's moves, `move` the lowest index that holds it; a NaN
// difference takes no part in the maximum (its logit is outside all the same), and a leaf without a positive difference reports 0 at move 0.
// dvalue: verify_dlogit of the two values, a NaN as the one quiet NaN 0x7fc00000.
struct VerifyRecord {
    float max_dlogit;
    uint32_t move;
    float dvalue;
    uint32_t flags;
};
static_assert(sizeof(VerifyRecord) == 16, "a record is one 16-byte store");
constexpr uint32_t VERIFY_LEAF_OUTSIDE = 1, VERIFY_VALUE_OUTSIDE = 2;

// The running maximum of a leaf's moves: (d, i) replaces (best_d, best_i) when d is larger, or equal at a lower index -- the same result in
// whatever order the moves arrive, so a wave may split them among its lanes.  Starts at (0, 0xffffffff); verify_record() closes it.
CATTUS_HD inline void verify_take_max(float d, uint32_t i, float& best_d, uint32_t& best_i) {
    if (d > best_d || (d == best_d && i < best_i)) best_d = d, best_i = i;
}

CATTUS_HD inline float verify_dvalue(float a, float b) {
    const float d = verify_dlogit(a, b);
    if (d != d) {
        const uint32_t qnan = 0x7fc00000u;
        float f;
        memcpy(&f, &qnan, 4);
        return f;
    }
    return d;
}

CATTUS_HD inline VerifyRecord verify_record(float best_d, uint32_t best_i, bool any_logit_outside, float value_a, float value_b) {
    const bool v_out = !verify_value_inside(value_a, value_b);
    VerifyRecord r;
    r.max_dlogit = best_d;
    r.move = best_d > 0.0f ? best_i : 0u;
    r.dvalue = verify_dvalue(value_a, value_b);
    r.flags = (any_logit_outside || v_out ? VERIFY_LEAF_OUTSIDE : 0u) | (v_out ? VERIFY_VALUE_OUTSIDE : 0u);
    return r;
}

// The whole rule on one leaf in index order: what the kernel's wave computes in pieces.
inline VerifyRecord verify_leaf(const float* policy_a, const float* policy_b, uint32_t moves, float value_a, float value_b) {
    float best_d = 0.0f;
    uint32_t best_i = 0xffffffffu;
    bool outside = false;
    for (uint32_t m = 0; m < moves; m++) {
        verify_take_max(verify_dlogit(policy_a[m], policy_b[m]), m, best_d, best_i);
        outside = outside || !verify_logit_inside(policy_a[m], policy_b[m]);
    }
    return verify_record(best_d, best_i, outside, value_a, value_b);
}

}  // namespace cattus
