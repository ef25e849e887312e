// The ragged layout of the leaf server's legal-move lists (cattus_hip_submit_legal / wait_legal / apply_legal): the leaves of a batch keep
// their policy indices back to back in one array, idx [total], and one offset per leaf marks where its list starts, off [n + 1] with
// off[0] == 0 and off[n] == total; leaf i owns idx[off[i] .. off[i + 1]) and, at the same places, its probabilities.  A leaf without a
// list -- a plain cattus_hip_submit in a mixed batch, or a position without a legal move -- has an empty span.  Pure functions for the
// host and the device alike -- no HIP call, nothing of the evaluator -- so that every edge can be checked without a GPU
// (tests/test_legal_span.py) and the server's append, the kernel (kernels.hip, legal_softmax_ragged_kernel), the comparison
// (verify_priors_kernel with a row-offset table) and the evaluator's fold walk the same spans.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef CATTUS_HD
#ifdef __HIPCC__
#define CATTUS_HD __host__ __device__
#else
#define CATTUS_HD
#endif
#endif

#include <vector>

namespace cattus {

constexpr uint32_t LEGAL_CAP = 1024;  // the longest list a leaf may carry: the softmax kernels' LDS row

struct LegalSpan {
    uint32_t begin, count;
};
// Leaf `leaf` of an offset table off [n + 1], leaf < n.
CATTUS_HD inline LegalSpan legal_span(const uint32_t* off, uint32_t leaf) { return LegalSpan{off[leaf], off[leaf + 1] - off[leaf]}; }

// Why a list or a table is refused.
enum LegalFault { LEGAL_OK = 0, LEGAL_TOO_LONG = 1, LEGAL_BAD_INDEX = 2, LEGAL_BAD_OFFSETS = 3 };

// One leaf's list: at most LEGAL_CAP entries, every one a policy index < moves.  *at: the first offending position (LEGAL_BAD_INDEX).
CATTUS_HD inline LegalFault legal_list_check(const uint16_t* idx, uint32_t count, uint32_t moves, uint32_t* at) {
    if (count > LEGAL_CAP) return LEGAL_TOO_LONG;
    for (uint32_t k = 0; k < count; k++)
        if (idx[k] >= moves) {
            if (at) *at = k;
            return LEGAL_BAD_INDEX;
        }
    return LEGAL_OK;
}

// An offset table off [n + 1]: starts at 0, never descends, no span above LEGAL_CAP.  *at: the first offending leaf.
CATTUS_HD inline LegalFault legal_offsets_check(const uint32_t* off, uint32_t n, uint32_t* at) {
    if (off[0] != 0) {
        if (at) *at = 0;
        return LEGAL_BAD_OFFSETS;
    }
    for (uint32_t i = 0; i < n; i++)
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > LEGAL_CAP) {
            if (at) *at = i;
            return off[i + 1] < off[i] ? LEGAL_BAD_OFFSETS : LEGAL_TOO_LONG;
        }
    return LEGAL_OK;
}

// Which leaf owns element k of idx / probs, k < off[n]: the one leaf with off[leaf] <= k < off[leaf + 1] (empty spans own nothing),
// found by bisection on the table.
CATTUS_HD inline uint32_t legal_owner(const uint32_t* off, uint32_t n, uint32_t k) {
    uint32_t lo = 0, hi = n;  // off[lo] <= k < off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Host only.  A batch's table as the server grows it.  `off` holds one entry per leaf whose span is closed plus the running total; it stays empty
// until the batch's first list arrives, so that a batch of plain leaves keeps nothing.
// legal_close: the table for `leaves` leaves -- whoever came since the last list did so without one and gets an empty span.
inline void legal_close(std::vector<uint32_t>& off, uint32_t leaves) {
    if (off.empty()) off.push_back(0);
    const uint32_t total = off.back();
    off.resize((size_t)leaves + 1, total);
}
// legal_append: the leaf in slot `slot` (slots arrive in ascending order) brings `count` indices.
inline void legal_append(std::vector<uint16_t>& idx, std::vector<uint32_t>& off, uint32_t slot, const uint16_t* list, uint32_t count) {
    legal_close(off, slot);
    idx.insert(idx.end(), list, list + count);
    off.push_back((uint32_t)idx.size());
}

}  // namespace cattus
