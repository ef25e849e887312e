// Where a weight lives in the fragment-ordered buffers of the f16x2 kernels (kernels.h): shared by the host code that writes them
// (weight_layout.h) and the kernels' interface.  Plain C++, no HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cattus {

// CONV_W_FRAG: element index of weight (tap t, output channel co, input channel ci, part 0 = hi / 1 = lo)
inline size_t split_frag_index(uint32_t t, uint32_t co, uint32_t ci, uint32_t part, uint32_t cin_pad) {
    const uint32_t nst = cin_pad / 32 * 18, ch = ci >> 5, k = (ci >> 4) & 1, h = (ci >> 3) & 1, e = ci & 7;
    const uint32_t stage = ((ch * 3 + t / 3) * 3 + t % 3) * 2 + k, lane = h * 32 + (co & 31);
    return ((((size_t)(co >> 5) * nst + stage) * 2 + part) * 64 + lane) * 8 + e;
}
// K1w / K1w4: element index of U (frequency f, output channel co, input channel ci, part); the kernels' weight ring reads
// WINO_RING_STAGES stages (of 2,048 B) past a cout block's end: wu is allocated with that much behind it
constexpr int WINO_RING_STAGES = 8;
inline size_t wino_frag_index(uint32_t f, uint32_t co, uint32_t ci, uint32_t part, uint32_t cin_pad) {
    const uint32_t nst = cin_pad / 16 * 16, stage = (ci >> 4) * 16 + f, lane = ((ci >> 3) & 1) * 32 + (co & 31);
    return ((((size_t)(co >> 5) * nst + stage) * 2 + part) * 64 + lane) * 8 + (ci & 7);
}
// K1wh (dtype f16w): element index of the single f16 U (frequency f, output channel co, input channel ci): K1w's order without the lo
// part -- [cout / 32][k-step x 16 + f][lane][8 f16], 1 KiB per stage; the kernel reads nothing past a cout block's last stage
inline size_t wino_f16_frag_index(uint32_t f, uint32_t co, uint32_t ci, uint32_t cin_pad) {
    const uint32_t nst = cin_pad / 16 * 16, stage = (ci >> 4) * 16 + f, lane = ((ci >> 3) & 1) * 32 + (co & 31);
    return (((size_t)(co >> 5) * nst + stage) * 64 + lane) * 8 + (ci & 7);
}
inline size_t wino_f16_u_elems(uint32_t cout_pad, uint32_t cin_pad) { return (size_t)16 * cout_pad * cin_pad; }
// K1wf (dtype f32w): element index of the f32 U (frequency f, output channel co, input channel ci):
// [cout / 32][8-channel group x 16 + f][lane][4 f32], 1 KiB per stage, lane = (ci / 4 % 2) * 32 + co % 32 -- the operand piece
// Mfma<float>::mac takes (device_common.h); the kernel reads nothing past a cout block's last stage: no ring tail
inline size_t wino_f32_frag_index(uint32_t f, uint32_t co, uint32_t ci, uint32_t cin_pad) {
    const uint32_t nst = cin_pad / 8 * 16, stage = (ci >> 3) * 16 + f, lane = ((ci >> 2) & 1) * 32 + (co & 31);
    return (((size_t)(co >> 5) * nst + stage) * 64 + lane) * 4 + (ci & 3);
}
inline size_t wino_f32_u_elems(uint32_t cout_pad, uint32_t cin_pad) { return (size_t)16 * cout_pad * cin_pad; }

}  // namespace cattus
