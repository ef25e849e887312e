"""The f16 towers against the float64 network when the channels of the residual stream differ in scale.

test_split_range_gpu.py moves the whole stream by one factor; a trained network's channels differ.  An f16x2 epilogue keeps 22
significant bits of a stored activation only while it is above 2^-3 (below, its lo half is an f16 subnormal), and one stream shift
for the tower, chosen from the median channel, leaves every channel that runs far below the median on the wrong side of that.  So the
evaluator shifts per channel (evaluator.hip, choose_stream_shift; the rule: weight_layout.h, stream_shifts).  Here each network of
test_split_range_gpu.py runs as its channel twins (helpers.channel_twin: stream channel k x 2^e_k and its readers' weights
/ 2^e_k -- exact, the same function to the bit in float64 and in the f32 oracle), on every f16x2 kernel of that file's CASES:

    Q8   e_k = -8 where k % 4 == 1, else 0         a quarter of the channels small beside a unit median: global shift 0
    W8   e_k = default_rng(3).integers(-8, 9, F)   every scale from 2^-8 to 2^8: global shift 0
    M8   e_k = 0 where k % 4 == 1, else -8         a small median (global shift 8) with a quarter of the channels at 2^8 once shifted

Bars per (kernel, pattern), each twin against its own forward_f64 on the leaves test_split_range_gpu.py samples: (a) within
F16X2_POLICY_ATOL_VS_F64 / F16X2_VALUE_ATOL_VS_F64; (b) at most SCALE_RATIO_MAX x the same kernel's error on the base network on the
same leaves (the function is the same one: any growth is the kernel's); (c) nothing saturates; (d) the case's kernel ran; and the
shifts the evaluator reports (stream_shift, stream_shifts) are the ones the rule, restated here, gives.  With the shifts off
(CATTUS_STREAM_SHIFT=0) Q8 must FAIL -- (a) on the direct and resident kernels, (a) or (b) on the Winograd ones, as c = 2^-7 does in
test_split_range_gpu.py: the bars see what the per-channel shift is for.

Controls, per network at its largest batch: dtype f32 on every twin gives the base network's bits, and the oracle's on 4 rows;
dtype bf16 on every twin gives the base network's bf16 bits (bf16 rounding commutes with a power of two, a bf16 x bf16 product is
exact in f32, (w / c)(x c) = w x: the twin's f32 accumulator sees the same terms in the same order, and the epilogue's folded scale
and bias carry c exactly); dtype f16 stays within F16_VS_F64 and the relations of helpers.check_f16_against_f64.

helpers.hostile_tensors -- negative gammas, dead stream channels (gamma = beta = 0: the rule sees s_k = 0), all-zero folded conv1
rows (channel_shift(0)) -- is another network, held to its own forward_f64: f16x2 to (a), (c), (d) on every case, f32 to the
oracle's bits, f16 and bf16 to HOSTILE_F16_VS_F64 / HOSTILE_BF16_VS_F64 (measured here, as test_split_range_gpu.py's tables are).

Measured on an MI355X, max |dlogit| / max |dvalue| of f16x2 against float64, on the base network | Q8 W8 M8 | hostile:
    direct_cb1    6.1e-7 / 7.7e-8 | 7.3e-7 7.3e-7 8.5e-7 / 1.0e-7 1.1e-7 7.7e-8 | 8.5e-7 / 5.7e-8
    direct_cb2    8.0e-7 / 9.9e-8 | 6.2e-7 7.9e-7 6.2e-7 / 8.1e-8 9.9e-8 8.6e-8 | 6.7e-7 / 5.1e-8
    direct_big    3.7e-7 / 4.4e-8 | 3.9e-7 3.9e-7 4.6e-7 / 3.8e-8 5.0e-8 2.6e-8 | 3.8e-7 / 4.0e-8
    wino_*        5.5e-7 / 4.4e-8 | 6.1e-7 5.5e-7 5.1e-7 / 5.0e-8 5.1e-8 3.8e-8 | 6.1e-7 / 3.9e-8
    tower64s      5.1e-7 / 7.0e-8 | 5.1e-7 4.9e-7 5.5e-7 / 7.0e-8 6.7e-8 6.8e-8 | 4.9e-7 / 5.8e-8
(at most 1.38x / 1.39x the base network's), and with one shift for the whole tower -- the shifts off, which for Q8 and W8 (global
shift 0) is also what the global rule alone gave; M8, which it does shift, stays as above -- Q8 W8, and x the base network's:
    direct_cb1    4.5e-6 2.9e-6 / 9.7e-7 5.6e-7    7.3x 4.7x / 12.7x 7.4x
    direct_cb2    4.4e-6 3.1e-6 / 7.4e-7 5.6e-7    5.6x 3.9x /  7.5x 5.7x
    direct_big    3.7e-6 2.2e-6 / 6.8e-7 4.2e-7   10.1x 5.9x / 15.2x 9.5x
    wino_*        9.9e-7 6.8e-7 / 1.5e-7 9.1e-8    1.8x 1.3x /  3.3x 2.1x
    tower64s      6.4e-6 3.3e-6 / 1.9e-6 6.0e-7   12.5x 6.5x / 27.3x 8.6x
The direct and resident kernels leave (a) on both; the Winograd kernels, which split only the transformed input, stay inside (a)
and leave (b) on Q8 (their W8 growth, 2.1x, is inside it).  The controls: f32 and bf16 gave the base network's bits on every twin;
f16 moved by less than 1 % of its error.
"""

import math

import numpy as np
import pytest

from cattus_amd.evaluator import HipEvaluator
from cattus_amd.weights import NetDesc, pack_tensors, seeded_tensors
from oracle import oracle

from helpers import CHANNEL_PATTERNS, channel_twin, check_f16_against_f64, forward_f64, hostile_tensors
from test_f16_tower_gpu import random_planes
from test_hip_parity import F16X2_POLICY_ATOL_VS_F64, F16X2_VALUE_ATOL_VS_F64
from test_split_range_gpu import BF16_VS_F64, CASES, CONTROLS, F16_VS_F64, SCALE_RATIO_MAX, SEED, desc_of, err, expected_stream_shift, sample

pytestmark = pytest.mark.gpu

PATTERNS = ("Q8", "W8", "M8")
STREAM_SHIFT_MAX = 16
# the hostile networks' controls against their own forward_f64, max |dlogit|, max |dvalue|: 2x the measured.  Measured f16 | bf16:
#   chess2x256  3.45e-4 4.90e-5 | 4.01e-3 4.67e-4
#   hex9_2x128  3.46e-4 5.63e-5 | 4.03e-3 5.23e-4
#   chess2x128  3.75e-4 5.12e-5 | 4.04e-3 5.10e-4
#   hex7_6x64   4.51e-4 8.06e-5 | 3.93e-3 7.85e-4
HOSTILE_F16_VS_F64 = {"chess2x256": (7.0e-4, 9.9e-5), "hex9_2x128": (7.0e-4, 1.13e-4), "chess2x128": (7.5e-4, 1.03e-4), "hex7_6x64": (9.1e-4, 1.62e-4)}
HOSTILE_BF16_VS_F64 = {"chess2x256": (8.1e-3, 9.4e-4), "hex9_2x128": (8.1e-3, 1.05e-3), "chess2x128": (8.1e-3, 1.03e-3), "hex7_6x64": (7.9e-3, 1.58e-3)}


def expected_stream_shifts(d: NetDesc, t: dict) -> np.ndarray:
    """stream_shifts (weight_layout.h) restated: s_k = sqrt(gamma^2 + beta^2 of channel k summed over the stem BatchNorm and every
    block's _bn2), t the global shift (the median rule); t_k = t where s_k 2^t >= 1/2 or s_k is 0 or not finite, else
    -floor(log2 s_k) (the channel lifted into [1, 2)), at most 16."""
    s2 = t["_conv1._bn.weight"].astype(np.float64) ** 2 + t["_conv1._bn.bias"].astype(np.float64) ** 2
    for i in range(d.blocks):
        p = f"_residual_blocks.{i}._bn2."
        s2 = s2 + t[p + "weight"].astype(np.float64) ** 2 + t[p + "bias"].astype(np.float64) ** 2
    glob = expected_stream_shift(d, t)
    out = []
    for s in np.sqrt(s2):
        stays = not (s > 0 and math.isfinite(s)) or s * 2.0**glob >= 0.5
        out.append(glob if stays else min(STREAM_SHIFT_MAX, 1 - math.frexp(s)[1]))
    return np.array(out)


def run_f16x2(case, tensors, planes, switches_extra=None):
    """One f16x2 evaluator of the case on its planes: (policy, value) of the sampled leaves, global shift, per-channel shifts, saturated."""
    cid, net, n, form, switches, kernel = case
    d, words = desc_of(net)
    with HipEvaluator(pack_tensors(d, tensors), batch_size=n, plane_words=words, dtype="f16x2", tower_form=form,
                      switches={**switches, **(switches_extra or {})}) as ev:
        assert ev.tower_kernel() == kernel, (cid, ev.tower_kernel())  # (d)
        p, v = ev.eval(planes)
        shift, shifts, sat = ev.stream_shift(), ev.stream_shifts(), ev.stats()["saturated"]
    assert np.isfinite(p).all() and np.isfinite(v).all(), cid
    idx = sample(n)
    return (p[idx], v[idx]), shift, shifts, sat


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_f16x2_holds_the_f64_bound_when_stream_channels_differ_in_scale(case):
    cid, net, n = case[:3]
    d, words = desc_of(net)
    base = seeded_tensors(d, SEED)
    planes = random_planes(d, words, n, 5)
    idx = sample(n)
    out, shift, shifts, sat = run_f16x2(case, base, planes)
    one = err(out, forward_f64(d, base, planes[idx]))
    print("%s base: f16x2 vs f64 max |dlogit| %.3g |dvalue| %.3g" % (cid, *one))
    assert shift == 0 and not shifts.any() and sat == 0  # every seeded channel has s_k >= 0.75: nothing is shifted
    for pattern in PATTERNS:
        tw = channel_twin(d, base, CHANNEL_PATTERNS[pattern](d.filters))
        out, shift, shifts, sat = run_f16x2(case, tw, planes)
        ep, ev_ = err(out, forward_f64(d, tw, planes[idx]))
        print("%s %s shift %d, per channel %d..%d: f16x2 vs f64 max |dlogit| %.3g |dvalue| %.3g (%.2f / %.2f x base) saturated %d"
              % (cid, pattern, shift, shifts.min(), shifts.max(), ep, ev_, ep / one[0], ev_ / one[1], sat))
        want = expected_stream_shifts(d, tw)
        assert shift == expected_stream_shift(d, tw) and (shifts == want).all(), (pattern, shift, shifts, want)
        assert (shift >= 8 if pattern == "M8" else shift == 0) and shifts.min() == shift and shifts.max() >= 7, (pattern, shift, shifts)
        assert sat == 0, (pattern, sat)  # (c)
        assert ep <= F16X2_POLICY_ATOL_VS_F64 and ev_ <= F16X2_VALUE_ATOL_VS_F64, (pattern, ep, ev_)  # (a)
        assert ep <= SCALE_RATIO_MAX[0] * one[0] and ev_ <= SCALE_RATIO_MAX[1] * one[1], (pattern, ep / one[0], ev_ / one[1])  # (b)
    # the bars see the problem: without the shifts Q8 leaves (a), or in the Winograd form (b)
    tw = channel_twin(d, base, CHANNEL_PATTERNS["Q8"](d.filters))
    out, shift, shifts, sat = run_f16x2(case, tw, planes, {"CATTUS_STREAM_SHIFT": "0"})
    ep, ev_ = err(out, forward_f64(d, tw, planes[idx]))
    print("%s Q8 shifts off: f16x2 vs f64 max |dlogit| %.3g |dvalue| %.3g (%.2f / %.2f x base)" % (cid, ep, ev_, ep / one[0], ev_ / one[1]))
    assert shift == 0 and not shifts.any() and sat == 0
    if case[3] == "winograd":
        assert (ep > F16X2_POLICY_ATOL_VS_F64 or ev_ > F16X2_VALUE_ATOL_VS_F64
                or ep > SCALE_RATIO_MAX[0] * one[0] or ev_ > SCALE_RATIO_MAX[1] * one[1]), ("Q8 passes (a) and (b) without the shifts", ep, ev_)
    else:
        assert ep > F16X2_POLICY_ATOL_VS_F64 or ev_ > F16X2_VALUE_ATOL_VS_F64, ("Q8 passes (a) without the shifts", ep, ev_)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_f16x2_holds_the_f64_bound_on_the_hostile_network(case):
    cid, net, n = case[:3]
    d, words = desc_of(net)
    h = hostile_tensors(d, seeded_tensors(d, SEED))
    planes = random_planes(d, words, n, 5)
    out, shift, shifts, sat = run_f16x2(case, h, planes)
    ep, ev_ = err(out, forward_f64(d, h, planes[sample(n)]))
    print("%s hostile shift %d, per channel %d..%d: f16x2 vs f64 max |dlogit| %.3g |dvalue| %.3g saturated %d"
          % (cid, shift, shifts.min(), shifts.max(), ep, ev_, sat))
    assert shift == expected_stream_shift(d, h) and (shifts == expected_stream_shifts(d, h)).all(), (shift, shifts)
    assert (shifts[5::16] == shift).all()  # a dead channel gets no shift of its own
    assert sat == 0, sat
    assert ep <= F16X2_POLICY_ATOL_VS_F64 and ev_ <= F16X2_VALUE_ATOL_VS_F64, (ep, ev_)


def run_dtype(d, words, blob, planes, dtype, n):
    with HipEvaluator(blob, batch_size=n, plane_words=words, dtype=dtype, switches={}) as ev:
        p, v = ev.eval(planes[:n])
        assert ev.stats()["saturated"] == 0, dtype
        shift, shifts = ev.stream_shift(), ev.stream_shifts()
    return p, v, shift, shifts


@pytest.mark.parametrize("net,n", CONTROLS, ids=[f"{a}_n{b}" for a, b in CONTROLS])
def test_f32_f16_bf16_controls_when_stream_channels_differ_in_scale(net, n):
    d, words = desc_of(net)
    base = seeded_tensors(d, SEED)
    planes = random_planes(d, words, n, 5)
    idx = sample(n)
    ref = forward_f64(d, base, planes[idx])  # every twin's float64 run is this one to the bit (test_f64_reference.py)
    blob = pack_tensors(d, base)
    want32 = run_dtype(d, words, blob, planes, "f32", n)[:2]
    want_bf = run_dtype(d, words, blob, planes, "bf16", n)[:2]
    for pattern in PATTERNS:
        tw = channel_twin(d, base, CHANNEL_PATTERNS[pattern](d.filters))
        blob = pack_tensors(d, tw)
        p, v, shift, shifts = run_dtype(d, words, blob, planes, "f32", n)
        assert shift == 0 and not shifts.any()
        assert p.tobytes() == want32[0].tobytes() and v.tobytes() == want32[1].tobytes(), ("f32 on the twin is not the base network's bits", net, pattern)
        want_p, want_v = oracle.OracleNet(blob).forward(planes[:4])
        assert (p[:4] == want_p).all() and (v[:4] == want_v).all(), ("f32 is not bit-exact against the oracle", net, pattern)
        bp, bv, shift, shifts = run_dtype(d, words, blob, planes, "bf16", n)
        assert shift == 0 and not shifts.any()
        assert bp.tobytes() == want_bf[0].tobytes() and bv.tobytes() == want_bf[1].tobytes(), ("bf16 on the twin is not the base network's bits", net, pattern)
        hp, hv, shift, shifts = run_dtype(d, words, blob, planes, "f16", n)
        assert shift == expected_stream_shift(d, tw) and (shifts == expected_stream_shifts(d, tw)).all(), (pattern, shift, shifts)
        check_f16_against_f64("%s n=%d %s" % (net, n, pattern), F16_VS_F64[net], (hp[idx], hv[idx]), (bp[idx], bv[idx]), ref)
        eb = err((bp[idx], bv[idx]), ref)
        assert eb[0] <= BF16_VS_F64[net][0] and eb[1] <= BF16_VS_F64[net][1], (net, pattern, eb)


@pytest.mark.parametrize("net,n", CONTROLS, ids=[f"{a}_n{b}" for a, b in CONTROLS])
def test_f32_f16_bf16_controls_on_the_hostile_network(net, n):
    d, words = desc_of(net)
    h = hostile_tensors(d, seeded_tensors(d, SEED))
    planes = random_planes(d, words, n, 5)
    idx = sample(n)
    ref = forward_f64(d, h, planes[idx])
    blob = pack_tensors(d, h)
    p, v, _, _ = run_dtype(d, words, blob, planes, "f32", 4)
    want_p, want_v = oracle.OracleNet(blob).forward(planes[:4])
    assert (p == want_p).all() and (v == want_v).all(), ("f32 is not bit-exact against the oracle", net)
    bp, bv, shift, shifts = run_dtype(d, words, blob, planes, "bf16", n)
    assert shift == 0 and not shifts.any()
    hp, hv, shift, shifts = run_dtype(d, words, blob, planes, "f16", n)
    assert shift == expected_stream_shift(d, h) and (shifts == expected_stream_shifts(d, h)).all(), (shift, shifts)
    check_f16_against_f64("%s n=%d hostile" % (net, n), HOSTILE_F16_VS_F64[net], (hp[idx], hv[idx]), (bp[idx], bv[idx]), ref)
    eb = err((bp[idx], bv[idx]), ref)
    assert eb[0] <= HOSTILE_BF16_VS_F64[net][0] and eb[1] <= HOSTILE_BF16_VS_F64[net][1], (net, eb)
