"""The split-precision tower (dtype f16x2) against the float64 network at every scale of the residual stream.

An f16x2 epilogue splits an activation y unscaled into hi = f16(y), lo = f16(y - hi); once |y| < 2^-3 lo is an f16 subnormal and
y keeps an absolute resolution of 2^-25 instead of 22 significant bits.  The residual stream (the stem output, each block's
output) has the scale that the trained BatchNorm gamma / beta of the stem and the blocks' _bn2 give it, and the seeded networks
all put it at O(1).  Here each network runs as its stream twins (helpers.stream_twin: the same function with the stream x c, c a
power of two from 2^-7 to 2^8), each twin against its own forward_f64, on every f16x2 kernel the launch code can pick:

    direct_cb1    conv3x3_splitw_kernel, CB=1 tile (chess 2x256, 40 leaves: full_grid 40)
    direct_cb2    conv3x3_splitw_kernel, CB=2 tile (chess 2x256, 256 leaves, direct form: full_grid 256)
    direct_big    conv3x3_splitw_kernel on 128-slot boards (hex9 2x128, 100 leaves)
    wino_tower    tower_wino4_kernel, the Winograd tower in one launch (chess 2x128, 256 leaves)
    wino_layers   conv3x3_wino4_kernel, the same per layer (CATTUS_WINO_PERSIST=0)
    tower64s      tower64_split_kernel, the resident tower (hex7 6x64, 128 leaves)

(tile rule: test_f16_tower_gpu.py's docstring).  Bars per (kernel, c): (a) within F16X2_POLICY_ATOL_VS_F64 / F16X2_VALUE_ATOL_VS_F64
of the float64 twin on every sampled leaf; (b) at most SCALE_RATIO_MAX x the kernel's own error at c = 1 on the same leaves (the
sharp check: no growth as the stream shrinks); (c) nothing saturates; and the evaluator's stream shift (evaluator.hip,
choose_stream_shift) is the one the rule gives.  With the shift off (CATTUS_STREAM_SHIFT=0) c = 2^-7 must FAIL: the bar sees
what the shift is for.  The direct and resident kernels fail (a), 6-17x their error at c = 1; the Winograd kernels read f32 rows
and split only the transformed input, so they stay inside (a) and fail (b) (the value error grows 4.3x).  Controls on the same
networks and twins: dtype f32 bit-exact against the oracle on a few rows, dtype f16 (helpers.check_f16_against_f64) and bf16
(f32's exponent range: no shift) within their bounds, at every c.

Measured on an MI355X, max |dlogit| / max |dvalue| of f16x2 against float64 by c = 2^-7, 2^-5, 2^-3, 2^-1, 1, 2^4, 2^8:
    direct_cb1    7.0e-7 6.1e-7 6.5e-7 8.9e-7 6.1e-7 7.7e-7 7.9e-7 / 8.9e-8 7.7e-8 1.0e-7 7.3e-8 7.7e-8 1.1e-7 9.8e-8
    direct_cb2    7.2e-7 8.0e-7 6.3e-7 6.6e-7 8.0e-7 6.8e-7 7.2e-7 / 7.8e-8 9.9e-8 8.3e-8 1.0e-7 9.9e-8 6.7e-8 8.8e-8
    direct_big    3.7e-7 3.7e-7 3.8e-7 4.2e-7 3.7e-7 4.0e-7 4.0e-7 / 3.8e-8 4.4e-8 3.3e-8 4.5e-8 4.4e-8 4.9e-8 3.8e-8
    wino_*        6.0e-7 5.4e-7 6.1e-7 5.1e-7 5.5e-7 5.4e-7 5.4e-7 / 4.2e-8 4.4e-8 4.9e-8 5.4e-8 4.4e-8 4.7e-8 4.1e-8
    tower64s      4.6e-7 5.1e-7 5.2e-7 4.0e-7 5.1e-7 5.4e-7 4.8e-7 / 7.1e-8 7.2e-8 4.1e-8 6.2e-8 7.0e-8 7.2e-8 6.8e-8
and with the shift off, at c = 2^-7 and 2^-5 (from 2^-3 up the shift is 0 or the errors are those above):
    direct_cb1    5.1e-6 1.3e-6 / 8.1e-7 2.1e-7        direct_cb2    4.8e-6 1.4e-6 / 7.6e-7 2.3e-7
    direct_big    4.5e-6 1.1e-6 / 6.3e-7 1.7e-7        wino_*        9.3e-7 6.0e-7 / 1.9e-7 5.3e-8
    tower64s      8.1e-6 1.9e-6 / 1.2e-6 2.9e-7
"""

import math

import numpy as np
import pytest

from cattus_amd.evaluator import HipEvaluator
from cattus_amd.weights import CHESS, NetDesc, hex_game, pack_tensors, seeded_tensors
from oracle import oracle

from helpers import check_f16_against_f64, forward_f64, stream_twin
from test_f16_tower_gpu import random_planes
from test_hip_parity import F16X2_POLICY_ATOL_VS_F64, F16X2_VALUE_ATOL_VS_F64

pytestmark = pytest.mark.gpu

SCALES = [2.0**-7, 2.0**-5, 2.0**-3, 2.0**-1, 1.0, 2.0**4, 2.0**8]
SEED = 41
SAMPLE = 32  # leaves held to the float64 network on the larger batches (spread over the batch)

NETS = {
    # game preset, blocks, filters, head channels, plane words
    "chess2x256": (CHESS, 2, 256, 8, 1),
    "hex9_2x128": (hex_game(9), 2, 128, 4, 2),
    "chess2x128": (CHESS, 2, 128, 8, 1),
    "hex7_6x64": (hex_game(7), 6, 64, 16, 2),
}
CASES = [
    # id, network, leaves, tower_form, switches, the kernel that must run the tower
    ("direct_cb1", "chess2x256", 40, "direct", {}, "conv3x3_splitw_kernel"),
    ("direct_cb2", "chess2x256", 256, "direct", {}, "conv3x3_splitw_kernel"),
    ("direct_big", "hex9_2x128", 100, "direct", {}, "conv3x3_splitw_kernel"),
    ("wino_tower", "chess2x128", 256, "winograd", {}, "tower_wino4_kernel"),
    ("wino_layers", "chess2x128", 256, "winograd", {"CATTUS_WINO_PERSIST": "0"}, "conv3x3_wino4_kernel"),
    ("tower64s", "hex7_6x64", 128, "auto", {}, "tower64_split_kernel"),
]
# (b): an f16x2 error (max |dlogit|, max |dvalue|) at any c over the same kernel's at c = 1, per component: 2x the largest
# measured ratio, 1.46 / 1.40 (direct_cb1 at c = 2^-1 / 2^4; every other case <= 1.23)
SCALE_RATIO_MAX = (2.9, 2.8)
# the controls against forward_f64 on the same leaves, max |dlogit|, max |dvalue|: 2x the largest measured over every c.  Measured
# f16 | bf16 (the f16 errors move by < 2 % with c, bf16's by < 8 %):
#   chess2x256  3.87e-4 8.15e-5 | 4.85e-3 6.05e-4
#   hex9_2x128  3.61e-4 2.91e-5 | 3.41e-3 5.91e-4
#   chess2x128  3.62e-4 4.10e-5 | 3.99e-3 5.56e-4
#   hex7_6x64   5.11e-4 8.26e-5 | 3.89e-3 8.63e-4
F16_VS_F64 = {"chess2x256": (7.8e-4, 1.7e-4), "hex9_2x128": (7.3e-4, 5.9e-5), "chess2x128": (7.3e-4, 8.2e-5), "hex7_6x64": (1.03e-3, 1.66e-4)}
BF16_VS_F64 = {"chess2x256": (9.7e-3, 1.21e-3), "hex9_2x128": (6.9e-3, 1.19e-3), "chess2x128": (8.0e-3, 1.12e-3), "hex7_6x64": (7.8e-3, 1.73e-3)}


def desc_of(net: str) -> tuple[NetDesc, int]:
    game, blocks, filters, heads, words = NETS[net]
    return NetDesc(**game, blocks=blocks, filters=filters, vhc=heads, phc=heads), words


def sample(n: int) -> np.ndarray:
    return np.arange(n) if n <= 64 else np.linspace(0, n - 1, SAMPLE).round().astype(int)


def expected_stream_shift(d: NetDesc, t: dict) -> int:
    """choose_stream_shift (evaluator.hip) restated: S = median over channels of sqrt(gamma^2 + beta^2 summed over the stem
    BatchNorm and every block's _bn2); 0 for S >= 1/2, else -floor(log2 S), at most 16."""
    s = t["_conv1._bn.weight"].astype(np.float64) ** 2 + t["_conv1._bn.bias"].astype(np.float64) ** 2
    for i in range(d.blocks):
        p = f"_residual_blocks.{i}._bn2."
        s = s + t[p + "weight"].astype(np.float64) ** 2 + t[p + "bias"].astype(np.float64) ** 2
    S = math.sqrt(float(np.median(s)))
    return 0 if S >= 0.5 else min(16, -math.frexp(S)[1] + 1)


def err(out, ref):
    return float(np.abs(out[0] - ref[0]).max()), float(np.abs(out[1] - ref[1]).max())


def sweep(case, switches_extra=None, scales=SCALES):
    """One case over the scales: per c (c, stream shift, max |dlogit|, max |dvalue|, saturated), printed as it goes."""
    cid, net, n, form, switches, kernel = case
    d, words = desc_of(net)
    base = seeded_tensors(d, SEED)
    planes = random_planes(d, words, n, 5)
    idx = sample(n)
    rows = []
    for c in scales:
        tw = stream_twin(d, base, c)
        with HipEvaluator(pack_tensors(d, tw), batch_size=n, plane_words=words, dtype="f16x2", tower_form=form,
                          switches={**switches, **(switches_extra or {})}) as ev:
            assert ev.tower_kernel() == kernel, (cid, ev.tower_kernel())
            p, v = ev.eval(planes)
            shift, sat = ev.stream_shift(), ev.stats()["saturated"]
        assert np.isfinite(p).all() and np.isfinite(v).all(), (cid, c)
        ep, ev_ = err((p[idx], v[idx]), forward_f64(d, tw, planes[idx]))
        rows.append((c, shift, ep, ev_, sat))
        print("%s %s c=2^%d shift %d: f16x2 vs f64 max |dlogit| %.3g |dvalue| %.3g saturated %d"
              % (cid, switches_extra or "", round(math.log2(c)), shift, ep, ev_, sat))
    return rows


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_f16x2_holds_the_f64_bound_at_every_stream_scale(case):
    d, _ = desc_of(case[1])
    base = seeded_tensors(d, SEED)
    rows = sweep(case)
    one = next(r for r in rows if r[0] == 1.0)
    for c, shift, ep, ev_, sat in rows:
        assert shift == expected_stream_shift(d, stream_twin(d, base, c)), (c, shift)
        assert sat == 0, (c, sat)
        assert ep <= F16X2_POLICY_ATOL_VS_F64 and ev_ <= F16X2_VALUE_ATOL_VS_F64, (c, ep, ev_)
        assert ep <= SCALE_RATIO_MAX[0] * one[2] and ev_ <= SCALE_RATIO_MAX[1] * one[3], (c, ep / one[2], ev_ / one[3])
    assert rows[0][1] > 0  # the smallest stream was shifted
    # the bars see the problem: without the shift the smallest stream leaves (a), or in the Winograd form (b)
    ((c, shift, ep, ev_, sat),) = sweep(case, {"CATTUS_STREAM_SHIFT": "0"}, scales=[SCALES[0]])
    assert shift == 0 and sat == 0
    if case[3] == "winograd":
        assert ep > SCALE_RATIO_MAX[0] * one[2] or ev_ > SCALE_RATIO_MAX[1] * one[3], ("c = 2^-7 passes (b) without the shift", ep, ev_)
    else:
        assert ep > F16X2_POLICY_ATOL_VS_F64 or ev_ > F16X2_VALUE_ATOL_VS_F64, ("c = 2^-7 passes (a) without the shift", ep, ev_)


CONTROLS = [("chess2x256", 256), ("hex9_2x128", 100), ("chess2x128", 256), ("hex7_6x64", 128)]  # every network, at its largest batch


@pytest.mark.parametrize("net,n", CONTROLS, ids=[f"{a}_n{b}" for a, b in CONTROLS])
def test_f32_f16_bf16_controls_at_every_stream_scale(net, n):
    d, words = desc_of(net)
    base = seeded_tensors(d, SEED)
    planes = random_planes(d, words, n, 5)
    idx = sample(n)
    for c in SCALES:
        tw = stream_twin(d, base, c)
        blob = pack_tensors(d, tw)
        with HipEvaluator(blob, batch_size=4, plane_words=words, dtype="f32", switches={}) as ev:
            p, v = ev.eval(planes[:4])
        want_p, want_v = oracle.OracleNet(blob).forward(planes[:4])
        assert (p == want_p).all() and (v == want_v).all(), ("f32 is not bit-exact against the oracle", net, c)
        outs = {}
        for dtype in ("f16", "bf16"):
            with HipEvaluator(blob, batch_size=n, plane_words=words, dtype=dtype, switches={}) as ev:
                p, v = ev.eval(planes)
                assert ev.stats()["saturated"] == 0, (dtype, c)
                assert ev.stream_shift() == (expected_stream_shift(d, tw) if dtype == "f16" else 0)
            outs[dtype] = (p[idx], v[idx])
        ref = forward_f64(d, tw, planes[idx])
        label = "%s n=%d c=2^%d" % (net, n, round(math.log2(c)))
        check_f16_against_f64(label, F16_VS_F64[net], outs["f16"], outs["bf16"], ref)
        bp, bv = err(outs["bf16"], ref)
        assert bp <= BF16_VS_F64[net][0] and bv <= BF16_VS_F64[net][1], (label, bp, bv)
