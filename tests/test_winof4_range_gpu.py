"""The Winograd F(4x4, 3x3) form of the f16x2 tower (tower_form="winograd_f4", conv3x3_winof4_kernel) against the float64 network
across the scales of the residual stream: the form with the least range -- activations capped at WINOF4_ACT_MAX = 655 where the F(2x2)
form caps at 16,376 and the direct form at 65,504 -- on the range machinery of test_split_range_gpu.py (stream twins),
test_channel_scale_gpu.py (channel twins, the hostile network) and test_stream_calibration_gpu.py (calibrated shifts), none of which
runs this kernel.

Cases, the smallest at which the kernel takes each path (test_winof4_gpu.py has the reasoning):
    f4_groups   chess 2x128, max_batch 80, 77 leaves: ten board groups, the last leaves short of the padding, 4 cout blocks, 8 k-steps
    f4_half     chess 2x256, max_batch 12, 12 leaves: a half group at the end, 8 cout blocks, 16 k-steps
(two blocks: both HAS_RES instances run).  Every leaf of f4_half and 32 of f4_groups' 77 (test_split_range_gpu.sample) are held to
forward_f64; every run asserts the kernel's name.

Bars.  F16X2_*_ATOL_VS_F64 (1.5e-6) is not applied: it straddles this form's honest error.
    (a0) the base network: error against forward_f64 <= 3x the CPU emulation's (scripts/winograd_gate_f4.py run(), computed here on the
         same blob and leaves; 3x is test_winof4_gpu.py's margin), and inside the reference's tolerance against the float64 outputs
    (b)  every in-range twin: error <= SCALE_RATIO_MAX x this kernel's own error on the base network on the same leaves (the function is
         the same one: any growth is the kernel's), and inside the reference's tolerance against its own forward_f64
    (c)  saturated == 0 on every in-range twin
    (d)  the shifts the evaluator reports are the rule's, restated in Python: test_channel_scale_gpu.expected_stream_shifts, then the
         ceiling this form alone puts on the estimate (weight_layout.h WINOF4_STREAM_CEILING = 2; test_winof4_rule.guarded_shifts):
         while t_k > 0 and s_k 2^t_k >= 2, t_k drops by one
No "must fail with the shift off" assertion: this form reads f32 rows and splits only its transformed input, the unshifted c = 2^-7 twin
grows 1.7x in the emulation, and such an assertion would not discriminate.  c = 2^8 does.

Why the ceiling.  The estimate rule lifts channels below the median and never held back one far above it.  Under M8 (the median channel
at 2^-8, a quarter of the channels at 1) it gave t = t_k = 8 everywhere; the float64 stream x 2^t_k then reaches 864 (2x128) and 986
(2x256), 4 and 7 channels above 655: the stem and the kernel's epilogue clamp them and the logits are wrong.  Observed with the library of
this file's parent commit, on an MI355X (test_channel_twins_and_the_hostile_network, M8; red on both cases): shifts 8..8, saturated 109
(f4_groups) and 65 (f4_half) -- (c) fails -- at 9.62e-3 / 1.23e-3 and 1.16e-2 / 2.36e-3 against float64, 17160x / 17344x and 14514x /
28131x the base network's -- (b) fails; with the ceiling the unit channels run at t_k 0 or 1 and M8 gives Q8's bits.

Tests: 1. the stream sweep c = 2^-7 .. 2^6 (before any GPU run: the float64 stream x 2^t_k stays <= 655 / 2); 2. past the cap, c = 2^8
(float64 first: >= 1.5 x 655): finite outputs, saturated > 0, doubled by a second eval of the same batch, bar (b) failed -- the bars and
the counter see a capped tower; 3. the channel twins Q8 and M8 and the hostile network (held to 3x its own emulation), and W8, whose
e_k = +8 channels are past the cap by construction (a stream is never shifted down): test 2's assertions; 4. the calibrated path on M8 and
on the hidden twin of Q8: calibrated_shifts_restated with the headroom 163.75 (WINOF4_CAL_HEADROOM), which no GPU test exercised; 5. a
leaf's bits under M8 do not depend on its slot.

Measured on an MI355X (profiles/winof4_range.txt has the table with the emulation's figures beside it):
max |dlogit| / max |dvalue| against float64 (x the base network's), global shift, t_k, saturated; f4_groups | f4_half:
    base      5.61e-7 / 7.10e-8, emulation 5.87e-7 / 1.15e-7                  | 7.98e-7 / 8.38e-8, emulation 6.55e-7 / 9.62e-8
    c=2^-7    6.78e-7 / 1.15e-7 (1.21 / 1.62)  t 7, 7..7   0                  | 7.82e-7 / 5.12e-8 (0.98 / 0.61)  t 7, 7..7   0
    c=2^-5    5.66e-7 / 7.18e-8 (1.01 / 1.01)  t 5, 5..5   0                  | 7.94e-7 / 8.31e-8 (0.99 / 0.99)  t 5, 5..5   0
    c=2^-3    5.22e-7 / 7.70e-8 (0.93 / 1.08)  t 3, 3..3   0                  | 8.37e-7 / 1.00e-7 (1.05 / 1.20)  t 3, 3..3   0
    c=2^-1    5.86e-7 / 8.16e-8 (1.05 / 1.15)  t 0, 0..2   0                  | 7.71e-7 / 1.00e-7 (0.97 / 1.20)  t 0, 0..2   0
    c=1       5.61e-7 / 7.10e-8 (1.00 / 1.00)  t 0, 0..0   0                  | 7.98e-7 / 8.38e-8 (1.00 / 1.00)  t 0, 0..0   0
    c=2^4     5.53e-7 / 8.72e-8 (0.99 / 1.23)  t 0, 0..0   0                  | 7.20e-7 / 1.08e-7 (0.90 / 1.28)  t 0, 0..0   0
    c=2^6     5.55e-7 / 8.85e-8 (0.99 / 1.25)  t 0, 0..0   0                  | 7.21e-7 / 1.07e-7 (0.90 / 1.28)  t 0, 0..0   0
    c=2^8     3.07e-2 / 4.26e-3 (54715 / 59924) t 0        1463, then 2926    | 3.10e-2 / 4.87e-3 (38879 / 58059) t 0        439, then 878
    Q8        5.28e-7 / 6.94e-8 (0.94 / 0.98)  t 0, 0..9   0                  | 7.17e-7 / 1.08e-7 (0.90 / 1.29)  t 0, 0..9   0
    M8        5.28e-7 / 6.94e-8 (0.94 / 0.98)  t 8, 0..8   0                  | 7.17e-7 / 1.08e-7 (0.90 / 1.29)  t 8, 0..8   0
    hostile   7.82e-7 / 6.86e-8, emulation 6.37e-7 / 1.23e-7            0     | 8.41e-7 / 9.69e-8, emulation 5.60e-7 / 9.69e-8            0
    W8        2.29e-2 / 2.40e-3 (40799 / 33772) t 0, 0..8  420, then 840      | 2.03e-2 / 9.43e-4 (25425 / 11257) t 0, 0..8  47, then 94
    M8 calibrated         5.49e-7 / 1.09e-7 (0.98 / 1.53)  t 10, 5..12  0     | 9.11e-7 / 8.57e-8 (1.14 / 1.02)  t 10, 5..12  0
    hidden Q8 calibrated  5.50e-7 / 1.06e-7 (0.98 / 1.50)  t 2, 2..12   0     | 7.58e-7 / 9.81e-8 (0.95 / 1.17)  t 2, 2..12   0
The device sits at 0.96 - 1.50x the emulation's logit error and 0.56 - 1.00x its value error (bar 3x); past the cap the emulation gives the
device's figures to three digits (3.07e-2 / 4.26e-3, 2.29e-2 / 2.40e-3 | 3.10e-2 / 4.87e-3, 2.03e-2 / 9.43e-4): that error is the clamp's.
"""

import importlib.util
import math
import sys
from pathlib import Path

import numpy as np
import pytest

from cattus_amd.evaluator import HipEvaluator
from cattus_amd.weights import pack_tensors, seeded_tensors

from helpers import CHANNEL_PATTERNS, channel_twin, forward_f64, hostile_tensors, outputs_equal_ref_tol, stream_twin
from test_channel_scale_gpu import expected_stream_shifts
from test_f16_tower_gpu import random_planes
from test_split_range_gpu import SCALE_RATIO_MAX, SEED, desc_of, err, expected_stream_shift, sample
from test_stream_calibration import calibrated_shifts_restated, hidden_twin
from test_stream_calibration_gpu import stream_range_f64
from test_winof4_rule import CEILING, guarded_shifts

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KERNEL = "conv3x3_winof4_kernel"
ACT_MAX = 655.0  # WINOF4_ACT_MAX (winof4_rule.h derives it; tests/winof4_rule_check.cpp checks the derivation)
CAL_HEADROOM = ACT_MAX / 4  # WINOF4_CAL_HEADROOM, 163.75
EMULATION_MARGIN = 3.0  # test_winof4_gpu.py's: the device sat at 0.58 - 0.96 of the emulation on the reference-made fixtures

CASES = [
    # id, network (test_split_range_gpu.NETS), max_batch, leaves
    ("f4_groups", "chess2x128", 80, 77),
    ("f4_half", "chess2x256", 12, 12),
]
IDS = [c[0] for c in CASES]
SWEEP = [2.0**-7, 2.0**-5, 2.0**-3, 2.0**-1, 1.0, 2.0**4, 2.0**6]
PAST_THE_CAP = 2.0**8


def _gate():
    """scripts/winograd_gate_f4.py, loaded as tests/test_winof4_gate.py loads it"""
    if "winograd_gate_f4" in sys.modules:
        return sys.modules["winograd_gate_f4"]
    spec = importlib.util.spec_from_file_location("winograd_gate_f4", ROOT / "scripts" / "winograd_gate_f4.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules["winograd_gate_f4"] = mod
    spec.loader.exec_module(mod)
    return mod


def emulated(name, d, tensors, planes):
    """The CPU emulation of the kernel's arithmetic on these leaves: (max |dlogit|, max |dvalue|) against float64, activations capped."""
    out = _gate().run(name, pack_tensors(d, tensors), planes)["winograd_f4_split"]
    return (out["dp_vs_f64"], out["dv_vs_f64"]), out["activations_capped"]


def expected_f4_shifts(d, t):
    """(d): (global shift, t_k) as the F(4x4) tower chooses them on the estimate path.  s_k as expected_stream_shifts has it; the
    unguarded rule of guarded_shifts must be that function's, the global shift expected_stream_shift's."""
    s2 = t["_conv1._bn.weight"].astype(np.float64) ** 2 + t["_conv1._bn.bias"].astype(np.float64) ** 2
    for i in range(d.blocks):
        p = f"_residual_blocks.{i}._bn2."
        s2 = s2 + t[p + "weight"].astype(np.float64) ** 2 + t[p + "bias"].astype(np.float64) ** 2
    glob, plain, held = guarded_shifts([float(x) for x in s2], CEILING)
    assert glob == expected_stream_shift(d, t) and plain == list(expected_stream_shifts(d, t))
    return glob, np.array(held)


def shifted_abs_max(d, tensors, planes, shifts):
    """The float64 network's stream as the tower carries it: max over channels of abs_max_k 2^t_k, and how many channels pass the cap."""
    carried = stream_range_f64(d, tensors, planes)[1] * np.exp2(np.asarray(shifts, dtype=np.float64))
    return float(carried.max()), int((carried > ACT_MAX).sum())


def run_f4(case, tensors, planes, calibration=None, again=False):
    """One F(4x4) evaluator of the case on its planes: (policy, value) of the sampled leaves, global shift, per-channel shifts, saturated
    -- after a second eval of the same batch as well where `again`."""
    cid, net, max_batch, n = case
    d, words = desc_of(net)
    assert len(planes) == n
    with HipEvaluator(pack_tensors(d, tensors), max_batch, words, dtype="f16x2", tower_form="winograd_f4", switches={}, calibration=calibration) as ev:
        assert ev.tower_kernel() == KERNEL, (cid, ev.tower_kernel())
        p, v = ev.eval(planes)
        shift, shifts, sat = ev.stream_shift(), ev.stream_shifts(), ev.stats()["saturated"]
        if again:
            ev.eval(planes)
            sat = (sat, ev.stats()["saturated"])
    assert np.isfinite(p).all() and np.isfinite(v).all(), cid
    idx = sample(n)
    return (p[idx], v[idx]), shift, shifts, sat


_shared = {}


def setup_of(case):
    """Per case, once: the base tensors, the planes, the sampled leaves, and the kernel's own error on the base network on those leaves
    (bar (b)'s yardstick) with the float64 outputs it was taken against -- shared between the tests and left as they are."""
    cid, net, max_batch, n = case
    if cid not in _shared:
        d, words = desc_of(net)
        base = seeded_tensors(d, SEED)
        planes = random_planes(d, words, n, 5)
        idx = sample(n)
        ref = forward_f64(d, base, planes[idx])
        out, shift, shifts, sat = run_f4(case, base, planes)
        assert shift == 0 and not shifts.any() and sat == 0  # every seeded channel has s_k >= 0.75: nothing is shifted, the guard cannot act
        _shared[cid] = dict(d=d, base=base, planes=planes, idx=idx, ref=ref, out=out, one=err(out, ref))
    return _shared[cid]


def report(cid, what, shift, shifts, e, one, sat, emu=None):
    print("winof4_range %-9s %-12s shift %2d per channel %2d..%2d: max |dlogit| %.3g |dvalue| %.3g (%.2f / %.2f x base) saturated %s%s"
          % (cid, what, shift, shifts.min(), shifts.max(), e[0], e[1], e[0] / one[0], e[1] / one[1], sat,
             "" if emu is None else "; emulation %.3g / %.3g" % emu))


def check_in_range(cid, what, out, ref, one, sat):
    """bars (b) and (c)"""
    e = err(out, ref)
    assert sat == 0, (cid, what, sat)  # (c)
    assert e[0] <= SCALE_RATIO_MAX[0] * one[0] and e[1] <= SCALE_RATIO_MAX[1] * one[1], (cid, what, e[0] / one[0], e[1] / one[1])  # (b)
    assert outputs_equal_ref_tol(out[0], out[1], ref[0], ref[1]), (cid, what)


def check_past_the_cap(cid, what, out, ref, one, sat):
    """what a capped tower must look like from outside (run_f4 has asserted finite outputs): counted, per eval, and outside bar (b)"""
    first, second = sat
    e = err(out, ref)
    assert first > 0 and second == 2 * first, (cid, what, sat)
    assert e[0] > SCALE_RATIO_MAX[0] * one[0] or e[1] > SCALE_RATIO_MAX[1] * one[1], ("a capped tower passes (b)", cid, what, e, one)


# ---- 1. the stream sweep ----
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_form_holds_float64_at_every_stream_scale_inside_its_range(case):
    cid = case[0]
    s = setup_of(case)
    d, base, planes, idx, one = s["d"], s["base"], s["planes"], s["idx"], s["one"]
    # the reference alone keeps the inputs in range: nothing below depends on the kernel for that
    twins = []
    for c in SWEEP:
        tw = stream_twin(d, base, c)
        glob, want = expected_f4_shifts(d, tw)
        top, over = shifted_abs_max(d, tw, planes, want)
        print("winof4_range %-9s c=2^%-3d float64 stream x 2^t_k: abs max %.3g" % (cid, round(math.log2(c)), top))
        assert top <= ACT_MAX / 2 and over == 0, (c, top)
        twins.append((c, tw, glob, want))
    # (a0)
    emu, capped = emulated(cid, d, base, planes[idx])
    report(cid, "base", 0, np.zeros(1, dtype=int), one, one, 0, emu)
    assert capped == 0
    assert one[0] <= EMULATION_MARGIN * emu[0] and one[1] <= EMULATION_MARGIN * emu[1], (one, emu)
    assert outputs_equal_ref_tol(s["out"][0], s["out"][1], s["ref"][0], s["ref"][1])
    for c, tw, glob, want in twins:
        what = "c=2^%d" % round(math.log2(c))
        out, shift, shifts, sat = run_f4(case, tw, planes)
        ref = forward_f64(d, tw, planes[idx])
        report(cid, what, shift, shifts, err(out, ref), one, sat)
        assert shift == glob and (shifts == want).all(), (c, shift, shifts, want)  # (d)
        check_in_range(cid, what, out, ref, one, sat)
    assert twins[0][2] >= 6 and twins[-1][2] == 0  # the smallest stream was shifted, the largest was not


# ---- 2. past the cap ----
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_stream_past_the_cap_is_counted_and_leaves_the_bars(case):
    cid = case[0]
    s = setup_of(case)
    d, planes, idx = s["d"], s["planes"], s["idx"]
    tw = stream_twin(d, s["base"], PAST_THE_CAP)
    glob, want = expected_f4_shifts(d, tw)
    top, over = shifted_abs_max(d, tw, planes, want)
    print("winof4_range %-9s c=2^8   float64 stream x 2^t_k: abs max %.3g, %d channels past the cap" % (cid, top, over))
    assert glob == 0 and not want.any() and top >= 1.5 * ACT_MAX, top
    out, shift, shifts, sat = run_f4(case, tw, planes, again=True)
    ref = forward_f64(d, tw, planes[idx])
    report(cid, "c=2^8", shift, shifts, err(out, ref), s["one"], sat)
    assert shift == 0 and not shifts.any()
    check_past_the_cap(cid, "c=2^8", out, ref, s["one"], sat)


# ---- 3. channel twins and the hostile network ----
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_channel_twins_and_the_hostile_network(case):
    """M8 is the defect the ceiling answers.  With the parent commit's library this test is red on both cases: t_k = 8 on every channel,
    saturated 109 (f4_groups) / 65 (f4_half), the error 17160x / 14514x the base network's -- (d), (c) and (b) fail; Q8 passes there."""
    cid = case[0]
    s = setup_of(case)
    d, base, planes, idx, one = s["d"], s["base"], s["planes"], s["idx"], s["one"]
    for pattern in ("Q8", "M8"):
        tw = channel_twin(d, base, CHANNEL_PATTERNS[pattern](d.filters))
        glob, want = expected_f4_shifts(d, tw)
        top, over = shifted_abs_max(d, tw, planes, want)
        assert top <= CAL_HEADROOM and over == 0, (pattern, top)  # the guarded twin is in range by the reference alone
        out, shift, shifts, sat = run_f4(case, tw, planes)
        report(cid, pattern, shift, shifts, err(out, s["ref"]), one, sat)  # a channel twin's float64 run is the base network's to the bit
        assert shift == glob and (shifts == want).all(), (pattern, shift, shifts, want)  # (d)
        if pattern == "M8":  # a small median, and the unit channels held back below it
            assert shift >= 8 and (shifts[1::4] <= 1).all() and (np.delete(shifts, np.s_[1::4]) == shift).all(), (shift, shifts)
        else:
            assert shift == 0 and (shifts[1::4] >= 7).all() and not np.delete(shifts, np.s_[1::4]).any(), (shift, shifts)
        check_in_range(cid, pattern, out, forward_f64(d, tw, planes[idx]), one, sat)
    # the hostile network: another function, held to its own emulation
    h = hostile_tensors(d, base)
    glob, want = expected_f4_shifts(d, h)
    out, shift, shifts, sat = run_f4(case, h, planes)
    ref = forward_f64(d, h, planes[idx])
    emu, capped = emulated(cid + "_hostile", d, h, planes[idx])
    e = err(out, ref)
    report(cid, "hostile", shift, shifts, e, one, sat, emu)
    assert shift == glob and (shifts == want).all() and (shifts[5::16] == shift).all(), (shift, shifts)  # a dead channel gets no shift of its own
    assert sat == 0 and capped == 0
    assert e[0] <= EMULATION_MARGIN * emu[0] and e[1] <= EMULATION_MARGIN * emu[1], (e, emu)
    assert outputs_equal_ref_tol(out[0], out[1], ref[0], ref[1])
    # W8: its e_k = +8 channels are unshifted and a stream is never shifted down -- past the cap by construction
    tw = channel_twin(d, base, CHANNEL_PATTERNS["W8"](d.filters))
    glob, want = expected_f4_shifts(d, tw)
    top, over = shifted_abs_max(d, tw, planes, want)
    print("winof4_range %-9s W8      float64 stream x 2^t_k: abs max %.3g, %d channels past the cap" % (cid, top, over))
    assert top > ACT_MAX, top
    out, shift, shifts, sat = run_f4(case, tw, planes, again=True)
    report(cid, "W8", shift, shifts, err(out, s["ref"]), one, sat)
    assert shift == glob == 0 and (shifts == want).all()
    check_past_the_cap(cid, "W8", out, forward_f64(d, tw, planes[idx]), one, sat)


# ---- 4. the calibrated path ----
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_calibrated_shifts_keep_the_forms_headroom(case):
    cid, net, max_batch, n = case
    s = setup_of(case)
    d, base, planes, idx, one = s["d"], s["base"], s["planes"], s["idx"], s["one"]
    words = desc_of(net)[1]
    twins = (("M8 cal", channel_twin(d, base, CHANNEL_PATTERNS["M8"](d.filters))), ("hidden Q8", hidden_twin(d, base, CHANNEL_PATTERNS["Q8"](d.filters))))
    for what, tw in twins:
        # what cattus_hip_create_calibrated measures: stream_range of an f32 evaluator of the same blob on the same planes
        with HipEvaluator(pack_tensors(d, tw), batch_size=min(n, 256), plane_words=words, dtype="f32", switches={}) as ev:
            rms, mx = ev.stream_range(planes)
        want_shift, want = calibrated_shifts_restated(rms, mx, CAL_HEADROOM)
        out, shift, shifts, sat = run_f4(case, tw, planes, calibration=planes)
        report(cid, what, shift, shifts, err(out, s["ref"]), one, sat)  # both twins compute the base network's function
        assert shift == want_shift and (shifts == want).all(), (what, shift, want_shift, shifts, want)
        carried = mx.astype(np.float64) * np.exp2(shifts.astype(np.float64))
        assert (carried[shifts > 0] <= CAL_HEADROOM).all(), (what, carried.max())
        assert carried.max() <= ACT_MAX
        if what == "hidden Q8":  # the estimate sees nothing of this twin; the measurement lifts its hidden channels
            assert not expected_stream_shifts(d, tw).any() and (shifts[1::4] >= 6).all(), shifts[1::4]
        check_in_range(cid, what, out, forward_f64(d, tw, planes[idx]), one, sat)


# ---- 5. a leaf's bits under M8 ----
def test_a_leafs_bits_under_the_guarded_twin_do_not_depend_on_its_slot():
    case = CASES[1]
    s = setup_of(case)
    d, planes = s["d"], s["planes"]
    leaf = random_planes(d, 1, 1, 6)[0]
    tw = channel_twin(d, s["base"], CHANNEL_PATTERNS["M8"](d.filters))
    want = None
    with HipEvaluator(pack_tensors(d, tw), case[2], 1, dtype="f16x2", tower_form="winograd_f4", switches={}) as ev:
        assert ev.tower_kernel() == KERNEL
        shifts = ev.stream_shifts()
        assert shifts.min() < ev.stream_shift() == shifts.max()  # the twin with channels held back
        for slot in (0, 9, 11):
            batch = planes.copy()
            batch[slot] = leaf
            p, v = ev.eval(batch)
            if want is None:
                want = (p[slot].copy(), v[slot].copy())
            assert np.array_equal(p[slot], want[0]) and v[slot] == want[1], slot
        assert ev.stats()["saturated"] == 0
    ref = forward_f64(d, tw, leaf[None])
    e = err((want[0][None], np.array([want[1]])), ref)
    print("winof4_range f4_half   M8 one leaf : max |dlogit| %.3g |dvalue| %.3g" % e)
    assert outputs_equal_ref_tol(want[0][None], np.array([want[1]]), ref[0], ref[1])
