"""Stream shifts from measured activations, on the GPU: cattus_hip_stream_range and cattus_hip_create_calibrated.

1. Range against float64.  HipEvaluator.stream_range of an f32 evaluator against the network in float64 (cattus_amd.torch_model.
   PolicyValueNet built from the raw tensors, as helpers.forward_f64 builds it) with the stem output and every block's output captured:
   rms and abs_max per channel over leaves x pixels x stream tensors.  Shapes small enough that one miscounted pixel or padded board shows:

       ttt 0x8      3 leaves    stem only, 27 values per channel (one wrong value moves the mean square by ~1 / 27)
       chess 2x64   5 leaves    64-slot boards
       hex9 2x40    37 leaves   128-slot boards of which 81 slots are live, 40 of 64 channels, an odd board in the last workgroup
       chess 1x128  150 leaves  an evaluator of max_batch 64: three chunks, the last of 22 leaves

   RMS_RTOL / ABS_MAX_RTOL are 4x the largest relative error measured on an MI355X -- the f32 tower's own error against float64:
       ttt_0x8 rms 1.35e-7 abs_max 2.74e-7 | chess_2x64 2.05e-7 4.48e-7 | hex9_2x40 1.03e-7 1.61e-7 | chess_1x128 2.30e-7 4.03e-7
   (rms and abs_max come back as f32: up to 6e-8 of each figure is that rounding)
   and neither may exceed 1e-4 (the constants are asserted against that too).
2. Determinism and isolation: the same call twice gives the same bytes, and eval before and after a range pass the same bits.
3. The hidden twin (test_stream_calibration.hidden_twin with the Q8 pattern: the channel twin's function, its scale where the estimate of
   stream_shifts does not look) on four of test_split_range_gpu.CASES -- a direct 64-slot case, the direct 128-slot one, the resident
   tower and the one-launch Winograd tower.  A plain HipEvaluator reports the estimate's shifts, 0 on the hidden channels, and gives the
   bits of the Q8 channel twin under CATTUS_STREAM_SHIFT=0 (the folded tensors and the shifts are the same); with it the direct and
   resident kernels leave bar (a) (F16X2_*_ATOL_VS_F64 against the twin's own forward_f64), the Winograd tower, which splits only its
   transformed input, stays inside it.  With calibration= (the case's own planes): (i) the shifts are calibrated_shifts_restated of
   stream_range of an f32 evaluator on the same planes; (ii) every hidden channel has t_k >= 6; (iii) bar (a); (iv) bar (b), at most
   SCALE_RATIO_MAX x the base network's error on the sampled leaves; (v) nothing saturates; (vi) the case's kernel ran.
4. The base seeded network with calibration=: bars (a), (c), (d) of test_channel_scale_gpu.py; its shifts are the restatement's again
   and need not be the estimate's zeros.
5. Refusals and identities.

Measured on an MI355X, max |dlogit| / max |dvalue| of f16x2 against float64 on the hidden twin, plain | calibrated (and x the base network's):
    direct_cb1    4.45e-6 / 9.73e-7 | 7.27e-7 / 8.86e-8  (1.19x / 1.16x)    hidden channels at t_k 8..13, the others 2..4, global 2
    direct_big    3.70e-6 / 6.75e-7 | 3.08e-7 / 3.38e-8  (0.84x / 0.76x)    9..12, 3..5, 3
    wino_tower    9.88e-7 / 1.45e-7 | 6.05e-7 / 5.47e-8  (1.11x / 1.26x)    8..12, 2..4, 2
    tower64s      6.39e-6 / 1.91e-6 | 5.35e-7 / 9.35e-8  (1.04x / 1.33x)    9..11, 2, 2
(the plain runs are the recorded Q8-without-shifts figures of test_channel_scale_gpu.py, as they must be).  The seeded networks' streams
measure at an rms of 0.2 .. 0.4 where the estimate says about 1: calibrated, the base network runs at a global shift of 2, per channel 2..5,
at 7.15e-7 / 7.37e-8, 3.98e-7 / 3.38e-8, 5.45e-7 / 5.24e-8, 4.91e-7 / 7.86e-8 in the order above.
"""

import numpy as np
import pytest

from cattus_amd.evaluator import CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, TTT, NetDesc, hex_game, pack_tensors, seeded_tensors

from helpers import CHANNEL_PATTERNS, channel_twin, forward_f64, planes_to_f64
from test_channel_scale_gpu import expected_stream_shifts
from test_f16_tower_gpu import random_planes
from test_hip_parity import F16X2_POLICY_ATOL_VS_F64, F16X2_VALUE_ATOL_VS_F64
from test_split_range_gpu import CASES, SCALE_RATIO_MAX, SEED, desc_of, err, expected_stream_shift, sample
from test_stream_calibration import calibrated_shifts_restated, hidden_twin

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -2

# 4x the largest measured relative error of the f32 tower's rms / abs_max against float64 (the table above: 2.30e-7, 4.48e-7)
RMS_RTOL, ABS_MAX_RTOL = 9.2e-7, 1.8e-6

RANGE_SHAPES = [
    # id, game, blocks, filters, plane words, leaves, max_batch of the evaluator
    ("ttt_0x8", TTT, 0, 8, 1, 3, 3),
    ("chess_2x64", CHESS, 2, 64, 1, 5, 5),
    ("hex9_2x40", hex_game(9), 2, 40, 2, 37, 37),
    ("chess_1x128", CHESS, 1, 128, 1, 150, 64),
]


def stream_range_f64(desc: NetDesc, tensors: dict, planes: np.ndarray):
    """(rms, abs_max) per stream channel in float64: the stem output and every block's output of PolicyValueNet, loaded from the raw
    tensors as helpers.forward_f64 loads it, over leaves x pixels x the 1 + blocks tensors."""
    import torch

    from cattus_amd.torch_model import PolicyValueNet

    net = PolicyValueNet(desc).to(torch.float64)
    sd = net.state_dict()
    for k in sd:
        if not k.endswith("num_batches_tracked"):
            sd[k] = torch.from_numpy(np.asarray(tensors[k], dtype=np.float64).reshape(tuple(sd[k].shape)))
    net.load_state_dict(sd, strict=True)
    net.eval()
    with torch.no_grad():
        x = net._cbr(net._conv1, torch.from_numpy(planes_to_f64(planes, desc.board)))
        streams = [x]
        for b in net._residual_blocks:
            t = torch.relu(b._bn1(b._conv1(x)))
            x = torch.relu(x + b._bn2(b._conv2(t)))
            streams.append(x)
        s = torch.stack(streams)  # [1 + blocks, n, F, S, S]
    assert s.shape == (1 + desc.blocks, len(planes), desc.filters, desc.board, desc.board)
    return (s * s).mean(dim=(0, 1, 3, 4)).sqrt().numpy(), s.abs().amax(dim=(0, 1, 3, 4)).numpy()


def rel_err(got, ref):
    assert (got[ref == 0] == 0).all()
    live = ref != 0
    return float((np.abs(got[live] - ref[live]) / ref[live]).max()) if live.any() else 0.0


def test_the_range_tolerances_are_tight_enough_to_see_one_wrong_element():
    assert RMS_RTOL <= 1e-4 and ABS_MAX_RTOL <= 1e-4


@pytest.mark.parametrize("shape", RANGE_SHAPES, ids=[s[0] for s in RANGE_SHAPES])
def test_stream_range_is_the_float64_networks(shape):
    name, game, blocks, filters, words, n, batch = shape
    d = NetDesc(**game, blocks=blocks, filters=filters, vhc=4, phc=4)
    tensors = seeded_tensors(d, SEED)
    planes = random_planes(d, words, n, 7)
    with HipEvaluator(pack_tensors(d, tensors), batch_size=batch, plane_words=words, dtype="f32", switches={}) as ev:
        assert ev.tower_kernel() == "conv3x3_mfma_v2_kernel"
        rms, mx = ev.stream_range(planes)
    assert rms.dtype == np.float32 and rms.shape == (filters,) and mx.shape == (filters,)
    want_rms, want_mx = stream_range_f64(d, tensors, planes)
    er, em = rel_err(rms.astype(np.float64), want_rms), rel_err(mx.astype(np.float64), want_mx)
    print("%s: stream_range vs f64, max relative error rms %.3g abs_max %.3g" % (name, er, em))
    assert (want_rms > 0).sum() >= filters - 1  # a channel that ReLU kills on every leaf (one of ttt's eight) must read 0; the others are compared
    assert er <= RMS_RTOL and em <= ABS_MAX_RTOL, (name, er, em)


def test_stream_range_is_deterministic_and_leaves_evaluations_alone():
    d = NetDesc(**CHESS, blocks=1, filters=128, vhc=4, phc=4)
    planes = random_planes(d, 1, 150, 7)
    with HipEvaluator(pack_tensors(d, seeded_tensors(d, SEED)), batch_size=64, plane_words=1, dtype="f32", switches={}) as ev:
        p0, v0 = ev.eval(planes[:64])
        first = ev.stream_range(planes)
        p1, v1 = ev.eval(planes[:64])
        second = ev.stream_range(planes)
        # a shorter pass in between: the accumulators start from zero on every call
        short = ev.stream_range(planes[:3])
        third = ev.stream_range(planes)
        p2, v2 = ev.eval(planes[:64])
        batches = ev.stats()["batches"]
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(first, third):
        assert a.tobytes() == b.tobytes()
    assert (short[1] <= first[1]).all() and short[0].tobytes() != first[0].tobytes()
    assert p0.tobytes() == p1.tobytes() == p2.tobytes() and v0.tobytes() == v1.tobytes() == v2.tobytes()
    assert batches == 3  # a range pass is no evaluation


TWIN_CASES = [c for c in CASES if c[0] in ("direct_cb1", "direct_big", "tower64s", "wino_tower")]
_f64_cache = {}


def f64_of(key, d, tensors, planes):
    """forward_f64 once per (network, what) -- the reference is shared between the tests and left as it is"""
    if key not in _f64_cache:
        _f64_cache[key] = forward_f64(d, tensors, planes)
    return _f64_cache[key]


def run_case(case, tensors, planes, calibration=None, extra=None):
    """One f16x2 evaluator of the case: (policy, value) of every leaf, global shift, per-channel shifts, saturated; the case's kernel ran."""
    cid, net, n, form, switches, kernel = case
    d, words = desc_of(net)
    with HipEvaluator(pack_tensors(d, tensors), batch_size=n, plane_words=words, dtype="f16x2", tower_form=form, switches={**switches, **(extra or {})},
                      calibration=calibration) as ev:
        assert ev.tower_kernel() == kernel, (cid, ev.tower_kernel())
        p, v = ev.eval(planes)
        shift, shifts, sat = ev.stream_shift(), ev.stream_shifts(), ev.stats()["saturated"]
    assert np.isfinite(p).all() and np.isfinite(v).all(), cid
    return (p, v), shift, shifts, sat


def measured_shifts(d, words, tensors, planes):
    """calibrated_stream_shifts restated, on what an f32 evaluator (of the batch cattus_hip_create_calibrated measures with) reports"""
    with HipEvaluator(pack_tensors(d, tensors), batch_size=min(len(planes), 256), plane_words=words, dtype="f32", switches={}) as ev:
        rms, mx = ev.stream_range(planes)
    return calibrated_shifts_restated(rms, mx)


@pytest.mark.parametrize("case", TWIN_CASES, ids=[c[0] for c in TWIN_CASES])
def test_calibration_finds_the_scale_the_estimate_misses(case):
    cid, net, n = case[:3]
    d, words = desc_of(net)
    base = seeded_tensors(d, SEED)
    planes = random_planes(d, words, n, 5)
    idx = sample(n)
    e = CHANNEL_PATTERNS["Q8"](d.filters)
    hidden = e < 0
    ht = hidden_twin(d, base, e)
    at = lambda out: (out[0][idx], out[1][idx])
    out, _, _, _ = run_case(case, base, planes)
    one = err(at(out), f64_of((net, n, "base"), d, base, planes[idx]))
    ref = f64_of((net, n, "hidden"), d, ht, planes[idx])
    # a plain evaluator: the estimate's shifts, nothing on the hidden channels; the Q8 channel twin without its shifts, to the bit
    plain, shift, shifts, sat = run_case(case, ht, planes)
    assert shift == expected_stream_shift(d, ht) == 0 and (shifts == expected_stream_shifts(d, ht)).all() and not shifts[hidden].any() and sat == 0
    q8, shift, shifts, _ = run_case(case, channel_twin(d, base, e), planes, extra={"CATTUS_STREAM_SHIFT": "0"})
    assert shift == 0 and not shifts.any()
    assert plain[0].tobytes() == q8[0].tobytes() and plain[1].tobytes() == q8[1].tobytes()
    pp, pv = err(at(plain), ref)
    print("%s hidden twin, plain: f16x2 vs f64 max |dlogit| %.3g |dvalue| %.3g (%.2f / %.2f x base)" % (cid, pp, pv, pp / one[0], pv / one[1]))
    if case[3] == "winograd":
        assert pp <= F16X2_POLICY_ATOL_VS_F64 and pv <= F16X2_VALUE_ATOL_VS_F64, (pp, pv)
    else:
        assert pp > F16X2_POLICY_ATOL_VS_F64 or pv > F16X2_VALUE_ATOL_VS_F64, ("the hidden twin passes (a) without calibration", pp, pv)
    # calibrated on the case's own planes
    cal, shift, shifts, sat = run_case(case, ht, planes, calibration=planes)
    want_shift, want = measured_shifts(d, words, ht, planes)
    cp, cv = err(at(cal), ref)
    print("%s hidden twin, calibrated: shift %d, hidden channels %d..%d, others %d..%d: f16x2 vs f64 max |dlogit| %.3g |dvalue| %.3g (%.2f / %.2f x base) saturated %d"
          % (cid, shift, shifts[hidden].min(), shifts[hidden].max(), shifts[~hidden].min(), shifts[~hidden].max(), cp, cv, cp / one[0], cv / one[1], sat))
    assert shift == want_shift and (shifts == want).all(), (shift, want_shift, shifts, want)  # (i)
    assert (shifts[hidden] >= 6).all(), shifts[hidden]  # (ii)
    assert cp <= F16X2_POLICY_ATOL_VS_F64 and cv <= F16X2_VALUE_ATOL_VS_F64, (cp, cv)  # (iii)
    assert cp <= SCALE_RATIO_MAX[0] * one[0] and cv <= SCALE_RATIO_MAX[1] * one[1], (cp / one[0], cv / one[1])  # (iv)
    assert sat == 0, sat  # (v); (vi) is run_case's


@pytest.mark.parametrize("case", TWIN_CASES, ids=[c[0] for c in TWIN_CASES])
def test_calibration_keeps_the_seeded_network_inside_its_bars(case):
    cid, net, n = case[:3]
    d, words = desc_of(net)
    base = seeded_tensors(d, SEED)
    planes = random_planes(d, words, n, 5)
    idx = sample(n)
    out, shift, shifts, sat = run_case(case, base, planes, calibration=planes)
    ep, ev_ = err((out[0][idx], out[1][idx]), f64_of((net, n, "base"), d, base, planes[idx]))
    print("%s base, calibrated: shift %d, per channel %d..%d: f16x2 vs f64 max |dlogit| %.3g |dvalue| %.3g saturated %d" % (cid, shift, shifts.min(), shifts.max(), ep, ev_, sat))
    want_shift, want = measured_shifts(d, words, base, planes)
    assert shift == want_shift and (shifts == want).all(), (shift, want_shift, shifts, want)
    assert sat == 0, sat
    assert ep <= F16X2_POLICY_ATOL_VS_F64 and ev_ <= F16X2_VALUE_ATOL_VS_F64, (ep, ev_)


def test_refusals_and_identities():
    d, words = desc_of("hex7_6x64")
    tensors = seeded_tensors(d, SEED)
    blob = pack_tensors(d, tensors)
    planes = random_planes(d, words, 8, 5)
    ref = forward_f64(d, tensors, planes)
    for dtype in ("f16x2", "bf16", "f16"):
        with HipEvaluator(blob, batch_size=8, plane_words=words, dtype=dtype, switches={}) as ev:
            with pytest.raises(CattusHipError) as bad:
                ev.stream_range(planes)
            assert bad.value.status == E_UNSUPPORTED, dtype
    with HipEvaluator(blob, batch_size=8, plane_words=words, dtype="f32", switches={"CATTUS_FORCE_GENERIC": "1"}) as ev:
        with pytest.raises(CattusHipError) as bad:  # the SIMT checker keeps NCHW tensors: not the tower that is measured
            ev.stream_range(planes)
        assert bad.value.status == E_UNSUPPORTED
    with HipEvaluator(blob, batch_size=8, plane_words=words, dtype="f32", switches={}) as ev:
        import ctypes as C

        from cattus_amd.evaluator import ChannelRange, _u64

        out = (ChannelRange * (d.filters + 1))()
        assert ev._lib.cattus_hip_stream_range(ev._h, _u64(planes), 8, out, d.filters + 1) == E_INVALID
        assert ev._lib.cattus_hip_stream_range(ev._h, _u64(planes), 8, out, d.filters - 1) == E_INVALID
        assert ev._lib.cattus_hip_stream_range(ev._h, _u64(planes), 0, out, d.filters) == E_INVALID
        assert ev._lib.cattus_hip_stream_range(ev._h, _u64(planes), 8, out, d.filters) == 0
        assert C.sizeof(ChannelRange) == 8
        want = ev.eval(planes)
    # nothing to calibrate: the plain evaluator's bits, and the planes are still validated
    for dtype in ("f32", "bf16"):
        with HipEvaluator(blob, batch_size=8, plane_words=words, dtype=dtype, switches={}) as ev:
            plain = ev.eval(planes)
        with HipEvaluator(blob, batch_size=8, plane_words=words, dtype=dtype, switches={}, calibration=planes) as ev:
            got = ev.eval(planes)
            assert ev.stream_shift() == 0 and not ev.stream_shifts().any()
        assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes(), dtype
        if dtype == "f32":
            assert got[0].tobytes() == want[0].tobytes()
        with pytest.raises(CattusHipError) as bad:
            HipEvaluator(blob, batch_size=8, plane_words=words, dtype=dtype, switches={}, calibration=planes[:0])
        assert bad.value.status == E_INVALID, dtype
    with pytest.raises(CattusHipError) as bad:
        HipEvaluator(blob, batch_size=8, plane_words=words, dtype="f16x2", switches={}, calibration=planes[:0])
    assert bad.value.status == E_INVALID
    # one leaf is a calibration set; through the diagnostic entry point as well (per-layer launches instead of the resident tower)
    for switches, kernel in (({}, "tower64_split_kernel"), ({"CATTUS_TOWER64": "0"}, "conv3x3_splitw_kernel")):
        with HipEvaluator(blob, batch_size=8, plane_words=words, dtype="f16x2", switches=switches, calibration=planes[:1]) as ev:
            assert ev.tower_kernel() == kernel
            p, v = ev.eval(planes)
            shifts = ev.stream_shifts()
        with HipEvaluator(blob, batch_size=1, plane_words=words, dtype="f32", switches={}) as ev:
            want_shift, want_shifts = calibrated_shifts_restated(*ev.stream_range(planes[:1]))
        assert (shifts == want_shifts).all()
        assert np.abs(p - ref[0]).max() <= F16X2_POLICY_ATOL_VS_F64 and np.abs(v - ref[1]).max() <= F16X2_VALUE_ATOL_VS_F64
