"""dtype "f16w" on the device: the single-term f16 tower in Winograd F(2x2, 3x3) form with an f32 stream (conv3x3_wino_f16_kernel).

The dtype has bits of its own, so nothing here compares it bit for bit with another tower: it is held to the exact f32 tower and to the
float64 outputs of the reference-made fixtures by the direct f16 tower's error on the same leaves (the tower it is an alternative to:
the CPU emulation, profiles/winograd_gate_f16w.json, puts it at 0.5 - 0.9 of that error), and to itself (a leaf's bits depend on nothing
but the leaf).  tests/test_wino_f16_rule.py checks, without a GPU, the header the kernel is written with.

Device figures of the first build, as this file prints them (rms |dlogit| f16w / direct f16, ratio):
    see profiles/f16w_numerics.txt"""

import json
from pathlib import Path

import numpy as np
import pytest

from cattus_amd import synth
from cattus_amd.evaluator import CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, NetDesc, hex_game, pack_tensors, seeded_blob, seeded_tensors

from helpers import blob_for, stream_twin

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KERNEL = "conv3x3_wino_f16_kernel"


def w_eval(blob, max_batch, **kw):
    kw.setdefault("switches", {})
    return HipEvaluator(blob, max_batch, 1, dtype="f16w", **kw)


def small_net(blocks, filters, seed=7):
    return seeded_blob(NetDesc(**CHESS, blocks=blocks, filters=filters, vhc=8, phc=8), seed)


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, dtype=np.float64)))))


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


# ---- 1. creation ----
def test_the_dtype_creates_the_new_tower():
    planes = synth.random_chess_planes(8, 3)
    with w_eval(small_net(2, 192), 8) as ev:
        assert ev.tower_kernel() == KERNEL
        assert ev.tail_leaves() == 0
        p, v = ev.eval(planes)
        assert ev.stats()["saturated"] == 0
    assert p.shape == (8, CHESS["moves"]) and np.isfinite(p).all() and np.isfinite(v).all()
    assert np.abs(p).max() > 0


# ---- 2. small shapes against the exact tower, beside the direct f16 tower ----
# (1, 128): the fewest chunks (4: one pass of the ring and one step more), no in-place skip; (2, 192): 6 chunks, cin % 64 == 32, skip rows
# over the output; (2, 256): 8 chunks, two steps behind the ring's last whole pass.  max_batch 8: whole workgroups; 12: a last board group
# some of whose boards do not exist; 80 with 77 leaves: a grid that is no multiple of 8 with 192 filters (240 workgroups are; 160 and 320),
# leaves short of the padding.  (2, 128) at 256 leaves: the grid from which a workgroup takes two cout blocks (wf16_ncb).
_refs = {}


def reference_outputs(blocks, filters, max_batch, n):
    """(planes, f32 outputs, direct-f16 outputs) of a shape, computed once."""
    key = (blocks, filters, max_batch, n)
    if key not in _refs:
        blob, planes = small_net(blocks, filters), synth.random_chess_planes(n, 3)
        with HipEvaluator(blob, max_batch, 1, dtype="f32", switches={}) as ev:
            exact = ev.eval(planes)
        with HipEvaluator(blob, max_batch, 1, dtype="f16", switches={}) as ev:
            assert ev.tower_kernel() == "conv3x3_mfma_v2_kernel"
            direct = ev.eval(planes)
        _refs[key] = (planes, exact, direct)
    return _refs[key]


@pytest.mark.parametrize("blocks,filters,bar", [(1, 128, 1.25), (2, 192, 1.0), (2, 256, 1.0)])
@pytest.mark.parametrize("max_batch,n", [(8, 8), (12, 12), (80, 77)])
def test_small_shapes_are_at_least_as_close_to_the_exact_tower_as_the_direct_f16_tower(blocks, filters, bar, max_batch, n):
    planes, (xp, xv), (dp, dv) = reference_outputs(blocks, filters, max_batch, n)
    with w_eval(small_net(blocks, filters), max_batch) as ev:
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)
        assert ev.stats()["saturated"] == 0
    assert np.isfinite(p).all() and np.isfinite(v).all()
    ew, ed = rms(p - xp), rms(dp - xp)
    print("(%d, %d) batch %d/%d: rms |dlogit| f16w %.3g, direct f16 %.3g, ratio %.3f; max f16w %.3g direct %.3g; max |dvalue| f16w %.3g direct %.3g"
          % (blocks, filters, n, max_batch, ew, ed, ew / ed, np.abs(p - xp).max(), np.abs(dp - xp).max(), np.abs(v - xv).max(), np.abs(dv - xv).max()))
    assert ed > 0 and ew <= bar * ed


def test_two_cout_blocks_per_workgroup_compute_the_same_leaf():
    """256 leaves x 128 filters is the smallest grid on which a workgroup takes 64 couts; 8 leaves run the 32-cout workgroups."""
    blob = small_net(2, 128)
    planes = synth.random_chess_planes(256, 9)
    with w_eval(blob, 8) as ev:
        want = ev.eval(planes[:8])
    with HipEvaluator(blob, 8, 1, dtype="f32", switches={}) as ev:
        exact = ev.eval(planes[:8])
    with w_eval(blob, 256) as ev:
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)
        short = ev.eval(planes[:8])  # 8 boards of a 256-board evaluator: 32-cout workgroups again
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert rms(want[0] - exact[0]) < 1e-3  # an 11-bit tower, not garbage
    assert same(p[:8], want[0]) and same(v[:8], want[1])
    assert same(short[0], want[0]) and same(short[1], want[1])


# ---- 3. the reference-made fixtures against float64 ----
@pytest.mark.parametrize("name,batch", [("chess_4x128", 64), ("chess_20x256", 8)])
def test_fixtures_are_closer_to_float64_than_the_direct_f16_tower(name, batch):
    gate = {r["net"]: r for r in json.loads((ROOT / "profiles" / "winograd_gate_f16w.json").read_text())["results"]}[name]
    d, blob, z = blob_for(name)
    planes = z["planes"]
    assert len(planes) <= batch
    with w_eval(blob, batch) as ev:
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)
        assert ev.stats()["saturated"] == 0
    with HipEvaluator(blob, batch, 1, dtype="f16", switches={}) as ev:
        dp, dv = ev.eval(planes)
    p64, v64 = z["policy_f64"], z["value_f64"].reshape(-1)
    ew, ed = rms(p - p64), rms(dp - p64)
    print("%s: rms |dlogit| vs f64 f16w %.3g (emulation %.3g), direct f16 %.3g (emulation %.3g), ratio %.3f (emulation %.3f); max f16w %.3g direct %.3g; "
          "max |dvalue| f16w %.3g direct %.3g"
          % (name, ew, gate["f16w"]["rms_dp_vs_f64"], ed, gate["f16_direct"]["rms_dp_vs_f64"], ew / ed, gate["f16w"]["rms_dp_vs_f64"] / gate["f16_direct"]["rms_dp_vs_f64"],
             np.abs(p - p64).max(), np.abs(dp - p64).max(), np.abs(v - v64).max(), np.abs(dv - v64).max()))
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert ew <= ed


# ---- 4. a leaf's bits depend on the leaf alone ----
def test_a_leafs_bits_do_not_depend_on_its_slot_its_batch_the_memory_plan_or_the_entry_point():
    blob = small_net(2, 192)
    fill = synth.random_chess_planes(80, 5)
    leaf = synth.random_chess_planes(1, 6)[0]
    want = None
    for max_batch, slots in ((8, (0, 5)), (12, (0, 5, 9, 11)), (80, (0, 5, 9, 76, 79))):
        with w_eval(blob, max_batch) as ev:
            for slot in slots:
                batch = fill[:max_batch].copy()
                batch[slot] = leaf
                p, v = ev.eval(batch)
                if want is None:
                    want = (p[slot].copy(), v[slot].copy())
                assert same(p[slot], want[0]) and same(v[slot], want[1]), (max_batch, slot)
            # a short batch (3, 7, 75 leaves), the leaf last
            p, v = ev.eval(np.concatenate([fill[: max_batch - 6], leaf[None]]))
            assert same(p[-1], want[0]) and same(v[-1], want[1]), (max_batch, "short")
            # the leaf server: the leaf among others, flushed
            tickets = [ev.submit(x) for x in list(fill[:2]) + [leaf]]
            ev.flush()
            got = [ev.wait(t) for t in tickets]
            assert same(got[-1][0], want[0]) and same(np.float32(got[-1][1]), want[1]), (max_batch, "server")
    for switches in ({"CATTUS_WINO_INPLACE": "0"}, {"CATTUS_ARENA": "0"}, {"CATTUS_ARENA": "0", "CATTUS_WINO_INPLACE": "0"}):
        with w_eval(blob, 12, switches=switches) as ev:
            assert ev.tower_kernel() == KERNEL
            batch = fill[:12].copy()
            batch[9] = leaf
            p, v = ev.eval(batch)
        assert same(p[9], want[0]) and same(v[9], want[1]), switches


# ---- 5. the cap ----
def test_activations_beyond_the_cap_are_counted_and_stay_finite():
    """The construction of tests/test_winof4_gpu.py: a BatchNorm scale of 1e5 on the stem."""
    d = NetDesc(**CHESS, blocks=2, filters=128, vhc=8, phc=8)
    t = seeded_tensors(d, 6)
    planes = synth.random_chess_planes(9, 4)
    with w_eval(pack_tensors(d, t), 16) as ev:  # the ordinary network counts nothing
        ev.eval(planes)
        assert ev.stats()["saturated"] == 0
    t["_conv1._bn.weight"] = t["_conv1._bn.weight"] * np.float32(1e5)
    with w_eval(pack_tensors(d, t), 16) as ev:
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)
        first = ev.stats()["saturated"]
        ev.eval(planes)
        second = ev.stats()["saturated"]
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert first > 0 and second == 2 * first


# ---- 6. observation ----
def test_points_tap_and_trace_see_the_tower_on_itself():
    blob = small_net(2, 128)
    planes = synth.random_chess_planes(8, 8)
    with w_eval(blob, 8) as ev:
        P = ev.points()
        assert P == 2 + 2 * 2
        p, v = ev.eval(planes)
        stem, tp, tv = ev.tap(planes, 0, outputs=True)
        last = ev.tap(planes, P - 2)
        assert same(tp, p) and same(tv, v)  # an observed pass computes what an unobserved one does
        assert stem.shape == last.shape == (8, 128, 8, 8) and np.isfinite(stem).all() and np.isfinite(last).all()
        assert (stem >= 0).all() and (last >= 0).all() and last.max() > 0
        rec, rp, rv = ev.trace(planes)
        assert ev.tower_kernel() == KERNEL
    assert same(rp, p) and same(rv, v)
    assert rec.shape == (P, 8) and (rec["flags"] == 0).all()
    for f in ("max_diff", "rms_diff", "rms_ref", "x", "ref"):
        assert np.isfinite(rec[f]).all(), f
    with HipEvaluator(blob, 8, 1, dtype="f16", switches={}) as ev:
        drec, _, _ = ev.trace(planes)
    with HipEvaluator(blob, 8, 1, dtype="f32", switches={}) as ev:
        exact = ev.tap(planes, P - 2)
    # tap decodes the rows the tower keeps (f32, channel k at 2^t_k): the exact tower's tensor to 11-bit operands -- the record's figure
    ours = np.sqrt(np.mean(np.square(last.astype(np.float64) - exact), axis=(1, 2, 3)))
    assert np.allclose(ours, rec["rms_diff"][P - 2], rtol=1e-3)
    ratio, dratio = rec["rms_diff"][P - 2] / rec["rms_ref"][P - 2], drec["rms_diff"][P - 2] / drec["rms_ref"][P - 2]
    print("rms_diff / rms_ref at the last stream point: f16w mean %.3g max %.3g, direct f16 mean %.3g max %.3g" % (ratio.mean(), ratio.max(), dratio.mean(), dratio.max()))
    assert ratio.mean() <= dratio.mean()


def test_tap_decodes_a_shifted_stream_to_network_units():
    """A network whose stream is 2^-6 of the seeded one's carries it at 2^6 (stream_shifts): tap gives network units back."""
    d = NetDesc(**CHESS, blocks=2, filters=128, vhc=8, phc=8)
    blob = pack_tensors(d, stream_twin(d, seeded_tensors(d, 7), 2.0**-6))
    planes = synth.random_chess_planes(4, 8)
    with w_eval(blob, 4) as ev:
        shifts = ev.stream_shifts()
        last = ev.tap(planes, ev.points() - 2)
    with HipEvaluator(blob, 4, 1, dtype="f32", switches={}) as ev:
        exact = ev.tap(planes, ev.points() - 2)
    assert (shifts > 0).all()
    # 11-bit operands over two blocks: a relative rms error of 1e-2 is 20 units of 2^-11; a missing 2^-t_k would be a factor of 2^6
    assert rms(last - exact) <= 1e-2 * rms(exact)


# ---- 7. calibration ----
def test_calibration_is_accepted_and_a_seeded_net_keeps_its_shifts_and_its_bits():
    """cattus_hip_create_calibrated takes the dtype.  The tower's stream is f32, so it keeps the estimate's shifts and takes the measured
    headroom guard alone (weight_layout.h: calibrated_stream_shifts_f32_stream): a seeded net, whose estimate is right, gives all shifts
    0 and the bits of the uncalibrated evaluator."""
    blob = small_net(2, 128)
    planes = synth.random_chess_planes(8, 3)
    with w_eval(blob, 8) as ev:
        assert (ev.stream_shifts() == 0).all()
        want = ev.eval(planes)
    with w_eval(blob, 8, calibration=synth.random_chess_planes(16, 12)) as ev:
        assert ev.tower_kernel() == KERNEL
        shift, shifts = ev.stream_shift(), ev.stream_shifts()
        p, v = ev.eval(planes)
        assert ev.stats()["saturated"] == 0
    assert shift == 0 and shifts.shape == (128,) and (shifts == 0).all()
    assert same(p, want[0]) and same(v, want[1])


def test_calibration_lowers_a_shift_that_would_carry_a_channel_past_the_cap():
    """What the sample is for on this tower: the guard.  A network whose stream is 2^-6 of the seeded one's carries it at 2^6 by the
    estimate; every fourth channel is then made 2^14 larger where gamma does not show it (test_stream_calibration.hidden_twin), so the
    estimate still gives those channels the global shift and they run at 2^14 times the seeded size: past the cap of 16,376, counted.
    Calibrated on the leaves it evaluates, the tower lowers the shift of every channel whose measured largest |value| 2^6 exceeds 4096
    until it fits -- the estimate's shifts guarded, restated here -- and nothing saturates.  Only enlarged channels can be among them
    (the others measure below 1, far under 64); an enlarged channel whose seeded values stay under 0.25 needs no lowering and gets none."""
    from test_channel_scale_gpu import expected_stream_shifts
    from test_stream_calibration import hidden_twin

    d = NetDesc(**CHESS, blocks=2, filters=128, vhc=8, phc=8)
    hidden = np.arange(128) % 4 == 1
    tensors = hidden_twin(d, stream_twin(d, seeded_tensors(d, 7), 2.0**-6), np.where(hidden, 14, 0))
    blob = pack_tensors(d, tensors)
    planes = synth.random_chess_planes(16, 3)
    estimate = expected_stream_shifts(d, tensors)
    with HipEvaluator(blob, 16, 1, dtype="f32", switches={}) as ev:
        _, abs_max = ev.stream_range(planes)
        exact = ev.eval(planes)
    want = estimate.copy()
    for k in range(128):
        while want[k] > 0 and float(abs_max[k]) * 2.0 ** int(want[k]) > 4096.0:
            want[k] -= 1
    with w_eval(blob, 16) as ev:
        assert (ev.stream_shifts() == estimate).all()
        plain = ev.eval(planes)
        plain_sat = ev.stats()["saturated"]
    with w_eval(blob, 16, calibration=planes) as ev:
        assert ev.tower_kernel() == KERNEL
        shifts = ev.stream_shifts()
        p, v = ev.eval(planes)
        sat = ev.stats()["saturated"]
    print("estimate %d..%d; calibrated: hidden channels %d..%d, others %d..%d; saturated plain %d calibrated %d; rms |dlogit| vs f32 plain %.3g calibrated %.3g"
          % (estimate.min(), estimate.max(), shifts[hidden].min(), shifts[hidden].max(), shifts[~hidden].min(), shifts[~hidden].max(), plain_sat, sat,
             rms(plain[0] - exact[0]), rms(p - exact[0])))
    assert (estimate > 0).all() and (shifts == want).all()
    assert (shifts <= estimate).all() and (shifts[hidden] < estimate[hidden]).any() and (shifts[~hidden] == estimate[~hidden]).all()
    assert plain_sat > 0 and sat == 0
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert rms(p - exact[0]) <= rms(plain[0] - exact[0])


# ---- 8. plan and refusals ----
def test_auto_and_winograd_are_the_form_and_everything_else_is_refused():
    blob = small_net(1, 128)
    planes = synth.random_chess_planes(8, 3)
    outs = []
    for form in ("auto", "winograd"):
        with w_eval(blob, 16, tower_form=form) as ev:
            assert ev.tower_kernel() == KERNEL
            outs.append(ev.eval(planes))
    assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1])
    hex7 = seeded_blob(NetDesc(**hex_game(7), blocks=2, filters=128, vhc=8, phc=8), 1)
    no_blocks = seeded_blob(NetDesc(**CHESS, blocks=0, filters=128, vhc=8, phc=8), 1)
    cases = [(hex7, 2, "auto"), (no_blocks, 1, "auto"), (small_net(2, 64), 1, "auto"), (blob, 1, "direct"), (blob, 1, "winograd_f4"), (blob, 1, "direct_splitk")]
    for b, words, form in cases:
        with pytest.raises(CattusHipError) as ei:
            HipEvaluator(b, 16, words, dtype="f16w", tower_form=form, switches={})
        assert ei.value.status == -2, (words, form)  # CATTUS_E_UNSUPPORTED
