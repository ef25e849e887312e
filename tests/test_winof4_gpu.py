"""The Winograd F(4x4, 3x3) form of the f16x2 tower on the device: tower_form="winograd_f4" (conv3x3_winof4_kernel).

The form is opt-in and has bits of its own, so nothing here compares it bit for bit with another form: it is held to the reference-made
outputs by the reference's tolerance, to the float64 outputs by its own CPU emulation (profiles/winograd_gate_f4.json), to the exact f32
tower by cattus_hip_verify on the smallest shapes at which the kernel takes another path, and to itself (a leaf's bits depend on nothing
but the leaf).  tests/test_winof4_rule.py checks, without a GPU, the header the kernel is written with."""

import json
from pathlib import Path

import numpy as np
import pytest

from cattus_amd import synth
from cattus_amd.evaluator import CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, NetDesc, hex_game, pack_tensors, seeded_blob, seeded_tensors

from helpers import blob_for, outputs_equal_ref_tol

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KERNEL = "conv3x3_winof4_kernel"


def f4_eval(blob, max_batch, **kw):
    kw.setdefault("switches", {})
    return HipEvaluator(blob, max_batch, 1, dtype="f16x2", tower_form="winograd_f4", **kw)


def small_net(blocks, filters, seed=7):
    return seeded_blob(NetDesc(**CHESS, blocks=blocks, filters=filters, vhc=8, phc=8), seed)


# ---- 1. the reference-made fixtures ----
# The emulation's max |d| against float64 (profiles/winograd_gate_f4.json, winograd_f4_split): chess_4x128 4.35e-7 (policy) / 7.95e-8
# (value), chess_20x256 8.21e-7 / 1.98e-7.  The kernel may take 3x that: the F(2x2) kernel sits at 1.3x / 1.6x of ITS emulation on
# chess_20x256 because the MFMA's accumulation order is not torch's, and 3x leaves about 2x over that.  The hard bar is the reference's.
@pytest.mark.parametrize("name,batch", [("chess_4x128", 64), ("chess_20x256", 8)])
def test_fixtures_inside_the_reference_tolerance_and_near_the_emulation(name, batch):
    gate = {r["net"]: r["winograd_f4_split"] for r in json.loads((ROOT / "profiles" / "winograd_gate_f4.json").read_text())["results"]}[name]
    d, blob, z = blob_for(name)
    planes = z["planes"]
    assert len(planes) <= batch
    with f4_eval(blob, batch) as ev:
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)
        assert ev.stats()["saturated"] == 0
    dp, dv = float(np.abs(p - z["policy_f64"]).max()), float(np.abs(v - z["value_f64"].reshape(-1)).max())
    print("%s: max |dlogit| %.3g (emulation %.3g), max |dvalue| %.3g (emulation %.3g)" % (name, dp, gate["dp_vs_f64"], dv, gate["dv_vs_f64"]))
    assert outputs_equal_ref_tol(p, v, z["policy"], z["value"].reshape(-1))
    assert dp <= 3 * gate["dp_vs_f64"] and dv <= 3 * gate["dv_vs_f64"]


# ---- 2. small shapes against the exact tower ----
# (1, 128): no in-place skip, 4 cout blocks of 32, 8 k-steps; (2, 192): 6 cout blocks, skip rows over the output; (2, 256).  max_batch 8: one
# full board group; 12: a half group at the end (boards 8..11 beside four that do not exist); 80 with 77 leaves: ten groups, the last leaves
# short of the padding.
@pytest.mark.parametrize("blocks,filters", [(1, 128), (2, 192), (2, 256)])
@pytest.mark.parametrize("max_batch,n", [(8, 8), (12, 12), (80, 77)])
def test_small_shapes_verify_against_the_exact_tower(blocks, filters, max_batch, n):
    blob = small_net(blocks, filters)
    planes = synth.random_chess_planes(n, 3)
    with f4_eval(blob, max_batch, verify_every=1) as ev:
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)
        vs, st = ev.verify_stats(), ev.stats()
    assert np.isfinite(p).all() and np.isfinite(v).all()
    print("(%d, %d) batch %d: max_dlogit %.3g max_dvalue %.3g" % (blocks, filters, max_batch, vs["max_dlogit"], vs["max_dvalue"]))
    assert vs["leaves"] == n and vs["leaves_outside"] == 0 and st["saturated"] == 0


# ---- 3. a leaf's bits depend on nothing but the leaf ----
def test_a_leafs_bits_do_not_depend_on_its_slot_its_batch_or_the_memory_plan():
    blob = small_net(2, 192)
    fill = synth.random_chess_planes(80, 5)
    leaf = synth.random_chess_planes(1, 6)[0]
    want = None
    for max_batch, slots in ((8, (0, 5)), (12, (0, 5, 9, 11)), (80, (0, 5, 9, 76, 79))):
        with f4_eval(blob, max_batch) as ev:
            for slot in slots:
                batch = fill[:max_batch].copy()
                batch[slot] = leaf
                p, v = ev.eval(batch)
                if want is None:
                    want = (p[slot].copy(), v[slot].copy())
                assert np.array_equal(p[slot], want[0]) and v[slot] == want[1], (max_batch, slot)
            # a short batch (3, 7, 75 leaves: 4, 8, 76 boards), the leaf last: a half group alone, a full one, a half group at the end
            p, v = ev.eval(np.concatenate([fill[: max_batch - 6], leaf[None]]))
            assert np.array_equal(p[-1], want[0]) and v[-1] == want[1], (max_batch, "short")
    with f4_eval(blob, 12, switches={"CATTUS_WINO_INPLACE": "0"}) as ev:
        assert ev.tower_kernel() == KERNEL
        batch = fill[:12].copy()
        batch[9] = leaf
        p, v = ev.eval(batch)
    assert np.array_equal(p[9], want[0]) and v[9] == want[1]


# ---- 4. range ----
def test_activations_beyond_the_cap_are_counted_and_stay_finite():
    """The construction of test_winograd_tower_counts_inputs_that_leave_the_f16_range: a BatchNorm scale of 1e5 on the stem."""
    d = NetDesc(**CHESS, blocks=2, filters=128, vhc=8, phc=8)
    t = seeded_tensors(d, 6)
    t["_conv1._bn.weight"] = t["_conv1._bn.weight"] * np.float32(1e5)
    planes = synth.random_chess_planes(9, 4)
    with f4_eval(pack_tensors(d, t), 16) as ev:
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)
        first = ev.stats()["saturated"]
        ev.eval(planes)
        second = ev.stats()["saturated"]
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert first > 0 and second == 2 * first


# ---- 5. observation ----
def test_points_tap_and_trace_see_the_form():
    blob = small_net(4, 128)
    planes = synth.random_chess_planes(8, 8)
    with f4_eval(blob, 8) as ev:
        P = ev.points()
        assert P == 2 + 2 * 4
        p, v = ev.eval(planes)
        stem, tp, tv = ev.tap(planes, 0, outputs=True)
        last = ev.tap(planes, P - 2)
        assert np.array_equal(tp, p) and np.array_equal(tv, v)  # an observed pass computes what an unobserved one does
        assert stem.shape == last.shape == (8, 128, 8, 8) and np.isfinite(stem).all() and np.isfinite(last).all()
        assert (stem >= 0).all() and (last >= 0).all() and last.max() > 0
        rec, rp, rv = ev.trace(planes)
    assert np.array_equal(rp, p) and np.array_equal(rv, v)
    assert rec.shape == (P, 8) and (rec["flags"] == 0).all()
    for f in ("max_diff", "rms_diff", "rms_ref", "x", "ref"):
        assert np.isfinite(rec[f]).all(), f
    ratio = rec["rms_diff"][P - 2] / rec["rms_ref"][P - 2]
    print("rms_diff / rms_ref at the last stream point: max %.3g" % ratio.max())
    # 22-bit operands over 4 blocks: 1e-5 is ~40 units of 2^-22.  Measured: 4.5e-7 at most over the 8 leaves -- 22x room
    assert (ratio < 1e-5).all()


# ---- 6. plan ----
def test_auto_never_picks_the_form_and_uncovered_shapes_are_refused():
    blob = small_net(1, 128)
    with HipEvaluator(blob, 256, 1, dtype="f16x2", switches={}) as ev:
        assert ev.tower_kernel() == "tower_wino4_kernel"
    with HipEvaluator(blob, 128, 1, dtype="f16x2", switches={}) as ev:
        assert ev.tower_kernel() == "conv3x3_splitw_kernel"
    hex7 = seeded_blob(NetDesc(**hex_game(7), blocks=2, filters=128, vhc=8, phc=8), 1)
    no_blocks = seeded_blob(NetDesc(**CHESS, blocks=0, filters=128, vhc=8, phc=8), 1)
    for b, words, dtype in ((blob, 1, "bf16"), (hex7, 2, "f16x2"), (no_blocks, 1, "f16x2")):
        with pytest.raises(CattusHipError) as ei:
            HipEvaluator(b, 16, words, dtype=dtype, tower_form="winograd_f4", switches={})
        assert ei.value.status == -2, (dtype, words)  # CATTUS_E_UNSUPPORTED
