"""The split-K direct form of the f16x2 tower on the device: tower_form="direct_splitk" (conv3x3_splitk_kernel).

The form divides the K walk of every layer behind the stem over the W waves of a workgroup and adds the W partial sums in f32, so its
bits are its own -- except with one way, where it must BE the direct form.  It is therefore held to the direct form bit for bit where
that is exact (CATTUS_SPLITK_WAYS=1; networks whose weights are zero outside one wave's range), to the reference-made outputs by the
reference's tolerance, to float64 relative to the direct form, to the exact f32 tower by cattus_hip_verify, and to itself (a leaf's bits
depend on nothing but the leaf).  tests/test_splitk_rule.py checks, without a GPU, the header the kernel is written with.

Shapes (blocks x filters): 1x128 = 4 chunks, 2x192 = 6 chunks in uneven ranges (2, 2, 1, 1), 2x256 = 8 chunks, 1x320 = 10 chunks in
uneven ranges over 8 waves.  Batches (max_batch, n): (1, 1) one board among three of padding, (3, 3) and (9, 9) odd board counts,
(40, 33) a grid of hundreds of workgroups with leaves short of max_batch."""

import functools

import numpy as np
import pytest

from cattus_amd import synth
from cattus_amd.evaluator import CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, NetDesc, hex_game, pack_tensors, seeded_blob, seeded_tensors

from helpers import blob_for, forward_f64, outputs_equal_ref_tol

pytestmark = pytest.mark.gpu

KERNEL = "conv3x3_splitk_kernel"
SHAPES = [(1, 128), (2, 192), (2, 256), (1, 320)]
BATCHES = [(1, 1), (3, 3), (9, 9), (40, 33)]


def sk_eval(blob, max_batch, words=1, ways=None, **kw):
    kw.setdefault("switches", {} if ways is None else {"CATTUS_SPLITK_WAYS": str(ways)})
    return HipEvaluator(blob, max_batch, words, dtype="f16x2", tower_form="direct_splitk", **kw)


def direct_eval(blob, max_batch, words=1, **kw):
    kw.setdefault("switches", {})
    return HipEvaluator(blob, max_batch, words, dtype="f16x2", tower_form="direct", **kw)


def small_desc(blocks, filters):
    return NetDesc(**CHESS, blocks=blocks, filters=filters, vhc=8, phc=8)


@functools.lru_cache(maxsize=None)
def small_net(blocks, filters, seed=7):
    return seeded_blob(small_desc(blocks, filters), seed)


@functools.lru_cache(maxsize=None)
def leaves(n, seed=3):
    return synth.random_chess_planes(n, seed)


@functools.lru_cache(maxsize=None)
def direct_outputs(blocks, filters, max_batch, n):
    """The direct form's logits and values on leaves(n): computed once, shared, never written to."""
    with direct_eval(small_net(blocks, filters), max_batch) as ev:
        assert ev.tower_kernel() == "conv3x3_splitw_kernel"
        p, v = ev.eval(leaves(n))
    p.setflags(write=False), v.setflags(write=False)
    return p, v


# ---- 1. one way is the direct form, bit for bit ----
@pytest.mark.parametrize("blocks,filters", SHAPES)
@pytest.mark.parametrize("max_batch,n", BATCHES)
def test_one_way_is_the_direct_form_bit_for_bit(blocks, filters, max_batch, n):
    with sk_eval(small_net(blocks, filters), max_batch, ways=1) as ev:
        assert ev.tower_kernel() == KERNEL
        assert ev.splitk_plan() == (1, [0, filters // 32])
        p, v = ev.eval(leaves(n))
        assert ev.stats()["saturated"] == 0
    pd, vd = direct_outputs(blocks, filters, max_batch, n)
    assert np.array_equal(p, pd) and np.array_equal(v, vd)


# ---- 2. range twins, at the default W ----
@pytest.mark.parametrize("blocks,filters,want_bounds", [(2, 192, [0, 2, 4, 5, 6]), (2, 256, [0, 1, 2, 3, 4, 5, 6, 7, 8])])
def test_range_twins_equal_the_direct_form(blocks, filters, want_bounds):
    """Weights zero outside one wave's range: every other partial and every skipped term is an exact zero on both sides."""
    d = small_desc(blocks, filters)
    base = seeded_tensors(d, 7)
    planes = leaves(9)
    with sk_eval(small_net(blocks, filters), 9) as ev:
        ways, bounds = ev.splitk_plan()
    assert bounds == want_bounds and ways == len(bounds) - 1
    for w in range(ways):
        t = dict(base)
        for i in range(blocks):
            for conv in ("_conv1", "_conv2"):
                key = f"_residual_blocks.{i}.{conv}.weight"
                wgt = np.zeros_like(base[key])
                wgt[:, 32 * bounds[w]:32 * bounds[w + 1]] = base[key][:, 32 * bounds[w]:32 * bounds[w + 1]]
                t[key] = wgt
        blob = pack_tensors(d, t)
        with sk_eval(blob, 9) as ev:
            assert ev.tower_kernel() == KERNEL and ev.splitk_plan() == (ways, bounds)
            p, v = ev.eval(planes)
        with direct_eval(blob, 9) as ev:
            pd, vd = ev.eval(planes)
        assert np.abs(pd).max() > 0
        assert np.array_equal(p, pd) and np.array_equal(v, vd), (w, bounds)


# ---- 3. the reference-made fixtures ----
@pytest.mark.parametrize("name,batch", [("chess_4x128", 64), ("chess_20x256", 8)])
def test_fixtures_inside_the_reference_tolerance(name, batch):
    d, blob, z = blob_for(name)
    planes = z["planes"]
    assert len(planes) <= batch
    with sk_eval(blob, batch) as ev:
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)
        assert ev.stats()["saturated"] == 0
    assert outputs_equal_ref_tol(p, v, z["policy"], z["value"].reshape(-1))


# ---- 4. against float64, relative to the direct form ----
# The two forms are f32 summation orders of equal quality; maxima over ~1e5 logits fluctuate: at most 2x the direct form's figure.
# Measured on an MI355X (profiles/splitk_numerics.txt): see that file.
def _f64_case(name):
    if name == "2x256":
        d = small_desc(2, 256)
        t = seeded_tensors(d, 7)
        planes = leaves(33)
        p64, v64 = forward_f64(d, t, planes)
        return pack_tensors(d, t), planes, 40, np.asarray(p64), np.asarray(v64).reshape(-1)
    d, blob, z = blob_for(name)
    return blob, z["planes"], {"chess_4x128": 64, "chess_20x256": 8}[name], z["policy_f64"], z["value_f64"].reshape(-1)


@pytest.mark.parametrize("name", ["2x256", "chess_4x128", "chess_20x256"])
def test_error_against_float64_is_at_most_twice_the_direct_forms(name):
    blob, planes, batch, p64, v64 = _f64_case(name)
    figures = {}
    for form, make in (("direct", direct_eval), ("direct_splitk", sk_eval)):
        with make(blob, batch) as ev:
            p, v = ev.eval(planes)
        figures[form] = (float(np.abs(p - p64).max()), float(np.abs(v - v64).max()))
    (dp_d, dv_d), (dp_s, dv_s) = figures["direct"], figures["direct_splitk"]
    print("splitk-numerics: %-12s %3d leaves  max |dlogit| direct %.4g  direct_splitk %.4g   max |dvalue| direct %.4g  direct_splitk %.4g"
          % (name, len(planes), dp_d, dp_s, dv_d, dv_s))
    assert dp_s <= 2 * dp_d and dv_s <= 2 * dv_d


# ---- 5. against the exact tower ----
@pytest.mark.parametrize("blocks,filters", SHAPES)
@pytest.mark.parametrize("max_batch,n", BATCHES)
def test_small_shapes_verify_against_the_exact_tower(blocks, filters, max_batch, n):
    blob = small_net(blocks, filters)
    results = {}
    for form, make in (("direct", direct_eval), ("direct_splitk", sk_eval)):
        with make(blob, max_batch, verify_every=1) as ev:
            p, v = ev.eval(leaves(n))
            results[form] = (ev.verify_stats(), ev.stats(), np.isfinite(p).all() and np.isfinite(v).all())
    for form, (vs, st, finite) in results.items():
        print("%s (%d, %d) batch %d: max_dlogit %.3g max_dvalue %.3g" % (form, blocks, filters, max_batch, vs["max_dlogit"], vs["max_dvalue"]))
    for form, (vs, st, finite) in results.items():  # the direct form too: a failure of the bar itself is visible
        assert finite and vs["leaves"] == n and vs["leaves_outside"] == 0 and st["saturated"] == 0, form


# ---- 6. a leaf's bits depend on nothing but the leaf ----
def test_a_leafs_bits_do_not_depend_on_its_slot_or_its_batch():
    blob = small_net(2, 192)
    fill = leaves(40, 5)
    leaf = leaves(1, 6)[0]
    want, plan = None, None
    for max_batch, slots in ((1, (0,)), (3, (0, 2)), (9, (0, 5, 8)), (40, (0, 5, 9, 36, 39))):
        with sk_eval(blob, max_batch) as ev:
            assert ev.tower_kernel() == KERNEL
            if plan is None:
                plan = ev.splitk_plan()
            assert ev.splitk_plan() == plan == (4, [0, 2, 4, 5, 6])
            for slot in slots:
                batch = fill[:max_batch].copy()
                batch[slot] = leaf
                p, v = ev.eval(batch)
                if want is None:
                    want = (p[slot].copy(), v[slot].copy())
                assert np.array_equal(p[slot], want[0]) and v[slot] == want[1], (max_batch, slot)
            if max_batch > 1:  # a short batch, the leaf last: 2, 6 and 33 leaves
                short = {3: 2, 9: 6, 40: 33}[max_batch]
                p, v = ev.eval(np.concatenate([fill[: short - 1], leaf[None]]))
                assert np.array_equal(p[-1], want[0]) and v[-1] == want[1], (max_batch, "short")


# ---- 7. range ----
def test_activations_beyond_the_f16_range_are_counted_and_stay_finite():
    """The construction of test_winof4_gpu.py's range case: a BatchNorm scale of 1e5 on the stem."""
    d = small_desc(2, 128)
    t = seeded_tensors(d, 6)
    t["_conv1._bn.weight"] = t["_conv1._bn.weight"] * np.float32(1e5)
    planes = leaves(9, 4)
    with sk_eval(pack_tensors(d, t), 16) as ev:
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)
        first = ev.stats()["saturated"]
        ev.eval(planes)
        second = ev.stats()["saturated"]
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert first > 0 and second == 2 * first


# ---- 8. observation ----
def test_points_tap_and_trace_see_the_form():
    blob = small_net(4, 128)
    planes = leaves(8, 8)
    with sk_eval(blob, 8) as ev:
        P = ev.points()
        assert P == 2 + 2 * 4
        p, v = ev.eval(planes)
        stem, tp, tv = ev.tap(planes, 0, outputs=True)
        mid = ev.tap(planes, 1)
        last = ev.tap(planes, P - 2)
        assert np.array_equal(tp, p) and np.array_equal(tv, v)  # an observed pass computes what an unobserved one does
        assert stem.shape == mid.shape == last.shape == (8, 128, 8, 8)
        for x in (stem, mid, last):
            assert np.isfinite(x).all() and (x >= 0).all() and x.max() > 0
        rec, rp, rv = ev.trace(planes)
    with direct_eval(blob, 8) as ev:
        dstem = ev.tap(planes, 0)
        dmid = ev.tap(planes, 1)
    assert np.array_equal(stem, dstem)  # the stem runs on the kernel it runs on in the direct form
    assert np.allclose(mid, dmid, rtol=1e-4, atol=1e-5)  # rows in the direct form's layout: another f32 order, nothing else
    assert np.array_equal(rp, p) and np.array_equal(rv, v)
    assert rec.shape == (P, 8) and (rec["flags"] == 0).all()
    for f in ("max_diff", "rms_diff", "rms_ref", "x", "ref"):
        assert np.isfinite(rec[f]).all(), f
    ratio = rec["rms_diff"][P - 2] / rec["rms_ref"][P - 2]
    print("rms_diff / rms_ref at the last stream point: max %.3g" % ratio.max())
    assert (ratio < 1e-5).all()  # the bound of the F(4x4) test, which the direct form satisfies


# ---- 9. plan ----
def test_auto_never_picks_the_form_and_uncovered_shapes_are_refused():
    blob = small_net(1, 128)
    for max_batch, kernel in ((4, "conv3x3_splitw_kernel"), (128, "conv3x3_splitw_kernel"), (256, "tower_wino4_kernel")):
        with HipEvaluator(blob, max_batch, 1, dtype="f16x2", switches={}) as ev:
            assert ev.tower_kernel() == kernel, max_batch
            with pytest.raises(CattusHipError) as ei:
                ev.splitk_plan()
            assert ei.value.status == -2
    hex9 = seeded_blob(NetDesc(**hex_game(9), blocks=2, filters=128, vhc=8, phc=8), 1)
    narrow = small_net(2, 64)
    no_blocks = small_net(0, 128)
    for b, words, dtype in ((blob, 1, "bf16"), (blob, 1, "f16"), (blob, 1, "f32"), (hex9, 2, "f16x2"), (narrow, 1, "f16x2"), (no_blocks, 1, "f16x2")):
        with pytest.raises(CattusHipError) as ei:
            HipEvaluator(b, 16, words, dtype=dtype, tower_form="direct_splitk", switches={})
        assert ei.value.status == -2, (dtype, words)  # CATTUS_E_UNSUPPORTED
    with pytest.raises(CattusHipError) as ei:  # the form needs the fragment-order weights
        HipEvaluator(blob, 16, 1, dtype="f16x2", tower_form="direct_splitk", switches={"CATTUS_SPLIT_W": "0"})
    assert ei.value.status == -2


def test_hex7_with_128_filters_is_accepted_and_inside_the_bar():
    """49 live pixels of 64 slots, two words per plane."""
    d = NetDesc(**hex_game(7), blocks=2, filters=128, vhc=8, phc=8)
    blob = seeded_blob(d, 1)
    planes = synth.random_hex_planes(9, 7, 2)
    results = {}
    for form, make in (("direct", direct_eval), ("direct_splitk", sk_eval)):
        with make(blob, 9, words=2, verify_every=1) as ev:
            if form == "direct_splitk":
                assert ev.tower_kernel() == KERNEL and ev.splitk_plan() == (4, [0, 1, 2, 3, 4])
            p, v = ev.eval(planes)
            results[form] = (ev.verify_stats(), ev.stats(), np.isfinite(p).all() and np.isfinite(v).all())
    for form, (vs, st, finite) in results.items():
        assert finite and vs["leaves"] == 9 and vs["leaves_outside"] == 0 and st["saturated"] == 0, form
