"""dtype "f32w" on the device: the f32-operand tower in Winograd F(2x2, 3x3) form on the f32 tower's rows (conv3x3_wino_f32_kernel).

Unlike the f16 towers this one can be pinned to a CPU restatement bit for bit: its stem is the exact f32 tower's, and every layer behind
it is an in-order fmaf chain that tests/wino_f32_layer_ref.cpp restates in the order of cattus_amd/csrc/wino_f32_rule.h.  Beside that
it is held to itself (a leaf's bits depend on nothing but the leaf), to the reference-made fixtures (the reference's cross-runtime bar,
and float64 by twice the exact f32 tower's error on the same leaves: the margin tests/test_splitk_gpu.py grants another f32 summation
order) and to the exact tower on networks whose stream is large.  tests/test_wino_f32_rule.py checks, without a GPU, the header the
kernel is written with.

Device figures, as this file prints them: profiles/f32w_numerics.txt."""

import ctypes as C

import numpy as np
import pytest

from cattus_amd import synth
from cattus_amd.evaluator import CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, NetDesc, hex_game, pack_tensors, seeded_blob, seeded_tensors

from helpers import blob_for, outputs_equal_ref_tol
from test_wino_f32_rule import build_layer_ref, run_layer_ref

pytestmark = pytest.mark.gpu

KERNEL = "conv3x3_wino_f32_kernel"
MARGIN = 2.0  # of the exact f32 tower's own error against float64


def w_eval(blob, max_batch, **kw):
    kw.setdefault("switches", {})
    return HipEvaluator(blob, max_batch, 1, dtype="f32w", **kw)


def x_eval(blob, max_batch, **kw):
    kw.setdefault("switches", {})
    return HipEvaluator(blob, max_batch, 1, dtype="f32", **kw)


def small_net(blocks, filters, seed=7):
    return seeded_blob(NetDesc(**CHESS, blocks=blocks, filters=filters, vhc=8, phc=8), seed)


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, dtype=np.float64)))))


def same(a, b):
    if isinstance(a, tuple):
        return all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def layer_ref(tmp_path_factory):
    return build_layer_ref(tmp_path_factory.mktemp("wino_f32_layer_ref"))


# ---- 1. creation: on the parent commit this fails with "unknown dtype 5" ----
@pytest.mark.parametrize("blocks,filters", [(1, 128), (2, 128), (1, 256)])
def test_the_dtype_creates_the_new_tower(blocks, filters):
    planes = synth.random_chess_planes(8, 3)
    with w_eval(small_net(blocks, filters), 8) as ev:
        assert ev.tower_kernel() == KERNEL
        assert ev.tail_leaves() == 0
        us, launches = ev.time_tower(8, 2)
        assert launches == 1 + 2 * blocks and us > 0  # the stem and 2 * blocks launches behind it
        p, v = ev.eval(planes)
        assert ev.stats()["saturated"] == 0
        assert (ev.stream_shifts() == 0).all() and ev.stream_shift() == 0
    assert p.shape == (8, CHESS["moves"]) and np.isfinite(p).all() and np.isfinite(v).all()
    assert np.abs(p).max() > 0


# ---- 2. a layer's bits are the CPU restatement's ----
def rows_of(tap):
    """tap's [n, C, 8, 8] -> the tower's rows [n * 64, C]."""
    return np.ascontiguousarray(tap.transpose(0, 2, 3, 1)).reshape(-1, tap.shape[1])


# (1, 128) on 3 leaves: one cout block per workgroup, a last board pair with a board that does not exist; (1, 256) on 128 leaves: the
# smallest grid on which a workgroup takes two cout blocks (wf32_ncb) -- restated for its first two leaves and its last
@pytest.mark.parametrize("filters,n,leaves", [(128, 3, (0, 1, 2)), (256, 128, (0, 1, 127))])
def test_a_layers_bits_are_the_cpu_restatements(layer_ref, tmp_path, filters, n, leaves):
    from oracle import oracle

    blob = small_net(1, filters)
    planes = synth.random_chess_planes(n, 11)
    with x_eval(blob, n) as ev:
        exact_stem = ev.tap(planes, 0)
    with w_eval(blob, n) as ev:
        assert ev.tower_kernel() == KERNEL
        stem, mid, out = (ev.tap(planes, point) for point in (0, 1, 2))
    assert same(stem, exact_stem)  # the stem is the exact tower's
    net = oracle.OracleNet(blob)
    pick = list(leaves)
    w1, b1 = net.folded_conv(1, filters)
    w2, b2 = net.folded_conv(2, filters)
    want_mid = run_layer_ref(layer_ref, tmp_path, rows_of(stem[pick]), w1, b1)
    assert np.abs(want_mid).max() > 0
    assert same(rows_of(mid[pick]), want_mid)
    want_out = run_layer_ref(layer_ref, tmp_path, rows_of(mid[pick]), w2, b2, skip=rows_of(stem[pick]))  # point 2: conv2 + the skip
    assert same(rows_of(out[pick]), want_out)


# ---- 3. two cout blocks per workgroup compute the same leaf ----
def test_two_cout_blocks_per_workgroup_compute_the_same_leaf():
    """128 leaves x 256 filters is the smallest grid on which a workgroup takes 64 couts; 126 leaves and fewer run the 32-cout workgroups."""
    blob = small_net(1, 256)
    planes = synth.random_chess_planes(128, 9)
    with w_eval(blob, 8) as ev:
        want = ev.eval(planes[:8])
    with w_eval(blob, 128) as ev:
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)                  # 128 boards: two cout blocks
        below = ev.eval(planes[:124])           # 124 boards: one, on the other side of the rule
        short = ev.eval(planes[:8])
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert same((p[:8], v[:8]), want) and same((short[0], short[1]), want)
    assert same((below[0], below[1]), (p[:124], v[:124]))


# ---- 4. a leaf's bits depend on the leaf alone ----
def test_a_leafs_bits_do_not_depend_on_its_slot_its_batch_the_lane_the_memory_plan_or_the_entry_point():
    torch = pytest.importorskip("torch")
    from oracle import oracle

    blob = small_net(2, 128)
    fill = synth.random_chess_planes(80, 5)
    leaf = synth.random_chess_planes(1, 6)[0]
    with w_eval(blob, 1) as ev:
        p, v = ev.eval(leaf[None])  # a batch of 1
        want = (p[0].copy(), v[0].copy())
    with w_eval(blob, 80) as ev:
        for size, slots in ((3, (0, 2)), (8, (0, 5)), (77, (0, 9, 76)), (80, (79,))):
            for slot in slots:
                batch = fill[:size].copy()
                batch[slot] = leaf
                p, v = ev.eval(batch)
                assert same((p[slot], v[slot]), want), (size, slot)
        batch = fill[:8].copy()
        batch[5] = leaf
        # the leaf server
        p, v = np.empty((8, 1880), dtype=np.float32), np.empty((8,), dtype=np.float32)
        f32p = C.POINTER(C.c_float)
        assert ev._lib.cattus_hip_apply(ev._h, batch.ctypes.data_as(C.POINTER(C.c_uint64)), 8, p.ctypes.data_as(f32p), v.ctypes.data_as(f32p)) == 0
        assert same((p[5], v[5]), want)
        tickets = [ev.submit(x) for x in list(fill[:2]) + [leaf]]
        ev.flush()
        got = [ev.wait(t) for t in tickets]
        assert same((got[-1][0], np.float32(got[-1][1])), want)
        # legal-move priors: the host softmax restatement on this tower's logits
        rng = np.random.default_rng(5)
        legal_idx = np.stack([rng.choice(1880, size=40, replace=False) for _ in range(8)]).astype(np.uint16)
        legal_count = rng.integers(1, 41, size=8).astype(np.uint16)
        probs, lv = ev.eval_legal(batch, legal_idx, legal_count)
        assert same(lv[5], want[1])
        assert same(probs[5, : legal_count[5]], oracle.softmax_legal_det(want[0], legal_idx[5, : legal_count[5]]))
        # device buffers, either lane
        dev = torch.device("cuda", 0)
        d_planes = torch.from_numpy(batch.view(np.int64)).to(dev)
        for lane in (0, 1):
            pol = torch.zeros((8, 1880), dtype=torch.float32, device=dev)
            val = torch.zeros((8,), dtype=torch.float32, device=dev)
            ev.eval_device(d_planes.data_ptr(), 8, pol.data_ptr(), val.data_ptr(), ev.lane_stream(lane), lane=lane)
            torch.cuda.synchronize()
            assert same((pol.cpu().numpy()[5], val.cpu().numpy()[5]), want), lane
    for switches in ({"CATTUS_WINO_INPLACE": "0"}, {"CATTUS_ARENA": "0"}, {"CATTUS_ARENA": "0", "CATTUS_WINO_INPLACE": "0"}):
        with w_eval(blob, 12, switches=switches) as ev:
            assert ev.tower_kernel() == KERNEL
            batch = fill[:12].copy()
            batch[9] = leaf
            p, v = ev.eval(batch)
        assert same((p[9], v[9]), want), switches


# ---- 5. the reference-made fixtures ----
@pytest.mark.parametrize("name", ["chess_4x128", "chess_20x256"])
def test_fixtures_are_inside_the_references_bar_and_within_twice_the_f32_towers_error_against_float64(name):
    d, blob, z = blob_for(name)
    planes = z["planes"]
    batch = len(planes)
    with w_eval(blob, batch) as ev:
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)
        assert ev.stats()["saturated"] == 0
    with x_eval(blob, batch) as ev:
        xp, xv = ev.eval(planes)
    p64, v64 = z["policy_f64"], z["value_f64"].reshape(-1)
    ew, ex = rms(p - p64), rms(xp - p64)
    vw, vx = float(np.abs(v - v64).max()), float(np.abs(xv - v64).max())
    print("%s (%d leaves) vs float64: rms |dlogit| f32w %.4g, f32 %.4g, ratio %.3f; max |dlogit| f32w %.4g, f32 %.4g; max |dvalue| f32w %.4g, f32 %.4g, ratio %.3f"
          % (name, batch, ew, ex, ew / ex, np.abs(p - p64).max(), np.abs(xp - p64).max(), vw, vx, vw / vx))
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert outputs_equal_ref_tol(p, v, z["policy"], z["value"].reshape(-1))
    assert ex > 0 and ew <= MARGIN * ex
    assert vx > 0 and vw <= MARGIN * vx


# ---- 6. large BatchNorm scales: the case the dtype exists for ----
@pytest.mark.parametrize("scale", [200.0, 1e5])
def test_large_batchnorm_scales_track_the_f32_tower_and_saturate_nothing(scale):
    """tests/test_hip_parity.py's test_f16x2_range_large_batchnorm_scales on a network wide enough for this form: a stem BatchNorm weight
    of 200, which the f16 towers still hold, and one of 1e5, which they clamp and count.  This tower has no range to leave."""
    d = NetDesc(**CHESS, blocks=2, filters=128, vhc=8, phc=8)
    planes = synth.random_chess_planes(9, 4)
    t = seeded_tensors(d, 6)
    t["_conv1._bn.weight"] = t["_conv1._bn.weight"] * np.float32(scale)
    t["_residual_blocks.0._conv1.weight"] = t["_residual_blocks.0._conv1.weight"] * np.float32(1e-3)  # tiny weights too
    blob = pack_tensors(d, t)
    with x_eval(blob, 16) as ev:
        want_p, want_v = ev.eval(planes)
    with w_eval(blob, 16) as ev:
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)
        ev.eval(planes)
        assert ev.stats()["saturated"] == 0
    print("stem BatchNorm x %g: max |logit| %.4g, max |dlogit| vs f32 %.4g, max |dvalue| %.4g" % (scale, np.abs(want_p).max(), np.abs(p - want_p).max(), np.abs(v - want_v).max()))
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert np.abs(want_p).max() > 20  # the scale did reach the logits
    np.testing.assert_allclose(p, want_p, rtol=2e-5, atol=2e-5 * np.abs(want_p).max())
    np.testing.assert_allclose(v, want_v, rtol=1e-4, atol=1e-6)


# ---- 7. observation and verification on the tower itself ----
def test_points_tap_trace_and_verify_see_the_tower_on_itself():
    blob = small_net(2, 128)
    planes = synth.random_chess_planes(8, 8)
    with w_eval(blob, 8) as ev:
        P = ev.points()
        assert P == 2 + 2 * 2
        p, v = ev.eval(planes)
        stem, tp, tv = ev.tap(planes, 0, outputs=True)
        last = ev.tap(planes, P - 2)
        assert same((tp, tv), (p, v))  # an observed pass computes what an unobserved one does
        assert stem.shape == last.shape == (8, 128, 8, 8) and np.isfinite(stem).all() and np.isfinite(last).all()
        assert (stem >= 0).all() and (last >= 0).all() and last.max() > 0
        rec, rp, rv = ev.trace(planes)
        assert ev.tower_kernel() == KERNEL
    assert same((rp, rv), (p, v))
    assert rec.shape == (P, 8) and (rec["flags"] == 0).all()
    for f in ("max_diff", "rms_diff", "rms_ref", "x", "ref"):
        assert np.isfinite(rec[f]).all(), f
    assert (rec["max_diff"][0] == 0).all()  # the stem is the shadow's
    with x_eval(blob, 8) as ev:
        exact = ev.tap(planes, P - 2)
    # tap decodes the rows the tower keeps: the exact tower's tensor to another f32 summation order -- the record's figure
    ours = np.sqrt(np.mean(np.square(last.astype(np.float64) - exact), axis=(1, 2, 3)))
    assert np.allclose(ours, rec["rms_diff"][P - 2], rtol=1e-3)
    ratio = rec["rms_diff"][P - 2] / rec["rms_ref"][P - 2]
    print("rms_diff / rms_ref at the last stream point: f32w mean %.3g max %.3g" % (ratio.mean(), ratio.max()))
    assert 0 < ratio.max() < 1e-5  # f32 against f32: 2^-24 a rounding, two blocks deep; the F(4x4) test's bound for 22-bit operands
    with w_eval(blob, 8, verify_every=1) as ev:
        vp, vv = ev.eval(planes)
        vs = ev.verify_stats()
        assert vs["batches"] == 1 and vs["leaves"] == 8 and vs["leaves_outside"] == 0, vs
        ev.verify_prior_stats()  # not refused: this evaluator has a shadow
    assert same((vp, vv), (p, v))  # with verification: bit for bit the outputs without it


# ---- 8. more than 32 planes: K0 + the stem as an ordinary f32 layer ----
def test_a_network_of_forty_planes():
    from test_many_planes_gpu import random_planes

    d = NetDesc(planes=40, board=8, moves=1880, blocks=1, filters=128, vhc=8, phc=8)
    blob = seeded_blob(d, 7)
    planes = random_planes(d, 1, 3, 5)
    with x_eval(blob, 3) as ev:
        want_p, want_v = ev.eval(planes)
        want_stem = ev.tap(planes, 0)
    with w_eval(blob, 3) as ev:
        assert ev.tower_kernel() == KERNEL
        assert ev.stem_input() == (64, True)
        p, v = ev.eval(planes)
        assert same(ev.tap(planes, 0), want_stem)
    assert np.abs(want_p).max() > 0
    assert outputs_equal_ref_tol(p, v, want_p, want_v)


# ---- 9. plan and refusals ----
def test_auto_and_winograd_are_the_form_and_everything_else_is_refused():
    blob = small_net(1, 128)
    planes = synth.random_chess_planes(8, 3)
    outs = []
    for form in ("auto", "winograd"):
        with w_eval(blob, 16, tower_form=form) as ev:
            assert ev.tower_kernel() == KERNEL
            outs.append(ev.eval(planes))
            with pytest.raises(CattusHipError) as ei:
                ev.stream_range(planes)
            assert ei.value.status == -2
    assert same(outs[0], outs[1])
    hex7 = seeded_blob(NetDesc(**hex_game(7), blocks=2, filters=128, vhc=8, phc=8), 1)
    no_blocks = seeded_blob(NetDesc(**CHESS, blocks=0, filters=128, vhc=8, phc=8), 1)
    wide_head = seeded_blob(NetDesc(**CHESS, blocks=1, filters=128, vhc=8, phc=28), 1)
    cases = [(hex7, 2, "auto"), (no_blocks, 1, "auto"), (small_net(2, 64), 1, "auto"), (wide_head, 1, "auto"), (blob, 1, "direct"), (blob, 1, "winograd_f4"),
             (blob, 1, "direct_splitk")]
    for b, words, form in cases:
        with pytest.raises(CattusHipError) as ei:
            HipEvaluator(b, 16, words, dtype="f32w", tower_form=form, switches={})
        assert ei.value.status == -2, (words, form)  # CATTUS_E_UNSUPPORTED
