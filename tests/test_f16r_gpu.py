"""dtype "f16r" on the device: the direct single-term f16 tower with the residual stream kept in f32 (conv3x3_f16r_kernel, K1hr).

The tower has bits of its own from point 2 on, and dtype f16's before that: a network without blocks and point 1 of any network are
compared with dtype f16 bit for bit, point 2 by a derived bound, everything behind it by dtype f16's error on the same leaves against
the exact f32 tower and against the float64 outputs of the reference-made fixtures (the CPU emulation, profiles/gate_f16r.json, puts
it at 0.44 - 0.82 of that error), and to itself (a leaf's bits depend on nothing but the leaf; the tile does not enter them).
tests/test_f16r_rule.py checks, without a GPU, the header the epilogue and the evaluator are written with.

Seeded networks have vhc = phc = 4 unless a fixture is named.  Device figures of the first build, as this file prints them:
    see profiles/f16r_numerics.txt"""

import ctypes as C
import functools
import json
from pathlib import Path

import numpy as np
import pytest

from cattus_amd import synth
from cattus_amd.evaluator import CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, TTT, NetDesc, hex_game, pack_tensors, seeded_blob, seeded_tensors, simple_desc

from helpers import CHANNEL_PATTERNS, blob_for, channel_twin, stream_twin

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KERNEL, F16_KERNEL = "conv3x3_f16r_kernel", "conv3x3_mfma_v2_kernel"


def r_eval(blob, max_batch, words=1, dtype="f16r", **kw):
    kw.setdefault("switches", {})
    return HipEvaluator(blob, max_batch, words, dtype=dtype, **kw)


def chess_desc(blocks, filters):
    return NetDesc(**CHESS, blocks=blocks, filters=filters, vhc=4, phc=4)


@functools.lru_cache(maxsize=None)
def chess_net(blocks, filters, seed=7):
    return seeded_blob(chess_desc(blocks, filters), seed)


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, dtype=np.float64)))))


def same(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. creation ----
def test_the_dtype_creates_the_new_tower():
    planes = synth.random_chess_planes(8, 3)
    with r_eval(chess_net(2, 128), 8) as ev:
        assert ev.tower_kernel() == KERNEL
        assert ev.time_tower(8, 1)[1] == 1 + 2 * 2
        assert ev.tail_leaves() == 0
        p, v = ev.eval(planes)
        assert ev.stats()["saturated"] == 0
    assert p.shape == (8, CHESS["moves"]) and np.isfinite(p).all() and np.isfinite(v).all()
    assert np.abs(p).max() > 0


# ---- 2. the anchors to dtype f16, bit for bit ----
def test_a_network_without_blocks_has_dtype_f16s_bits():
    blob, planes = chess_net(0, 64), synth.random_chess_planes(5, 3)
    with r_eval(blob, 5) as ev:
        assert ev.tower_kernel() == KERNEL and ev.time_tower(5, 1)[1] == 1
        p, v = ev.eval(planes)
        assert ev.stats()["saturated"] == 0
    with r_eval(blob, 5, dtype="f16") as ev:
        assert ev.tower_kernel() == F16_KERNEL
        fp, fv = ev.eval(planes)
    assert np.abs(p).max() > 0
    assert same(p, fp) and same(v, fv)


@functools.lru_cache(maxsize=None)
def one_block_taps():
    """Points 0, 1, 2 of a 1-block chess net of 128 filters on 5 leaves under f16r and under f16, and what either counted."""
    blob, planes = chess_net(1, 128), synth.random_chess_planes(5, 3)
    out = {}
    for dtype, kernel in (("f16r", KERNEL), ("f16", F16_KERNEL)):
        with r_eval(blob, 5, dtype=dtype) as ev:
            assert ev.tower_kernel() == kernel and ev.points() == 4
            out[dtype] = [ev.tap(planes, point) for point in range(3)], ev.stats()["saturated"]
        for t in out[dtype][0]:
            t.setflags(write=False)
    return out


def test_point_1_is_dtype_f16s_and_point_0_rounds_to_it():
    (r, rsat), (f, fsat) = one_block_taps()["f16r"], one_block_taps()["f16"]
    assert r[0].shape == f[0].shape == (5, 128, 8, 8) and r[0].max() > 0 and r[1].max() > 0
    assert same(r[1], f[1])  # conv1 read the same operand copy and ran dtype f16's layer
    assert same(np.float16(r[0]).astype(np.float32), f[0])  # the stream, rounded once, is dtype f16's stem
    assert not same(r[0], f[0])  # and is itself not rounded
    assert rsat == 0 and fsat == 0


# ---- 3. the f32 skip, by a derived bound ----
def test_point_2_differs_from_dtype_f16s_by_the_rounding_of_the_skip_and_no_more():
    """Behind conv2 of block 0 the two towers hold relu(c + skip) with the same conv sum c (the same MFMAs on the same bits: point 1 is
    equal).  dtype f16 rounds the skip to 11 bits (<= 2^-11 |p0|) and its result to at most 11 bits (<= 2^-11 |p2|); ReLU is
    1-Lipschitz; 2^-20 (|p0| + |p2|) covers the f32 roundings of the two sums and the second order.  p0, p2: f16r's own taps.  At
    least one element differs: a skip rounded to f16 after all would give dtype f16's bits."""
    (r, _), (f, _) = one_block_taps()["f16r"], one_block_taps()["f16"]
    p0, p2 = r[0].astype(np.float64), r[2].astype(np.float64)
    diff = np.abs(p2 - f[2].astype(np.float64))
    bound = 2.0**-11 * np.abs(p0) + 2.0**-11 * np.abs(p2) + 2.0**-20 * (np.abs(p0) + np.abs(p2))
    live = bound > 0
    print("point 2, f16r against f16: %d of %d elements differ, max |diff| %.3g, max diff / bound %.3f"
          % ((diff > 0).sum(), diff.size, diff.max(), (diff[live] / bound[live]).max()))
    assert (diff <= bound).all(), float((diff - bound).max())
    assert (diff > 0).any()


# ---- 4. tiles and shapes compute the same leaf ----
# name: (game, plane words, planes or None for the game's, blocks, filters, leaves = max_batch, switches of the second evaluator)
SHAPES = {
    "chess_2x128_cb1": ("chess", 1, None, 2, 128, 8, {"CATTUS_CONV_CB": "1"}),
    "chess_2x128_cb2": ("chess", 1, None, 2, 128, 8, {"CATTUS_CONV_CB": "2"}),
    "chess_2x128_pbw1": ("chess", 1, None, 2, 128, 8, {"CATTUS_CONV_CB": "1", "CATTUS_CONV_PBW": "1"}),
    "chess_2x128_pbw2": ("chess", 1, None, 2, 128, 8, {"CATTUS_CONV_CB": "1", "CATTUS_CONV_PBW": "2"}),
    "hex11_2x64": ("hex11", 2, None, 2, 64, 8, {"CATTUS_CONV_CB": "2"}),       # BIG: 128 pixel slots per board
    "hex7_6x64": ("hex7", 2, None, 6, 64, 16, {"CATTUS_CONV_CB": "2"}),
    "ttt_2x64": ("ttt", 1, None, 2, 64, 64, {"CATTUS_CONV_CB": "2"}),
    "chess_2x16": ("chess", 1, None, 2, 16, 32, {"CATTUS_CONV_PBW": "2"}),     # 16 filters padded to 64
    "planes40_2x64": ("chess", 1, 40, 2, 64, 16, {"CATTUS_CONV_CB": "2"}),      # more than 32 planes: the packed stem
    "chess_2x64_unfused": ("chess", 1, None, 2, 64, 16, {"CATTUS_FUSED_STEM": "0"}),  # 18 planes through the packed stem
}
GAMES = {"chess": CHESS, "ttt": TTT, "hex7": hex_game(7), "hex11": hex_game(11)}


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(desc, blob, plane words, planes, f32 outputs, f16 outputs, f16r outputs on the default tile) of a shape, computed once."""
    game, words, nplanes, blocks, filters, n, _ = SHAPES[name]
    g = dict(GAMES[game])
    if nplanes is not None:
        g["planes"] = nplanes
    d = NetDesc(**g, blocks=blocks, filters=filters, vhc=4, phc=4)
    blob = seeded_blob(d, 7)
    rng = np.random.default_rng(5)
    hw = d.board * d.board
    bits = rng.integers(0, 2, size=(n, d.planes, hw), dtype=np.uint64)
    planes = np.zeros((n, d.planes, words), dtype=np.uint64)
    for i in range(hw):
        planes[:, :, i >> 6] |= bits[:, :, i] << np.uint64(i & 63)
    out = []
    for dtype in ("f32", "f16", "f16r"):
        with r_eval(blob, n, words, dtype=dtype) as ev:
            assert ev.tower_kernel() == (KERNEL if dtype == "f16r" else F16_KERNEL)
            out.append(ev.eval(planes))
            if dtype != "f32":
                assert ev.stats()["saturated"] == 0
    return (d, blob, words, planes, *out)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_tiles_and_shapes_compute_the_same_leaf_and_stay_inside_dtype_f16s_error(name):
    d, blob, words, planes, (xp, xv), (fp, fv), (p, v) = shape_case(name)
    switches = SHAPES[name][6]
    with r_eval(blob, len(planes), words, switches=switches) as ev:
        assert ev.tower_kernel() == KERNEL
        if name in ("planes40_2x64", "chess_2x64_unfused"):
            assert ev.stem_input()[1], "the packed stem"
        sp, sv = ev.eval(planes)
        assert ev.stats()["saturated"] == 0
    assert np.isfinite(p).all() and np.isfinite(v).all() and np.abs(p).max() > 0
    assert same(sp, p) and same(sv, v), switches
    er, ef = rms(p - xp), rms(fp - xp)
    bar = 1.25 if d.blocks == 1 else 1.0
    print("%s: rms |dlogit| vs f32 f16r %.3g, f16 %.3g, ratio %.3f; max |dvalue| f16r %.3g f16 %.3g" % (name, er, ef, er / ef, np.abs(v - xv).max(), np.abs(fv - xv).max()))
    assert ef > 0 and er <= bar * ef


def test_256_leaves_on_the_default_tile_give_the_bits_of_8():
    """8 leaves of 128 filters run the 128-row x 32-cout workgroups, 256 leaves the 256-row x 32-cout ones."""
    blob = chess_net(2, 128)
    planes = synth.random_chess_planes(256, 9)
    with r_eval(blob, 8) as ev:
        want = ev.eval(planes[:8])
    with r_eval(blob, 256) as ev:
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)
        short = ev.eval(planes[:8])
        assert ev.stats()["saturated"] == 0
    with r_eval(blob, 256, dtype="f32") as ev:
        xp, _ = ev.eval(planes)
    with r_eval(blob, 256, dtype="f16") as ev:
        fp, _ = ev.eval(planes)
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert same(p[:8], want[0]) and same(v[:8], want[1])
    assert same(short[0], want[0]) and same(short[1], want[1])
    print("chess 2x128, 256 leaves: rms |dlogit| vs f32 f16r %.3g, f16 %.3g, ratio %.3f" % (rms(p - xp), rms(fp - xp), rms(p - xp) / rms(fp - xp)))
    assert rms(p - xp) <= rms(fp - xp)


# ---- 5. the reference-made fixtures against float64 ----
@pytest.mark.parametrize("name,batch,words", [("chess_4x128", 64, 1), ("chess_20x256", 8, 1), ("hex7_6x64", 8, 2)])
def test_fixtures_are_at_least_as_close_to_float64_as_dtype_f16(name, batch, words):
    gate = {r["net"]: r for r in json.loads((ROOT / "profiles" / "gate_f16r.json").read_text())["results"]}[name]
    d, blob, z = blob_for(name)
    planes = z["planes"]
    assert len(planes) <= batch
    with r_eval(blob, batch, words) as ev:
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)
        assert ev.stats()["saturated"] == 0
    with r_eval(blob, batch, words, dtype="f16") as ev:
        fp, fv = ev.eval(planes)
    p64, v64 = z["policy_f64"], z["value_f64"].reshape(-1)
    er, ef = rms(p - p64), rms(fp - p64)
    print("%s (%d leaves): rms |dlogit| vs f64 f16r %.3g (emulation %.3g), f16 %.3g (emulation %.3g), ratio %.3f (emulation %.3f); max |dlogit| f16r %.3g f16 %.3g; "
          "max |dvalue| f16r %.3g f16 %.3g"
          % (name, len(planes), er, gate["f16r"]["rms_dp_vs_f64"], ef, gate["f16_direct"]["rms_dp_vs_f64"], er / ef,
             gate["f16r"]["rms_dp_vs_f64"] / gate["f16_direct"]["rms_dp_vs_f64"], np.abs(p - p64).max(), np.abs(fp - p64).max(), np.abs(v - v64).max(),
             np.abs(fv - v64).max()))
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert er <= ef


# ---- 6. a leaf's bits depend on the leaf alone ----
def test_a_leafs_bits_do_not_depend_on_its_slot_its_batch_the_lane_or_the_entry_point():
    torch = pytest.importorskip("torch")
    blob, d = chess_net(2, 128), chess_desc(2, 128)
    fill = synth.random_chess_planes(80, 5)
    leaf = synth.random_chess_planes(1, 6)[0]
    legal = np.sort(np.random.default_rng(5).choice(d.moves, size=12, replace=False)).astype(np.uint16)
    f32p = C.POINTER(C.c_float)
    want = want_probs = None
    for max_batch, slots in ((8, (0, 5)), (80, (0, 5, 9, 76, 79))):
        with r_eval(blob, max_batch) as ev:
            assert ev.tower_kernel() == KERNEL
            for slot in slots:
                batch = fill[:max_batch].copy()
                batch[slot] = leaf
                p, v = ev.eval(batch)
                if want is None:
                    want = (p[slot].copy(), v[slot].copy())
                assert same(p[slot], want[0]) and same(v[slot], want[1]), (max_batch, slot)
            # a short batch (3 or 75 leaves), the leaf last
            short = np.concatenate([fill[: max_batch - 6], leaf[None]])
            n = len(short)
            p, v = ev.eval(short)
            assert same(p[-1], want[0]) and same(v[-1], want[1]), (max_batch, "short")
            # apply: the leaf server, blocking
            p, v = np.empty((n, d.moves), dtype=np.float32), np.empty((n,), dtype=np.float32)
            assert ev._lib.cattus_hip_apply(ev._h, np.ascontiguousarray(short).ctypes.data_as(C.POINTER(C.c_uint64)), n, p.ctypes.data_as(f32p), v.ctypes.data_as(f32p)) == 0
            assert same(p[-1], want[0]) and same(v[-1], want[1]), (max_batch, "apply")
            # eval_legal and apply_legal: the leaf's list among others
            idx = np.tile(legal, (n, 1))
            cnt = np.full(n, 12, dtype=np.uint16)
            cnt[0] = 5
            probs, lv = ev.eval_legal(short, idx, cnt)
            if want_probs is None:
                want_probs = probs[-1].copy()
            assert same(probs[-1], want_probs) and same(lv[-1], want[1]), (max_batch, "eval_legal")
            plists, av = ev.apply_legal(short, [legal[: cnt[i]] for i in range(n)])
            assert same(plists[-1], want_probs) and same(av[-1], want[1]), (max_batch, "apply_legal")
            assert abs(float(want_probs.sum()) - 1.0) < 1e-5
            # device buffers, either lane
            dev = torch.device("cuda", 0)
            d_planes = torch.from_numpy(short.copy().view(np.int64)).to(dev)
            for lane in (0, 1):
                pol = torch.zeros((n, d.moves), dtype=torch.float32, device=dev)
                val = torch.zeros((n,), dtype=torch.float32, device=dev)
                ev.eval_device(d_planes.data_ptr(), n, pol.data_ptr(), val.data_ptr(), ev.lane_stream(lane), lane=lane)
                torch.cuda.synchronize()
                assert same(pol[-1].cpu().numpy(), want[0]) and same(val[-1].cpu().numpy(), want[1]), (max_batch, "lane", lane)
            assert ev.stats()["saturated"] == 0


# ---- 7. range ----
def test_copies_beyond_the_f16_range_are_counted_and_the_outputs_stay_finite():
    """The networks of tests/test_hip_parity.py::test_f16x2_range_large_batchnorm_scales: a stem BatchNorm weight of 200 keeps every
    copy inside the f16 range; one of 1e5 sends the stem's beyond 65504: the copies are clamped and counted, the f32 stream keeps its
    values, everything stays finite."""
    d = NetDesc(**CHESS, blocks=2, filters=64, vhc=8, phc=8)
    planes = synth.random_chess_planes(9, 4)
    for scale, saturates in ((200.0, False), (1e5, True)):
        t = seeded_tensors(d, 6)
        t["_conv1._bn.weight"] = t["_conv1._bn.weight"] * np.float32(scale)
        t["_residual_blocks.0._conv1.weight"] = t["_residual_blocks.0._conv1.weight"] * np.float32(1e-3)  # tiny weights too
        with r_eval(pack_tensors(d, t), 16) as ev:
            assert ev.tower_kernel() == KERNEL and ev.stats()["saturated"] == 0
            p, v = ev.eval(planes)
            first = ev.stats()["saturated"]
            p2, v2 = ev.eval(planes)
            second = ev.stats()["saturated"]
        print("stem BatchNorm x %g: saturated %d, then %d" % (scale, first, second))
        assert np.isfinite(p).all() and np.isfinite(v).all()
        assert same(p, p2) and same(v, v2)
        assert second == 2 * first  # the same count on either run; the counter is sticky
        assert (first > 0) == saturates, (scale, first)


# ---- 8. observation ----
def test_points_trace_and_verify_see_the_tower_on_itself():
    blob = chess_net(2, 128)
    planes = synth.random_chess_planes(8, 8)
    with r_eval(blob, 8) as ev:
        P = ev.points()
        assert P == 2 + 2 * 2
        want = ev.eval(planes)
    with r_eval(blob, 8, verify_every=1) as ev:
        p, v = ev.eval(planes)
        assert same(p, want[0]) and same(v, want[1])
        assert ev.verify_stats()["batches"] == 1 and ev.verify_stats()["leaves"] == 8
        taps = []
        for point in range(P):
            x, tp, tv = ev.tap(planes, point, outputs=True)
            assert same(tp, want[0]) and same(tv, want[1]), point  # an observed pass computes what an unobserved one does
            taps.append(x)
        assert all(t.shape == (8, 128, 8, 8) for t in taps[: P - 1]) and taps[P - 1].shape == (8, 8, 8, 8)
        assert all(np.isfinite(t).all() and (t >= 0).all() and t.max() > 0 for t in taps)
        # the middle points are f16 values, the stream points are not
        assert same(np.float16(taps[1]).astype(np.float32), taps[1]) and same(np.float16(taps[3]).astype(np.float32), taps[3])
        assert not same(np.float16(taps[0]).astype(np.float32), taps[0]) and not same(np.float16(taps[2]).astype(np.float32), taps[2])
        rec, rp, rv = ev.trace(planes)
        assert ev.tower_kernel() == KERNEL
        p, v = ev.eval(planes)
        assert same(p, want[0]) and same(v, want[1])
        assert ev.verify_stats()["batches"] == 2 and ev.verify_stats()["leaves"] == 16  # tap and trace are not batches
        assert ev.stats()["saturated"] == 0
    assert same(rp, want[0]) and same(rv, want[1])
    assert rec.shape == (P, 8) and (rec["flags"] == 0).all()
    with r_eval(blob, 8, dtype="f16") as ev:
        frec, _, _ = ev.trace(planes)
    with r_eval(blob, 8, dtype="f32") as ev:
        exact = ev.tap(planes, P - 2)
    ours = np.sqrt(np.mean(np.square(taps[P - 2].astype(np.float64) - exact), axis=(1, 2, 3)))
    assert np.allclose(ours, rec["rms_diff"][P - 2], rtol=1e-3)  # the record is of the tensor tap decodes
    ratio, fratio = rec["rms_diff"][P - 2] / rec["rms_ref"][P - 2], frec["rms_diff"][P - 2] / frec["rms_ref"][P - 2]
    print("rms_diff / rms_ref at the last stream point: f16r mean %.3g max %.3g, f16 mean %.3g max %.3g" % (ratio.mean(), ratio.max(), fratio.mean(), fratio.max()))
    assert ratio.mean() <= fratio.mean()


def test_tap_decodes_a_shifted_stream_to_network_units():
    """Every fourth stream channel made 2^-8 small (helpers.channel_twin, Q8): the tower carries those at 2^8 (stream_shifts) in its f32
    rows, and tap gives network units back.  11-bit operands over two blocks: a relative rms error of 1e-2 is 20 units of 2^-11; a
    missing 2^-t_k would be a factor of 2^8 on the shifted channels, which are looked at on their own as well."""
    d = chess_desc(2, 128)
    e = CHANNEL_PATTERNS["Q8"](d.filters)
    blob = pack_tensors(d, channel_twin(d, seeded_tensors(d, 7), e))
    planes = synth.random_chess_planes(4, 8)
    with r_eval(blob, 4) as ev:
        shifts = ev.stream_shifts()
        P = ev.points()
        stem, last = ev.tap(planes, 0), ev.tap(planes, P - 2)
    with r_eval(blob, 4, dtype="f32") as ev:
        xstem, exact = ev.tap(planes, 0), ev.tap(planes, P - 2)
    small = e < 0
    assert (shifts[small] > 0).all() and (shifts[small] > shifts[~small].max()).all()
    for got, ref in ((stem, xstem), (last, exact)):
        assert rms(got - ref) <= 1e-2 * rms(ref)
        assert rms(got[:, small] - ref[:, small]) <= 1e-2 * rms(ref[:, small])


# ---- 9. calibration ----
def test_calibration_is_accepted_and_a_seeded_net_keeps_its_shifts_and_its_bits():
    """cattus_hip_create_calibrated takes the dtype.  The tower's stream is f32, so it keeps the estimate's shifts and takes the measured
    headroom guard alone (weight_layout.h: calibrated_stream_shifts_f32_stream): a seeded net, whose estimate is right, gives all shifts
    0 and the bits of the uncalibrated evaluator."""
    blob = chess_net(2, 128)
    planes = synth.random_chess_planes(8, 3)
    with r_eval(blob, 8) as ev:
        assert (ev.stream_shifts() == 0).all()
        want = ev.eval(planes)
    with r_eval(blob, 8, calibration=synth.random_chess_planes(16, 12)) as ev:
        assert ev.tower_kernel() == KERNEL
        shift, shifts = ev.stream_shift(), ev.stream_shifts()
        p, v = ev.eval(planes)
        assert ev.stats()["saturated"] == 0
    assert shift == 0 and shifts.shape == (128,) and (shifts == 0).all()
    assert same(p, want[0]) and same(v, want[1])


def test_on_the_hidden_twin_the_calibrated_evaluator_is_at_least_as_close_to_f32():
    """The construction of tests/test_f16w_gpu.py with the scale this tower's range asks for: a network whose stream is 2^-6 of the
    seeded one's carries it at 2^6 by the estimate; every fourth channel is then made 2^16 larger where gamma does not show it
    (test_stream_calibration.hidden_twin), so the estimate still gives those channels the global shift and their f16 copies run at 2^16
    times the seeded size: past 65504 wherever the seeded value is above 1, clamped and counted.  Calibrated on the leaves it evaluates,
    the tower lowers the shift of every channel whose measured largest |value| 2^t exceeds 4096 until it fits -- the estimate's shifts
    guarded, restated here -- and nothing saturates: at least as close to the f32 tower as without."""
    from test_channel_scale_gpu import expected_stream_shifts
    from test_stream_calibration import hidden_twin

    d = chess_desc(2, 128)
    hidden = np.arange(128) % 4 == 1
    tensors = hidden_twin(d, stream_twin(d, seeded_tensors(d, 7), 2.0**-6), np.where(hidden, 16, 0))
    blob = pack_tensors(d, tensors)
    planes = synth.random_chess_planes(16, 3)
    estimate = expected_stream_shifts(d, tensors)
    with r_eval(blob, 16, dtype="f32") as ev:
        _, abs_max = ev.stream_range(planes)
        exact = ev.eval(planes)
    want = estimate.copy()
    for k in range(128):
        while want[k] > 0 and float(abs_max[k]) * 2.0 ** int(want[k]) > 4096.0:
            want[k] -= 1
    with r_eval(blob, 16) as ev:
        assert (ev.stream_shifts() == estimate).all()
        plain = ev.eval(planes)
        plain_sat = ev.stats()["saturated"]
    with r_eval(blob, 16, calibration=planes) as ev:
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


# ---- 10. edges ----
def test_the_forms_the_heads_tail_leaves_and_the_simple_model():
    blob = chess_net(2, 16)  # 64 padded filters: dtype f16 has a resident form here
    planes = synth.random_chess_planes(5, 3)
    outs = {}
    for form in ("auto", "direct", "winograd", "winograd_f4", "direct_splitk"):  # the forms 1 - 4 name forms of the f16x2 tower and are ignored
        with r_eval(blob, 8, tower_form=form) as ev:
            assert ev.tower_kernel() == KERNEL
            outs[form] = ev.eval(planes)
    assert all(same(o[0], outs["auto"][0]) and same(o[1], outs["auto"][1]) for o in outs.values())
    wide_heads = seeded_blob(NetDesc(**CHESS, blocks=1, filters=64, vhc=20, phc=20), 7)
    for label, b, kw in (("resident, 64 filters", blob, {"tower_form": "resident"}), ("resident, 128 filters", chess_net(2, 128), {"tower_form": "resident"}),
                         ("vhc + phc > 32", wide_heads, {})):
        with pytest.raises(CattusHipError) as ei:
            r_eval(b, 8, **kw)
        assert ei.value.status == -2, label  # CATTUS_E_UNSUPPORTED
    with r_eval(blob, 8, tail_leaves=4) as ev:
        assert ev.tower_kernel() == KERNEL and ev.tail_leaves() == 0
        p, v = ev.eval(planes)
        assert ev.tail_batches() == 0
    assert same(p, outs["auto"][0]) and same(v, outs["auto"][1])
    sd = simple_desc(**TTT)
    tplanes = synth.random_ttt_planes(3, 3)
    out = {}
    for dtype in ("f32", "f16r"):
        with r_eval(seeded_blob(sd, 4), 4, dtype=dtype) as ev:
            assert ev.tower_kernel() == "policy_fc_kernel"
            out[dtype] = ev.eval(tplanes)
    assert same(out["f16r"][0], out["f32"][0]) and same(out["f16r"][1], out["f32"][1])
