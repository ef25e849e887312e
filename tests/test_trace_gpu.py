"""Layer-level observation on the GPU: HipEvaluator.tap returns one point of the network in the reference's layout, HipEvaluator.trace holds
every point of an evaluator to the f32 shadow's (include/cattus_hip.h; layouts and the record's rule: cattus_amd/csrc/tap_layout.h, held to
numpy restatements without a GPU by tests/test_tap_layout.py).

Points of a network of B blocks: 0 the stem's output, 2i + 1 block i behind conv1 + bn1 + ReLU, 2i + 2 block i's output, P - 1 = 2B + 1
the two head convs' outputs (value channels first).  `stem0` / `tower0` of the fixtures under tests/golden/ are the reference module's own
activations at points 0 and P - 2 for leaf 0 (oracle/gen_golden.py): until now only the CPU oracle was held to them.
"""

import numpy as np
import pytest

from cattus_amd import synth
from cattus_amd.evaluator import TRACE_RECORD, CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, NetDesc, pack_tensors, seeded_blob, seeded_tensors, simple_desc
from oracle import oracle

from helpers import blob_for, golden_names, load_golden, stream_twin

pytestmark = pytest.mark.gpu

CATTUS_E_INVALID, CATTUS_E_UNSUPPORTED = -1, -2
DEEP = {"chess_20x256"}  # tests/test_oracle_golden.py: the deep tower's looser bound at its last block


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def golden_bounds(name):
    """(rtol, atol) at the stem and at the last block: exactly what test_oracle_golden.py holds the CPU oracle to."""
    return (1e-4, 1e-5), ((2e-3, 2e-4) if name in DEEP else (1e-3, 1e-5))


def words(planes):
    return planes.shape[2]


# ---------------------------------------------------------------------------------------- 1: the f32 tap is the oracle's


@pytest.mark.parametrize("name", golden_names())
def test_f32_tap_equals_the_cpu_oracle_to_the_bit_and_holds_the_reference_made_activations(name):
    d, blob, z = blob_for(name)
    leaf = z["planes"][:1]
    _, _, stem, tower = oracle.OracleNet(blob).forward_debug(leaf[0])
    with HipEvaluator(blob, batch_size=4, plane_words=words(leaf), dtype="f32", switches={}) as ev:
        P = ev.points()
        assert P == 2 + 2 * d.blocks
        want_p, want_v = ev.eval(leaf)
        got_stem, p0, v0 = ev.tap(leaf, 0, outputs=True)
        got_tower, p1, v1 = ev.tap(leaf, P - 2, outputs=True)
    assert got_stem.shape == (1, d.filters, d.board, d.board) and same_bits(got_stem[0], stem), np.abs(got_stem[0] - stem).max()
    assert same_bits(got_tower[0], tower), np.abs(got_tower[0] - tower).max()
    (rs, as_), (rt, at) = golden_bounds(name)
    np.testing.assert_allclose(got_stem[0], z["stem0"].reshape(stem.shape), rtol=rs, atol=as_)
    np.testing.assert_allclose(got_tower[0], z["tower0"].reshape(tower.shape), rtol=rt, atol=at)
    for p, v in ((p0, v0), (p1, v1)):
        assert same_bits(p, want_p) and same_bits(v, want_v)


# ---------------------------------------------------------------------------------------- 2: two independent layouts


@pytest.mark.parametrize("name", ["chess_7x16", "hex11_2x8", "ttt_5x8", "hex7_6x64"])
def test_every_point_of_the_mfma_tower_equals_the_generic_tower(name):
    """NHWC rows and fragment-ordered heads through the transposing kernel against NCHW through the gather: the same bits at all P points."""
    d, blob, z = blob_for(name)
    planes = z["planes"]
    with HipEvaluator(blob, batch_size=len(planes), plane_words=words(planes), dtype="f32", switches={}) as mfma, \
            HipEvaluator(blob, batch_size=len(planes), plane_words=words(planes), dtype="f32", switches={"CATTUS_FORCE_GENERIC": "1"}) as generic:
        assert mfma.tower_kernel() == "conv3x3_mfma_v2_kernel" and generic.tower_kernel() == "conv3x3_generic_kernel"
        for point in range(mfma.points()):
            a, b = mfma.tap(planes, point), generic.tap(planes, point)
            channels = d.filters if point + 1 < mfma.points() else d.vhc + d.phc
            assert a.shape == (len(planes), channels, d.board, d.board)
            assert same_bits(a, b), (point, np.abs(a - b).max())
            assert np.isfinite(a).all() and (a >= 0).all() and a.any()  # behind a ReLU, and something is there


# ---------------------------------------------------------------------------------------- 3, 5: every plan's twin; trace is two taps

# name: (fixture, dtype, batch size (None: the leaves'), switches, the product kernel).  chess_7x16's 16 filters are padded to 64, so
# bf16 and f16x2 would take the resident plans by themselves: CATTUS_TOWER64=0 is what makes them the PerLayer plan (f16 has no resident one).
PLANS = {
    "per_layer_bf16": ("chess_7x16", "bf16", None, {"CATTUS_TOWER64": "0"}, "conv3x3_mfma_v2_kernel"),
    "per_layer_f16": ("chess_7x16", "f16", None, {}, "conv3x3_mfma_v2_kernel"),
    "per_layer_f16x2": ("chess_7x16", "f16x2", None, {"CATTUS_TOWER64": "0"}, "conv3x3_splitw_kernel"),
    "resident64": ("hex7_6x64", "bf16", None, {}, "tower64_lds_kernel"),
    "resident64_split": ("hex7_6x64", "f16x2", None, {}, "tower64_split_kernel"),
    "wino4_one_launch": ("chess_4x128", "f16x2", 160, {}, "tower_wino4_kernel"),
    "wino16": ("chess_4x128", "f16x2", 160, {"CATTUS_WINO_KERNEL": "k16"}, "conv3x3_wino_kernel"),
}


def plan_case(plan):
    name, dtype, batch, switches, kernel = PLANS[plan]
    d, blob, z = blob_for(name)
    planes = z["planes"]
    if batch:  # a batch that is no multiple of the Winograd tower's four-board groups
        planes = np.concatenate([planes, synth.random_chess_planes(41, 5)])[:41]
    ev = HipEvaluator(blob, batch_size=batch or len(planes), plane_words=words(planes), dtype=dtype, switches=switches)
    return d, blob, planes, ev, kernel


@pytest.mark.parametrize("plan", list(PLANS))
def test_the_per_layer_twin_of_every_plan_is_the_plan(plan):
    """tap and trace run a resident or one-launch tower on its per-layer launches: the outputs they return are eval's to the bit, the
    evaluator still names and runs its product kernel afterwards, and neither call is a batch."""
    d, blob, planes, ev, kernel = plan_case(plan)
    with ev:
        assert ev.tower_kernel() == kernel
        want_p, want_v = ev.eval(planes)
        before = ev.stats()
        for point in range(ev.points()):
            _, p, v = ev.tap(planes, point, outputs=True)
            assert same_bits(p, want_p) and same_bits(v, want_v), point
        rec, p, v = ev.trace(planes)
        assert rec.shape == (ev.points(), len(planes)) and same_bits(p, want_p) and same_bits(v, want_v)
        after = ev.stats()
        for key in ("batches", "positions", "full_batches", "run_seconds_total"):
            assert after[key] == before[key], key
        assert ev.verify_stats()["every"] == 0 and ev.verify_stats()["leaves"] == 0  # the shadow exists now; no ticket was taken
        again_p, again_v = ev.eval(planes)
        assert same_bits(again_p, want_p) and same_bits(again_v, want_v)
        assert ev.tower_kernel() == kernel and ev.stats()["batches"] == before["batches"] + 1


def records_from_taps(x, ref):
    """[n] records from two taps [n, C, S, S] in float64 numpy: the rule of cattus_trace_record."""
    n = len(x)
    x, ref = x.reshape(n, -1), ref.reshape(n, -1)
    out = np.zeros(n, dtype=TRACE_RECORD)
    with np.errstate(all="ignore"):
        d = x.astype(np.float64) - ref.astype(np.float64)
        diff = np.abs(d).astype(np.float32)
        diff = np.where(np.isnan(diff), np.float32(-1), diff)
        positive = diff.max(axis=1) > 0
        at = np.where(positive, diff.argmax(axis=1), 0)
        rows = np.arange(n)
        out["max_diff"] = np.where(positive, diff[rows, at], np.float32(0))
        out["at"], out["x"], out["ref"] = at, x[rows, at], ref[rows, at]
        out["rms_diff"] = np.sqrt((d * d).sum(axis=1) / d.shape[1])
        out["rms_ref"] = np.sqrt((ref.astype(np.float64) ** 2).sum(axis=1) / d.shape[1])
        out["flags"] = ~(np.isfinite(x).all(axis=1) & np.isfinite(ref).all(axis=1))
    return out


@pytest.mark.parametrize("plan", list(PLANS))
def test_trace_is_what_two_taps_say(plan):
    """At every point the records equal what tap of this evaluator and tap of a separate dtype f32 evaluator of the same blob give: max_diff,
    at, x, ref and flags exactly, the two rms within 1e-6 relative of float64 numpy (the kernel's double sums associate differently: 1e-6
    is some 10^9 ulp of headroom over that, and far below any effect of interest).  A second trace returns the same bytes."""
    d, blob, planes, ev, _ = plan_case(plan)
    with ev, HipEvaluator(blob, batch_size=len(planes), plane_words=words(planes), dtype="f32", switches={}) as exact:
        rec, _, _ = ev.trace(planes)
        rec2, _, _ = ev.trace(planes)
        assert rec.tobytes() == rec2.tobytes()
        for point in range(ev.points()):
            want = records_from_taps(ev.tap(planes, point), exact.tap(planes, point))
            got = rec[point]
            for field in ("max_diff", "x", "ref"):
                assert (got[field].view(np.uint32) == want[field].view(np.uint32)).all(), (point, field, got[:3], want[:3])
            assert (got["at"] == want["at"]).all() and (got["flags"] == want["flags"]).all() and (got["reserved"] == 0).all(), point
            for field in ("rms_diff", "rms_ref"):
                assert np.allclose(got[field], want[field], rtol=1e-6, atol=0), (point, field, got[field], want[field])
            assert (got["rms_ref"] > 0).all()
        assert (rec["max_diff"] > 0).any()  # a reduced-precision tower does differ from the exact one somewhere


# ---------------------------------------------------------------------------------------- 4: stale padding


@pytest.mark.parametrize("dtype", ["f16x2", "bf16", "f32"])
def test_stale_rows_boards_and_channels_never_reach_a_result(dtype):
    """Batch size 8 on a 7x7 board (15 unused slots per board): after a full batch of other leaves, tap and trace of 3 leaves give what a
    fresh evaluator gives that has seen only those 3."""
    d, blob, _ = blob_for("hex7_6x64")
    planes = synth.random_hex_planes(11, 7, 3)
    used, fresh = (HipEvaluator(blob, batch_size=8, plane_words=words(planes), dtype=dtype, switches={}) for _ in range(2))
    with used, fresh:
        used.eval(planes[:8])
        if dtype != "f32":
            used.trace(planes[:8])  # fills the shadow's lanes too
        for point in range(used.points()):
            assert same_bits(used.tap(planes[8:], point), fresh.tap(planes[8:], point)), point
        if dtype != "f32":
            assert used.trace(planes[8:])[0].tobytes() == fresh.trace(planes[8:])[0].tobytes()


# ---------------------------------------------------------------------------------------- 6: shifts are divided out

# A stored f16x2 pair resolves 2^-22 of its value; 400 x that is the issue's bound at the stream points (a forgotten shift is off by 2^7).
# For the 11-bit f16 and the 8-bit bf16 towers the same 400 x their resolution, and never more than 7 (the reading of the issue's "bound
# 7" that asks the most of the code: a forgotten shift gives a ratio of 127 or, divided the wrong way, of 1 - 2^-14).
SHIFT_BOUNDS = {"f16x2": 1e-4, "f16": min(7.0, 400 * 2.0**-11), "bf16": min(7.0, 400 * 2.0**-8)}


@pytest.mark.parametrize("dtype", ["f16x2", "f16", "bf16"])
def test_stream_shifts_are_divided_out_at_the_stream_points(dtype):
    d, seed, _ = load_golden("chess_2x64")
    blob = pack_tensors(d, stream_twin(d, seeded_tensors(d, seed), 2.0**-7))
    planes = synth.random_chess_planes(6, 4)
    with HipEvaluator(blob, batch_size=8, plane_words=1, dtype=dtype, switches={}) as ev:
        if dtype != "bf16":
            assert (ev.stream_shifts() != 0).any()  # (bf16 carries its stream unshifted: nothing to forget)
        rec, _, _ = ev.trace(planes)
        ratio = rec["rms_diff"].astype(np.float64) / rec["rms_ref"]
        print(dtype, "rms_diff / rms_ref per point (max over leaves):", ratio.max(axis=1))
        for point in range(0, ev.points() - 1, 2):
            assert (ratio[point] <= SHIFT_BOUNDS[dtype]).all(), (point, ratio[point])
        assert ev.stats()["saturated"] == 0


# ---------------------------------------------------------------------------------------- 7: against the reference-made activations

# max |tap - fixture| / max |fixture| at (point 0, point P - 2) for leaf 0, measured on an MI355X against stem0 / tower0 of the fixture --
# reference-made data, never another run of the code under test; the test allows twice that (the rule of BF16_MEASURED in
# test_hip_parity.py).  The measured values are the ones written here.
TAP_MEASURED = {
    "bf16": {
        "chess_1x1": (3.34e-3, 6.58e-3), "chess_20x256": (3.38e-3, 9.58e-3), "chess_2x64": (3.91e-3, 5.33e-3), "chess_4x128": (2.40e-3, 7.75e-3),
        "chess_7x16": (4.01e-3, 1.44e-2), "hex11_1x1": (3.37e-3, 3.85e-3), "hex11_2x8": (3.79e-3, 5.88e-3), "hex4_7x16": (3.22e-3, 1.05e-2),
        "hex7_6x64": (2.36e-3, 5.40e-3), "ttt_1x1": (0.0, 2.79e-4), "ttt_2x64": (2.45e-3, 4.13e-3), "ttt_5x8": (2.21e-3, 8.19e-3),
    },
    "f16": {
        "chess_1x1": (5.50e-4, 6.61e-4), "chess_20x256": (3.69e-4, 1.31e-3), "chess_2x64": (4.02e-4, 7.71e-4), "chess_4x128": (3.49e-4, 7.16e-4),
        "chess_7x16": (4.64e-4, 1.25e-3), "hex11_1x1": (1.66e-4, 1.58e-4), "hex11_2x8": (3.70e-4, 4.73e-4), "hex4_7x16": (3.35e-4, 1.06e-3),
        "hex7_6x64": (3.57e-4, 8.60e-4), "ttt_1x1": (0.0, 7.07e-8), "ttt_2x64": (3.66e-4, 4.39e-4), "ttt_5x8": (3.87e-4, 6.36e-4),
    },
}  # (ttt_1x1's stem output for leaf 0 is all zeros in the fixture, and every tower returns zeros: 0 / 0 counts as 0)
# f16x2 is held to the oracle's own assert_allclose bounds (golden_bounds).  Measured on an MI355X, every fixture holds them with room:
# the worst |d| / (atol + rtol |ref|) is 0.014 at the stem (chess_4x128) and 0.026 at the last block (chess_4x128), so nothing is listed
# here.  (A fixture that needed more would get the factor it is allowed -- 2 x the measured excess -- with the measured figure beside it.)
F16X2_EXCESS = {}


def tap_errors(name, dtype):
    """((max |d| / max |ref|, worst |d| / (atol + rtol |ref|)) at point 0, the same at point P - 2) of leaf 0 against the fixture."""
    d, blob, z = blob_for(name)
    leaf = z["planes"][:1]
    with HipEvaluator(blob, batch_size=4, plane_words=words(leaf), dtype=dtype, switches={}) as ev:
        taps = ev.tap(leaf, 0)[0], ev.tap(leaf, ev.points() - 2)[0]
    out = []
    for got, ref, (rtol, atol) in zip(taps, (z["stem0"], z["tower0"]), golden_bounds(name)):
        ref = ref.reshape(got.shape).astype(np.float64)
        diff = np.abs(got.astype(np.float64) - ref)
        rel = float(diff.max() / np.abs(ref).max()) if diff.max() > 0 else 0.0  # (an all-zero tensor met exactly: 0, not 0 / 0)
        out.append((rel, float((diff / (atol + rtol * np.abs(ref))).max())))
    return out


@pytest.mark.parametrize("name", golden_names())
def test_f16x2_intermediates_hold_the_oracles_bounds_on_the_reference_made_activations(name):
    errors = tap_errors(name, "f16x2")
    print(name, "f16x2 (relative to max |ref|, in units of the allclose bound) stem, tower:", errors)
    for (_, in_bound), allowed in zip(errors, F16X2_EXCESS.get(name, (1.0, 1.0))):
        assert in_bound <= allowed, (name, errors)


@pytest.mark.parametrize("name", golden_names())
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_bf16_and_f16_intermediates_stay_within_twice_their_measured_error(dtype, name):
    errors = tap_errors(name, dtype)
    print(name, dtype, "max |d| / max |ref| at stem, tower:", errors[0][0], errors[1][0])
    for (rel, _), measured in zip(errors, TAP_MEASURED[dtype][name]):
        assert rel <= 2 * measured, (name, dtype, errors)


# ---------------------------------------------------------------------------------------- 8: localisation


def test_trace_names_the_block_where_the_f16_range_is_left():
    """Block 1's _bn2 gamma x 1e6 pushes that block's output out of the f16 range: the trace is clean up to point 3 and broken from
    point 4 on, and `saturated` says why.  (On the CPU oracle the two-block variant of this network has 22-50 % of a leaf's elements
    over 65504 there, and a clamp at 65504 then costs an rms ratio >= 0.59; the preconditions below guard the three-block shape.)"""
    d = NetDesc(**CHESS, blocks=3, filters=64, vhc=8, phc=8)
    tensors = seeded_tensors(d, 6)
    tensors["_residual_blocks.1._bn2.weight"] = (tensors["_residual_blocks.1._bn2.weight"] * np.float32(1e6)).astype(np.float32)
    blob = pack_tensors(d, tensors)
    planes = synth.random_chess_planes(9, 8)
    with HipEvaluator(blob, batch_size=9, plane_words=1, dtype="f32", switches={}) as exact:
        over = [(exact.tap(planes, point) > 65504).reshape(len(planes), -1).mean(axis=1) for point in range(5)]
    print("share of elements over 65504 per leaf at point 4:", over[4])
    assert (over[4] >= 0.2).all() and all((o == 0).all() for o in over[:4])
    with HipEvaluator(blob, batch_size=9, plane_words=1, dtype="f16x2", switches={}) as ev:
        assert ev.tower_kernel() == "tower64_split_kernel"  # Resident64Split: the trace runs its per-layer twin
        rec, _, _ = ev.trace(planes)
        ratio = rec["rms_diff"].astype(np.float64) / rec["rms_ref"]
        print("rms_diff / rms_ref per point (max over leaves):", ratio.max(axis=1))
        assert (ratio[:4] <= 1e-4).all(), ratio[:4].max(axis=1)
        assert (ratio[4] >= 0.1).all(), ratio[4]
        assert ev.stats()["saturated"] > 0


# ---------------------------------------------------------------------------------------- 9: refusals


def test_refusals():
    d = NetDesc(**CHESS, blocks=1, filters=64, vhc=8, phc=8)
    blob = seeded_blob(d, 27)
    planes = synth.random_chess_planes(5, 2)

    def status(call):
        with pytest.raises(CattusHipError) as err:
            call()
        return err.value.status

    with HipEvaluator(blob, batch_size=4, plane_words=1, dtype="f32", switches={}) as ev:
        assert status(lambda: ev.trace(planes[:2])) == CATTUS_E_UNSUPPORTED  # its shadow would be itself
        assert ev.tap(planes[:2], 0).shape == (2, 64, 8, 8)  # tap is not refused
    sd = simple_desc(3, 3, 9)
    with HipEvaluator(seeded_blob(sd, 2), batch_size=4, plane_words=1, dtype="f16x2", switches={}) as ev:
        ttt = synth.random_ttt_planes(2, 1)
        assert status(lambda: ev.tap(ttt, 0)) == CATTUS_E_UNSUPPORTED
        assert status(lambda: ev.trace(ttt)) == CATTUS_E_UNSUPPORTED
        assert status(ev.points) == CATTUS_E_UNSUPPORTED
    other_shape = NetDesc(**CHESS, blocks=2, filters=64, vhc=8, phc=8)
    with HipEvaluator(blob, batch_size=4, plane_words=1, dtype="f16x2", switches={}) as ev:
        P = ev.points()
        assert P == 4
        for wrong in (seeded_blob(d, 28), seeded_blob(other_shape, 27)):
            assert status(lambda: ev.trace(planes[:2], blob=wrong)) == CATTUS_E_INVALID
        assert status(lambda: ev.tap(planes[:2], P)) == CATTUS_E_INVALID
        assert status(lambda: ev.trace(planes[:2], points=P - 1)) == CATTUS_E_INVALID
        for bad in (planes[:0], planes[:5]):  # n = 0 and n = max_batch + 1
            assert status(lambda: ev.tap(bad, 0)) == CATTUS_E_INVALID
            assert status(lambda: ev.trace(bad)) == CATTUS_E_INVALID
        assert ev.verify_stats()["leaves"] == 0 and ev.stats()["batches"] == 0
        rec, _, _ = ev.trace(planes[:4])  # and the right call is taken
        assert rec.shape == (P, 4)
