"""Short batches of the Winograd F(2x2,3x3) tower on the small-tile kernel (cattus_eval_config.tail_leaves, conv3x3_wino4s_kernel).

The kernel takes 2 boards x 32 output channels per workgroup where tower_wino4_kernel takes 4 x 64, and computes the same arithmetic
in the same order: every logit and value of an evaluator with tail_leaves > 0 equals, BIT FOR BIT, what the default evaluator gives
the same leaf -- whatever the batch, the entry point, the lane, the plan's own kernel (k4 / k16) or the buffer plan.  Where the field
does not apply it is ignored and says so."""

import ctypes as C
import functools

import numpy as np
import pytest

from cattus_amd import synth
from cattus_amd.evaluator import CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, NetDesc, pack_tensors, seeded_blob, seeded_tensors

from helpers import blob_for, outputs_equal_ref_tol

pytestmark = pytest.mark.gpu

NETS = [(1, 128), (2, 192), (2, 256)]  # 4, 6 and 8 cout blocks / input chunks; one block and two (the in-place skip twice)
TAIL = 64
PLANES = synth.random_chess_planes(256, 23)


@functools.lru_cache(maxsize=None)
def net(blocks, filters):
    return seeded_blob(NetDesc(**CHESS, blocks=blocks, filters=filters, vhc=8, phc=8), 41)


def wino(blob, max_batch=256, tail=0, form="winograd", switches=None, **kw):
    return HipEvaluator(blob, batch_size=max_batch, plane_words=1, dtype="f16x2", tower_form=form, switches=switches or {}, tail_leaves=tail, **kw)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@functools.lru_cache(maxsize=None)
def reference(blocks, filters):
    """The default evaluator's logits and values of all 256 leaves, as batches of 256: what every leaf must get everywhere."""
    with wino(net(blocks, filters)) as ev:
        assert ev.tail_leaves() == 0 and ev.tower_kernel() == "tower_wino4_kernel"
        out = ev.eval(PLANES)
        assert ev.tail_batches() == 0 and ev.stats()["saturated"] == 0
    return out


@pytest.mark.parametrize("shape", NETS)
def test_short_batches_have_the_default_evaluators_bits(shape):
    """n = 1: a lone board in a pair; 2: a full pair; 3: an odd count; 4, 5: with padded boards; 17: bpad 20, no multiple of 8; 64: the
    full short grid.  Two evaluators side by side, the default one and one with tail_leaves = 64."""
    blob = net(*shape)
    with wino(blob) as dflt, wino(blob, tail=TAIL) as ev:
        assert ev.tail_leaves() == TAIL and dflt.tail_leaves() == 0
        assert ev.tower_kernel() == "tower_wino4_kernel" and dflt.tower_kernel() == "tower_wino4_kernel"
        for n in (1, 2, 3, 4, 5, 17, 64):
            before = ev.tail_batches()
            want, got = dflt.eval(PLANES[:n]), ev.eval(PLANES[:n])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (shape, n, np.abs(got[0] - want[0]).max())
            assert ev.tail_batches() == before + 1, n
        assert dflt.tail_batches() == 0
        assert ev.stats()["saturated"] == 0 and dflt.stats()["saturated"] == 0


@pytest.mark.parametrize("shape", NETS)
def test_above_the_threshold_nothing_changes(shape):
    want = reference(*shape)
    with wino(net(*shape), tail=TAIL) as ev:
        for n in (65, 256):
            got = ev.eval(PLANES[:n])
            assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), n
        assert ev.tail_batches() == 0


def test_every_entry_point_and_both_lanes():
    torch = pytest.importorskip("torch")
    shape, n = (2, 192), 9
    blob, want = net(*shape), reference(*shape)
    leaves = PLANES[:n]
    want = (want[0][:n], want[1][:n])
    rng = np.random.default_rng(5)
    legal_idx = np.stack([rng.choice(1880, size=40, replace=False) for _ in range(n)]).astype(np.uint16)
    legal_count = rng.integers(1, 41, size=n).astype(np.uint16)
    with wino(blob) as dflt:
        want_legal = dflt.eval_legal(leaves, legal_idx, legal_count)
    with wino(blob, tail=TAIL) as ev:
        assert same(ev.eval(leaves), want)
        # the leaf server
        p, v = np.empty((n, 1880), dtype=np.float32), np.empty((n,), dtype=np.float32)
        f32p = C.POINTER(C.c_float)
        assert ev._lib.cattus_hip_apply(ev._h, leaves.ctypes.data_as(C.POINTER(C.c_uint64)), n, p.ctypes.data_as(f32p), v.ctypes.data_as(f32p)) == 0
        assert same((p, v), want)
        got_legal = ev.eval_legal(leaves, legal_idx, legal_count)
        assert same(got_legal, want_legal)
        # device buffers, either lane
        dev = torch.device("cuda", 0)
        d_planes = torch.from_numpy(leaves.view(np.int64)).to(dev)
        for lane in (0, 1, 0, 1):
            before = ev.tail_batches()
            pol = torch.zeros((n, 1880), dtype=torch.float32, device=dev)
            val = torch.zeros((n,), dtype=torch.float32, device=dev)
            ev.eval_device(d_planes.data_ptr(), n, pol.data_ptr(), val.data_ptr(), ev.lane_stream(lane), lane=lane)
            torch.cuda.synchronize()
            assert same((pol.cpu().numpy(), val.cpu().numpy()), want), lane
            assert ev.tail_batches() == before + 1
        assert ev.tail_batches() >= 7


def test_a_leafs_bits_depend_on_nothing_but_the_leaf():
    shape = (2, 256)
    leaf = PLANES[200]
    want = reference(*shape)
    want = (want[0][200], want[1][200])
    with wino(net(*shape), tail=TAIL) as ev:
        for size, slots in ((1, (0,)), (3, (0, 1, 2)), (64, (0, 1, 2, 63)), (200, (70,))):
            for slot in slots:
                batch = PLANES[:size].copy()
                batch[slot] = leaf
                before = ev.tail_batches()
                p, v = ev.eval(batch)
                assert p[slot].shape == (1880,)
                assert np.array_equal(p[slot], want[0]) and v[slot] == want[1], (size, slot)
                assert ev.tail_batches() == before + (1 if size <= TAIL else 0)


def test_against_the_other_kernels_and_buffer_plans():
    shape = (2, 256)
    want = reference(*shape)
    for switches in ({"CATTUS_WINO_KERNEL": "k16"}, {"CATTUS_WINO_INPLACE": "0"}, {"CATTUS_ARENA": "0"}, {"CATTUS_WINO_INPLACE": "0", "CATTUS_ARENA": "0"}):
        with wino(net(*shape), tail=TAIL, switches=switches) as ev:
            assert ev.tail_leaves() == TAIL
            if "CATTUS_WINO_KERNEL" in switches:
                assert ev.tower_kernel() == "conv3x3_wino_kernel"
            for n in (5, 64):
                got = ev.eval(PLANES[:n])
                assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), (switches, n)
            assert ev.tail_batches() == 2


def test_reference_made_fixture_is_a_short_batch():
    d, blob, z = blob_for("chess_4x128")
    planes = z["planes"]
    assert len(planes) == 64
    with wino(blob) as dflt, wino(blob, tail=TAIL) as ev:
        want, got = dflt.eval(planes), ev.eval(planes)
        assert ev.tail_batches() == 1 and ev.stats()["saturated"] == 0
    assert outputs_equal_ref_tol(got[0], got[1], z["policy"], z["value"])
    assert same(got, want)


def test_range_is_counted_on_the_short_path_as_on_the_default_path():
    """A stem BatchNorm scale of 200 stays inside the Winograd form's range, one of 1e5 leaves it (test_hip_parity.py's
    test_f16x2_range_large_batchnorm_scales, on a network wide enough for this form): `saturated` says so on either path.  The counts
    are per thread that wrote the cap and depend on the partition; they are not compared."""
    d = NetDesc(**CHESS, blocks=2, filters=128, vhc=8, phc=8)
    planes = synth.random_chess_planes(9, 4)
    for scale, clamps in ((200.0, False), (1e5, True)):
        t = seeded_tensors(d, 6)
        t["_conv1._bn.weight"] = t["_conv1._bn.weight"] * np.float32(scale)
        t["_residual_blocks.0._conv1.weight"] = t["_residual_blocks.0._conv1.weight"] * np.float32(1e-3)
        blob = pack_tensors(d, t)
        sat = {}
        for tail in (0, TAIL):
            with wino(blob, tail=tail) as ev:
                p, v = ev.eval(planes)
                sat[tail] = ev.stats()["saturated"]
                assert ev.tail_batches() == (1 if tail else 0)
            assert np.isfinite(p).all() and np.isfinite(v).all()
        assert (sat[0] > 0) == clamps and (sat[TAIL] > 0) == (sat[0] > 0), (scale, sat)


def test_verification_and_observation_ride_along():
    shape, n = (2, 192), 17
    blob, want = net(*shape), reference(*shape)
    with wino(blob, tail=TAIL, verify_every=1) as ev:
        got = ev.eval(PLANES[:n])
        vs = ev.verify_stats()
        assert vs["batches"] == 1 and vs["leaves"] == n and vs["leaves_outside"] == 0, vs
        assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n])
        assert ev.tail_batches() == 1
    with wino(blob) as dflt, wino(blob, tail=TAIL) as ev:
        point = ev.points() - 2  # the last stream point: the tower's output
        a, pa, va = ev.tap(PLANES[:n], point, outputs=True)
        b, pb, vb = dflt.tap(PLANES[:n], point, outputs=True)
        assert np.array_equal(a, b) and np.array_equal(pa, pb) and np.array_equal(va, vb)
        assert np.array_equal(pa, want[0][:n])
        assert ev.tail_batches() == 0  # an observed pass runs the plan's per-layer twin, as before


def test_where_it_does_not_apply():
    shape = (2, 256)
    blob, want = net(*shape), reference(*shape)
    leaves = PLANES[:33]
    # the direct plan (AUTO up to 128 leaves), f32, and the F(4x4) form: the field is ignored
    for kw in (dict(max_batch=64, form="auto"), dict(form="winograd_f4")):
        with wino(blob, **kw) as plain, wino(blob, tail=33, **kw) as ev:
            assert ev.tail_leaves() == 0 and ev.tower_kernel() == plain.tower_kernel() != "tower_wino4_kernel"
            assert same(ev.eval(leaves), plain.eval(leaves))
            assert ev.tail_batches() == 0
    with HipEvaluator(blob, batch_size=256, plane_words=1, dtype="f32") as plain, \
            HipEvaluator(blob, batch_size=256, plane_words=1, dtype="f32", tail_leaves=33) as ev:
        assert ev.tail_leaves() == 0
        assert same(ev.eval(leaves), plain.eval(leaves))
        assert ev.tail_batches() == 0
    # more than max_batch
    with pytest.raises(CattusHipError) as err:
        wino(blob, max_batch=256, tail=300)
    assert err.value.status == -1  # CATTUS_E_INVALID
    # an evaluator all of whose batches are short
    with wino(blob, max_batch=64, tail=64) as ev:
        assert ev.tail_leaves() == 64
        for n in (64, 7):
            got = ev.eval(PLANES[:n])
            assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n]), n
        assert ev.tail_batches() == 2
