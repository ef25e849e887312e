"""tower_form="resident" on the device: the single-term f16 tower of a network with at most 64 filters in ONE LDS-resident launch
(tower64_lds_kernel<_Float16, ...>), held bit for bit to the tower it is another way of launching -- dtype f16 with tower_form "auto",
1 + 2 * blocks launches of conv3x3_mfma_v2_kernel<_Float16>.  On the parent commit form 5 is CATTUS_E_INVALID and every test here fails.

Cases: the smallest shapes that reach each instantiation of the kernel (seeded blobs, vhc = phc = 4):

  a    hex7   2 blocks x 64 filters   5 leaves                      CH = 4, one barrier per layer (49 pixels)
  a'   hex7   2 x 64                  5          CATTUS_T64_LS=0    CH = 4, three barriers per layer, under 64 pixels
  b    chess  2 x 16                  9                             CH = 4, padded channels, all 64 pixel slots live
  c    chess  2 x 16                  9          CATTUS_T64_CH=2    CH = 2 on 64-slot boards
  c'   chess  1 x 16                  260                           CH = 2 chosen by the grid (more than 256 boards)
  d    hex11  1 x 8                   3                             128-slot boards, two plane words
  e    ttt    0 x 8                   3                             the stem is the last layer

The AUTO evaluator's outputs of a case are computed once, shared, and never written to.  A diagnostic switch of a case goes to both
evaluators (the per-layer tower reads neither of the two)."""

import ctypes as C
import functools

import numpy as np
import pytest

from cattus_amd import evaluator, synth
from cattus_amd.evaluator import CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, TTT, NetDesc, hex_game, pack_tensors, seeded_blob, seeded_tensors, simple_desc

from helpers import stream_twin

pytestmark = pytest.mark.gpu

RESIDENT, PER_LAYER, SPLIT = "tower64_lds_kernel", "conv3x3_mfma_v2_kernel", "tower64_split_kernel"

# name: (game, blocks, filters, n, max_batch, switches)
CASES = {
    "a": ("hex7", 2, 64, 5, 8, {}),
    "a_no_ls": ("hex7", 2, 64, 5, 8, {"CATTUS_T64_LS": "0"}),
    "b": ("chess", 2, 16, 9, 12, {}),
    "c": ("chess", 2, 16, 9, 12, {"CATTUS_T64_CH": "2"}),
    "c_grid": ("chess", 1, 16, 260, 260, {}),
    "d": ("hex11", 1, 8, 3, 4, {}),
    "e": ("ttt", 0, 8, 3, 4, {}),
}
GAMES = {"hex7": hex_game(7), "hex11": hex_game(11), "chess": CHESS, "ttt": TTT}


def desc_of(case):
    game, blocks, filters = CASES[case][:3]
    return NetDesc(**GAMES[game], blocks=blocks, filters=filters, vhc=4, phc=4)


@functools.lru_cache(maxsize=None)
def planes_of(game, n, seed):
    if game == "chess":
        p = synth.random_chess_planes(n, seed)
    elif game == "ttt":
        p = synth.random_ttt_planes(n, seed)
    else:
        p = synth.random_hex_planes(n, int(game[3:]), seed)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def blob_of(case):
    return seeded_blob(desc_of(case), 11)


def other_n(case):
    """a batch of another size on the same evaluator: two leaves fewer, or (a case of 3) one more"""
    n, max_batch = CASES[case][3:5]
    return n - 2 if n > 3 else max_batch


def make(case, form, dtype="f16", blob=None, **kw):
    game, _, _, _, max_batch, switches = CASES[case]
    kw.setdefault("switches", dict(switches))
    return HipEvaluator(blob_of(case) if blob is None else blob, max_batch, 2 if game.startswith("hex") else 1, dtype=dtype, tower_form=form, **kw)


@functools.lru_cache(maxsize=None)
def auto_outputs(case):
    """dtype f16, tower_form auto: (logits, values) on the case's n leaves and on its other batch, the kernel and its launches per pass"""
    game, blocks, _, n, _, _ = CASES[case]
    with make(case, "auto") as ev:
        kernel, launches = ev.tower_kernel(), ev.time_tower(n, 1)[1]
        first = ev.eval(planes_of(game, n, 3))
        second = ev.eval(planes_of(game, other_n(case), 4))
        sat = ev.stats()["saturated"]
    for a in (*first, *second):
        a.setflags(write=False)
    assert kernel == PER_LAYER and launches == 1 + 2 * blocks and sat == 0
    return first, second


def same(got, want):
    return all(np.array_equal(np.asarray(g).view(np.uint32), np.asarray(w).view(np.uint32)) for g, w in zip(got, want))


# ---- 1. bit identity, on every instantiation ----
@pytest.mark.parametrize("case", sorted(CASES))
def test_resident_f16_equals_the_per_layer_f16_tower_bit_for_bit(case):
    game, blocks, _, n, _, _ = CASES[case]
    first, second = auto_outputs(case)
    assert np.isfinite(first[0]).all() and np.abs(first[0]).max() > 0
    planes, planes2 = planes_of(game, n, 3), planes_of(game, other_n(case), 4)
    with make(case, "resident") as ev:
        assert ev.tower_kernel() == RESIDENT
        assert same(ev.eval(planes), first), "a fresh evaluator"
        assert ev.time_tower(n, 1)[1] == 1
        for _ in range(3):
            got = ev.eval(planes)
        assert same(got, first), "after three passes"
        assert same(ev.eval(planes2), second), "a batch of another size"
        assert same(ev.eval(planes), first), "behind a batch of another size"
        assert ev.stats()["saturated"] == 0


# ---- 2. every entry point ----
def test_every_entry_point_returns_the_bits_of_eval():
    torch = pytest.importorskip("torch")
    game, _, _, n, _, _ = CASES["a"]
    d = desc_of("a")
    planes = planes_of(game, n, 3)
    want = auto_outputs("a")[0]
    rng = np.random.default_rng(5)
    legal_idx = np.stack([rng.choice(d.moves, size=12, replace=False) for _ in range(n)]).astype(np.uint16)
    legal_count = rng.integers(1, 13, size=n).astype(np.uint16)
    with make("a", "auto") as ev:
        want_legal = ev.eval_legal(planes, legal_idx, legal_count)
    with make("a", "resident") as ev:
        assert ev.tower_kernel() == RESIDENT
        assert same(ev.eval(planes), want)
        probs, lv = ev.eval_legal(planes, legal_idx, legal_count)
        assert same((lv,), (want[1],))
        for i in range(n):
            assert same((probs[i, : legal_count[i]],), (want_legal[0][i, : legal_count[i]],)), i
        # the leaf server: blocking, and by ticket
        p, v = np.empty((n, d.moves), dtype=np.float32), np.empty((n,), dtype=np.float32)
        f32p = C.POINTER(C.c_float)
        assert ev._lib.cattus_hip_apply(ev._h, np.ascontiguousarray(planes).ctypes.data_as(C.POINTER(C.c_uint64)), n, p.ctypes.data_as(f32p), v.ctypes.data_as(f32p)) == 0
        assert same((p, v), want)
        tickets = [ev.submit(x) for x in planes]
        ev.flush()
        got = [ev.wait(t) for t in tickets]
        assert same((np.stack([g[0] for g in got]), np.array([g[1] for g in got], dtype=np.float32)), want)
        # device buffers, either lane
        dev = torch.device("cuda", 0)
        d_planes = torch.from_numpy(planes.copy().view(np.int64)).to(dev)
        for lane in (0, 1):
            pol = torch.zeros((n, d.moves), dtype=torch.float32, device=dev)
            val = torch.zeros((n,), dtype=torch.float32, device=dev)
            ev.eval_device(d_planes.data_ptr(), n, pol.data_ptr(), val.data_ptr(), ev.lane_stream(lane), lane=lane)
            torch.cuda.synchronize()
            assert same((pol.cpu().numpy(), val.cpu().numpy()), want), lane


# ---- 3. range ----
def test_the_clamp_counts_the_same_elements_in_both_forms():
    """The networks of tests/test_hip_parity.py::test_f16x2_range_large_batchnorm_scales: a stem BatchNorm weight of 200 keeps the stream
    inside the f16 range, one of 1e5 sends it past 65504.  Both forms run the same padded batch (12 boards for 9 leaves: whole 256-row
    workgroups of the per-layer kernel, the same count on the resident plan), both expand only the n leaves' planes and both mask the
    pixel slots past the board, so the counts are compared as they come, on n = 9 of max_batch = 16."""
    d = NetDesc(**CHESS, blocks=2, filters=64, vhc=8, phc=8)
    planes = synth.random_chess_planes(9, 4)
    for scale, saturates in ((200.0, False), (1e5, True)):
        t = seeded_tensors(d, 6)
        t["_conv1._bn.weight"] = t["_conv1._bn.weight"] * np.float32(scale)
        t["_residual_blocks.0._conv1.weight"] = t["_residual_blocks.0._conv1.weight"] * np.float32(1e-3)
        blob = pack_tensors(d, t)
        out = {}
        for form, kernel in (("auto", PER_LAYER), ("resident", RESIDENT)):
            with HipEvaluator(blob, 16, 1, dtype="f16", tower_form=form, switches={}) as ev:
                assert ev.tower_kernel() == kernel and ev.stats()["saturated"] == 0
                p, v = ev.eval(planes)
                sat = ev.stats()["saturated"]
                ev.eval(planes)
                assert ev.stats()["saturated"] == 2 * sat  # sticky
            out[form] = (p, v, sat)
        print("stem BatchNorm x %g: saturated auto %d resident %d" % (scale, out["auto"][2], out["resident"][2]))
        assert np.isfinite(out["auto"][0]).all() and np.isfinite(out["auto"][1]).all()
        assert same(out["resident"][:2], out["auto"][:2]), scale
        assert out["resident"][2] == out["auto"][2] and (out["auto"][2] > 0) == saturates, (scale, out["auto"][2], out["resident"][2])


# ---- 4. stream shifts ----
def test_shifted_streams_are_folded_into_the_weights_of_both_forms_alike():
    game, _, _, n, _, _ = CASES["b"]
    d = desc_of("b")
    blob = pack_tensors(d, stream_twin(d, seeded_tensors(d, 11), 2.0**-6))
    planes = planes_of(game, n, 3)
    sample = planes_of(game, 32, 9)
    for cal in (None, sample):
        out = {}
        for form, kernel in (("auto", PER_LAYER), ("resident", RESIDENT)):
            with make("b", form, blob=blob, calibration=cal) as ev:
                assert ev.tower_kernel() == kernel
                out[form] = (ev.stream_shifts(), ev.stream_shift(), *ev.eval(planes), ev.stats()["saturated"])
        a, r = out["auto"], out["resident"]
        assert (a[0] != 0).any(), "the twin's scale shifts no channel"
        assert np.array_equal(a[0], r[0]) and a[1] == r[1]
        assert same(r[2:4], a[2:4]) and a[4] == r[4] == 0, "calibrated" if cal is not None else "estimated"


# ---- 5. observation ----
def test_observed_passes_see_the_per_layer_towers_tensors():
    game, blocks, filters, n, _, _ = CASES["a"]
    planes = planes_of(game, n, 3)
    want = auto_outputs("a")[0]
    P = 2 + 2 * blocks
    with make("a", "auto") as ev:
        assert ev.points() == P
        taps = [ev.tap(planes, point) for point in range(P)]
    with make("a", "resident", verify_every=1) as ev:
        assert ev.tower_kernel() == RESIDENT and ev.points() == P
        assert same(ev.eval(planes), want)
        assert ev.verify_stats()["batches"] == 1 and ev.verify_stats()["leaves"] == n
        for point in range(P):
            x, tp, tv = ev.tap(planes, point, outputs=True)
            assert same((x,), (taps[point],)), point
            assert same((tp, tv), want), point
        assert taps[0].shape == (n, filters, 7, 7) and taps[P - 1].shape == (n, 8, 7, 7)
        rec, rp, rv = ev.trace(planes)
        assert rec.shape == (P, n) and (rec["flags"] == 0).all()
        assert same((rp, rv), want)
        assert same(ev.eval(planes), want)
        # tap and trace are not batches.  (leaves_outside is not held to 0: 11 significant bits are outside the reference's cross-runtime
        # bar under either form -- the same leaves, since the outputs are the same bits)
        assert ev.verify_stats()["batches"] == 2 and ev.verify_stats()["leaves"] == 2 * n


# ---- 6. the form's edges ----
def test_the_form_is_refused_where_no_resident_kernel_covers_the_evaluator(monkeypatch):
    wide = seeded_blob(NetDesc(**CHESS, blocks=2, filters=128, vhc=4, phc=4), 11)
    refused = [
        ("f16 with 128 filters", wide, "f16", {}),
        ("f16 with CATTUS_TOWER64=0", blob_of("b"), "f16", {"CATTUS_TOWER64": "0"}),
        ("f32", blob_of("b"), "f32", {}),
        ("f16w", wide, "f16w", {}),
        ("f32w", wide, "f32w", {}),
        ("bf16 with 128 filters", wide, "bf16", {}),
        ("f16x2 with 128 filters", wide, "f16x2", {}),
        ("bf16 with CATTUS_TOWER64=0", blob_of("b"), "bf16", {"CATTUS_TOWER64": "0"}),
    ]
    for label, blob, dtype, switches in refused:
        with pytest.raises(CattusHipError) as ei:
            HipEvaluator(blob, 12, 1, dtype=dtype, tower_form="resident", switches=switches)
        assert ei.value.status == -2, label  # CATTUS_E_UNSUPPORTED
    monkeypatch.setitem(evaluator.TOWER_FORMS_RESIDENT, "six", 6)
    with pytest.raises(CattusHipError) as ei:
        HipEvaluator(blob_of("b"), 12, 1, dtype="f16", tower_form="six", switches={})
    assert ei.value.status == -1  # CATTUS_E_INVALID


@pytest.mark.parametrize("dtype,kernel", [("bf16", RESIDENT), ("f16x2", SPLIT)])
def test_the_form_is_what_auto_already_runs_for_bf16_and_f16x2(dtype, kernel):
    game, _, _, n, _, _ = CASES["b"]
    planes = planes_of(game, n, 3)
    out = {}
    for form in ("auto", "resident"):
        with make("b", form, dtype=dtype) as ev:
            assert ev.tower_kernel() == kernel and ev.time_tower(n, 1)[1] == 1
            out[form] = ev.eval(planes)
    assert same(out["resident"], out["auto"])


def test_auto_never_picks_the_form_for_f16_and_a_simple_model_runs_in_f32_under_it():
    for case in ("a", "b", "e"):
        with make(case, "auto") as ev:
            assert ev.tower_kernel() == PER_LAYER
        with make(case, None) as ev:  # the constructor's default
            assert ev.tower_kernel() == PER_LAYER
    d = simple_desc(**TTT)
    planes = planes_of("ttt", 3, 3)
    out = {}
    for form in ("auto", "resident"):
        with HipEvaluator(seeded_blob(d, 4), 4, 1, dtype="f16", tower_form=form, switches={}) as ev:
            assert ev.tower_kernel() == "policy_fc_kernel"
            out[form] = ev.eval(planes)
    assert same(out["resident"], out["auto"])
