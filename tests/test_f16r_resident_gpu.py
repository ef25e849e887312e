"""dtype "f16r_resident" on the device: the f16 tower with an f32 residual stream of a network with at most 64 filters in ONE
LDS-resident launch (tower64_stream_kernel<CH, BIG, LS>, the stream in the owning lanes' registers), held bit for bit to the tower it
is another way of launching -- dtype "f16r", 1 + 2 * blocks launches of conv3x3_f16r_kernel / conv3x3_mfma_v2_kernel<_Float16>.  On the
parent commit dtype 7 is CATTUS_E_INVALID (and the binding has no such name) and every test here fails.
tests/test_t64r_rule.py checks, without a GPU, the header the epilogue and the evaluator's layer table are written with.

`same` is bit equality.  The reference side of every comparison is dtype f16r, per layer, on the same blob -- never the code under
test.  Its outputs are computed once per network, shared, and never written to.  Seeded networks have vhc = phc = 4.

Workgroup shapes (the instances of the kernel), each with 0, 1, 2 and 3 blocks (the stem as the last layer; one skip out of the
registers; a skip of a value an earlier conv2 left there) and 16 and 64 filters (padded channels; all 64 live), on 1, 3 and 6 leaves of
max_batch 6 (8 padded boards: 3 leaves leave a two-board workgroup half empty and whole workgroups without a leaf):

  chess        8x8    CH = 4, three barriers per layer (64 pixels: every pixel slot live)
  hex7 / ttt   7x7 / 3x3   CH = 4, one barrier per layer (LS); *_no_ls: CATTUS_T64_LS=0, three barriers under 64 pixels
  chess_ch2    8x8    CATTUS_T64_CH=2: 128-row workgroups, two boards each
  hex9         9x9    BIG: 128 pixel slots per board, two plane words"""

import ctypes as C
import functools
import json
import threading

import numpy as np
import pytest

from cattus_amd import evaluator, synth
from cattus_amd.evaluator import CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, TTT, NetDesc, hex_game, pack_tensors, seeded_blob, seeded_tensors, simple_desc

from helpers import stream_twin

pytestmark = pytest.mark.gpu

STREAM, PER_LAYER, F16_KERNEL = "tower64_stream_kernel", "conv3x3_f16r_kernel", "conv3x3_mfma_v2_kernel"
GAMES = {"chess": CHESS, "ttt": TTT, "hex7": hex_game(7), "hex9": hex_game(9)}
# name: (game, switches)
SHAPES = {
    "chess": ("chess", {}),
    "hex7": ("hex7", {}),
    "hex7_no_ls": ("hex7", {"CATTUS_T64_LS": "0"}),
    "ttt": ("ttt", {}),
    "ttt_no_ls": ("ttt", {"CATTUS_T64_LS": "0"}),
    "chess_ch2": ("chess", {"CATTUS_T64_CH": "2"}),
    "hex9": ("hex9", {}),
}
MAX_BATCH, LEAVES = 6, (1, 3, 6)


def words_of(game):
    return 2 if game.startswith("hex") else 1


def desc_of(game, blocks, filters):
    return NetDesc(**GAMES[game], blocks=blocks, filters=filters, vhc=4, phc=4)


@functools.lru_cache(maxsize=None)
def blob_of(game, blocks, filters):
    return seeded_blob(desc_of(game, blocks, filters), 11)


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


def make(game, blob, dtype, max_batch=MAX_BATCH, switches=None, **kw):
    return HipEvaluator(blob, max_batch, words_of(game), dtype=dtype, switches=dict(switches or {}), **kw)


def same(got, want):
    got, want = (got, want) if isinstance(got, (tuple, list)) else ((got,), (want,))
    return len(got) == len(want) and all(
        np.asarray(g).shape == np.asarray(w).shape and np.array_equal(np.asarray(g, dtype=np.float32).view(np.uint32), np.asarray(w, dtype=np.float32).view(np.uint32))
        for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def per_layer_outputs(game, blocks, filters):
    """dtype f16r on the net's blob: {n: (logits, values)} for the leaf counts of LEAVES, and the saturated count behind them."""
    out = {}
    with make(game, blob_of(game, blocks, filters), "f16r") as ev:
        assert ev.tower_kernel() == PER_LAYER and ev.time_tower(1, 1)[1] == 1 + 2 * blocks
        for n in LEAVES:
            out[n] = ev.eval(planes_of(game, n, 3))
            for a in out[n]:
                a.setflags(write=False)
        sat = ev.stats()["saturated"]
    return out, sat


# ---- 1. bits, every workgroup shape ----
@pytest.mark.parametrize("filters", [16, 64])
@pytest.mark.parametrize("blocks", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_one_launch_tower_has_the_per_layer_f16r_towers_bits(shape, blocks, filters):
    game, switches = SHAPES[shape]
    want, want_sat = per_layer_outputs(game, blocks, filters)
    assert np.isfinite(want[MAX_BATCH][0]).all() and np.abs(want[MAX_BATCH][0]).max() > 0
    with make(game, blob_of(game, blocks, filters), "f16r_resident", switches=switches) as ev:
        assert ev.tower_kernel() == STREAM and ev.time_tower(1, 1)[1] == 1
        for n in LEAVES:
            assert same(ev.eval(planes_of(game, n, 3)), want[n]), n
        assert same(ev.eval(planes_of(game, LEAVES[0], 3)), want[LEAVES[0]]), "one leaf behind a full batch"
        assert ev.stats()["saturated"] == want_sat == 0


# ---- 2. every entry point ----
def test_every_entry_point_returns_the_per_layer_towers_bits():
    torch = pytest.importorskip("torch")
    game, blocks, filters, n = "hex7", 2, 64, 5
    d = desc_of(game, blocks, filters)
    blob, planes = blob_of(game, blocks, filters), planes_of(game, n, 3)
    rng = np.random.default_rng(5)
    legal_idx = np.stack([rng.choice(d.moves, size=12, replace=False) for _ in range(n)]).astype(np.uint16)
    legal_count = rng.integers(1, 13, size=n).astype(np.uint16)
    with make(game, blob, "f16r", 8) as ev:
        want = ev.eval(planes)
        want_probs, want_lv = ev.eval_legal(planes, legal_idx, legal_count)
    assert same(want_lv, want[1])
    f32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    with make(game, blob, "f16r_resident", 8) as ev:
        assert ev.tower_kernel() == STREAM
        assert same(ev.eval(planes), want)
        probs, lv = ev.eval_legal(planes, legal_idx, legal_count)
        assert same(lv, want[1])
        for i in range(n):
            assert same(probs[i, : legal_count[i]], want_probs[i, : legal_count[i]]), i
        # cattus_hip_apply from four threads at once: the leaf server batches them as it likes, a leaf's bits do not depend on its batch
        got, errors = {}, []

        def worker(k):
            p, v = np.empty((n, d.moves), dtype=np.float32), np.empty((n,), dtype=np.float32)
            rc = ev._lib.cattus_hip_apply(ev._h, np.ascontiguousarray(planes).ctypes.data_as(u64p), n, p.ctypes.data_as(f32p), v.ctypes.data_as(f32p))
            if rc:
                errors.append((k, rc))
            got[k] = (p, v)

        threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors and all(same(got[k], want) for k in range(4))
        # apply_legal: the leaf server with legal lists
        plists, av = ev.apply_legal(planes, [legal_idx[i, : legal_count[i]] for i in range(n)])
        assert same(av, want[1]) and all(same(plists[i], want_probs[i, : legal_count[i]]) for i in range(n))
        # device buffers, either lane
        dev = torch.device("cuda", 0)
        d_planes = torch.from_numpy(planes.copy().view(np.int64)).to(dev)
        for lane in (0, 1):
            pol = torch.zeros((n, d.moves), dtype=torch.float32, device=dev)
            val = torch.zeros((n,), dtype=torch.float32, device=dev)
            ev.eval_device(d_planes.data_ptr(), n, pol.data_ptr(), val.data_ptr(), ev.lane_stream(lane), lane=lane)
            torch.cuda.synchronize()
            assert same((pol.cpu().numpy(), val.cpu().numpy()), want), lane
        assert ev.stats()["saturated"] == 0


# ---- 3. no blocks: dtype f16's bits too (the rule's anchor) ----
@pytest.mark.parametrize("shape", ["chess", "hex7", "chess_ch2", "hex9"])
def test_without_blocks_the_bits_are_also_dtype_f16s(shape):
    game, switches = SHAPES[shape]
    blob, planes = blob_of(game, 0, 64), planes_of(game, 3, 3)
    with make(game, blob, "f16") as ev:
        assert ev.tower_kernel() == F16_KERNEL
        want = ev.eval(planes)
    with make(game, blob, "f16r_resident", switches=switches) as ev:
        assert ev.tower_kernel() == STREAM
        assert same(ev.eval(planes), want)


# ---- 4. range ----
def test_copies_beyond_the_f16_range_are_clamped_and_counted_as_per_layer():
    """The construction of tests/test_f16r_gpu.py: a stem BatchNorm weight of 200 keeps every copy inside the f16 range; one of 1e5 sends
    the stem's beyond 65504 -- the copies are clamped and counted, the f32 stream (here: the registers) keeps its values.  Both towers
    run 12 padded boards for 9 leaves and mask the same pixel slots, so the counts are compared as they come."""
    d = NetDesc(**CHESS, blocks=2, filters=64, vhc=8, phc=8)
    planes = synth.random_chess_planes(9, 4)
    for scale, saturates in ((200.0, False), (1e5, True)):
        t = seeded_tensors(d, 6)
        t["_conv1._bn.weight"] = t["_conv1._bn.weight"] * np.float32(scale)
        t["_residual_blocks.0._conv1.weight"] = t["_residual_blocks.0._conv1.weight"] * np.float32(1e-3)
        blob = pack_tensors(d, t)
        out = {}
        for dtype, kernel in (("f16r", PER_LAYER), ("f16r_resident", STREAM)):
            with make("chess", blob, dtype, 16) as ev:
                assert ev.tower_kernel() == kernel and ev.stats()["saturated"] == 0
                p, v = ev.eval(planes)
                sat = ev.stats()["saturated"]
                ev.eval(planes)
                assert ev.stats()["saturated"] == 2 * sat  # sticky
            out[dtype] = (p, v, sat)
        print("stem BatchNorm x %g: saturated f16r %d f16r_resident %d" % (scale, out["f16r"][2], out["f16r_resident"][2]))
        assert np.isfinite(out["f16r"][0]).all() and np.isfinite(out["f16r"][1]).all()
        assert same(out["f16r_resident"][:2], out["f16r"][:2]), scale
        assert out["f16r_resident"][2] == out["f16r"][2] and (out["f16r"][2] > 0) == saturates, (scale, out["f16r"][2], out["f16r_resident"][2])


def test_shifted_streams_and_calibrated_shifts_are_the_per_layer_towers():
    """A network whose estimate gives non-zero stream shifts (helpers.stream_twin at 2^-6), and the hidden-twin network of
    tests/test_stream_calibration.py on top of it (every fourth channel 2^16 larger where gamma does not show it), plain and through
    cattus_hip_create_calibrated: shifts, bits and counts are dtype f16r's."""
    from test_stream_calibration import hidden_twin

    d = desc_of("chess", 2, 64)
    planes, sample = planes_of("chess", 6, 3), planes_of("chess", 16, 9)
    twin = stream_twin(d, seeded_tensors(d, 11), 2.0**-6)
    hidden = np.arange(64) % 4 == 1
    nets = {"twin": pack_tensors(d, twin), "hidden": pack_tensors(d, hidden_twin(d, twin, np.where(hidden, 16, 0)))}
    for name, blob in nets.items():
        for cal in (None, sample):
            out = {}
            for dtype, kernel in (("f16r", PER_LAYER), ("f16r_resident", STREAM)):
                with make("chess", blob, dtype, 16, calibration=cal) as ev:
                    assert ev.tower_kernel() == kernel
                    out[dtype] = (ev.stream_shifts(), ev.stream_shift(), *ev.eval(planes), ev.stats()["saturated"])
            a, r = out["f16r"], out["f16r_resident"]
            print("%s, %s: shifts %d..%d, saturated f16r %d f16r_resident %d" % (name, "calibrated" if cal is not None else "estimated", a[0].min(), a[0].max(), a[4], r[4]))
            assert (a[0] != 0).any(), "the twin's scale shifts no channel"
            assert np.array_equal(a[0], r[0]) and a[1] == r[1]
            assert same(r[2:4], a[2:4]) and a[4] == r[4], (name, cal is not None)
        if name == "hidden":  # calibration lowered the hidden channels' shifts until nothing saturates (tests/test_f16r_gpu.py): under both dtypes
            assert a[4] == 0


# ---- 5. observation ----
def test_taps_traces_and_verification_are_the_per_layer_towers():
    game, blocks, filters, n = "hex7", 2, 64, 5
    blob, planes, planes2 = blob_of(game, blocks, filters), planes_of(game, n, 3), planes_of(game, 3, 4)
    P = 2 + 2 * blocks
    rng = np.random.default_rng(5)
    legal_idx = np.stack([rng.choice(49, size=12, replace=False) for _ in range(n)]).astype(np.uint16)
    legal_count = rng.integers(1, 13, size=n).astype(np.uint16)
    with make(game, blob, "f16r", 8, verify_every=1) as ev:
        assert ev.points() == P
        want, want2 = ev.eval(planes), ev.eval(planes2)
        want_probs, _ = ev.eval_legal(planes, legal_idx, legal_count)
        want_stats, want_prior = ev.verify_stats(), ev.verify_prior_stats()
        taps = [ev.tap(planes, point) for point in range(P)]
        want_rec, _, _ = ev.trace(planes)
    with make(game, blob, "f16r_resident", 8, verify_every=1) as ev:
        assert ev.tower_kernel() == STREAM and ev.points() == P
        assert same(ev.eval(planes), want) and same(ev.eval(planes2), want2)  # verified batches return the evaluator's own bits
        probs, _ = ev.eval_legal(planes, legal_idx, legal_count)
        assert all(same(probs[i, : legal_count[i]], want_probs[i, : legal_count[i]]) for i in range(n))
        stats = ev.verify_stats()
        assert stats["batches"] == 3 and stats["leaves"] == 2 * n + 3 and stats == want_stats
        assert want_prior["leaves"] == n and ev.verify_prior_stats() == want_prior
        for point in range(P):
            x, tp, tv = ev.tap(planes, point, outputs=True)
            assert same(x, taps[point]), point
            assert same((tp, tv), want), point
        assert taps[0].shape == (n, filters, 7, 7) and not same(np.float16(taps[2]).astype(np.float32), taps[2])  # a stream point: f32, not f16 values
        rec, rp, rv = ev.trace(planes)
        assert rec.shape == (P, n) and rec.tobytes() == want_rec.tobytes()
        assert same((rp, rv), want)
        assert same(ev.eval(planes), want), "behind observed passes"
        assert ev.verify_stats()["batches"] == 4  # tap and trace are not batches
        assert ev.tower_kernel() == STREAM


# ---- 6. the plan ----
def test_the_plan_one_launch_whatever_the_form():
    game, blocks, filters = "chess", 2, 16
    blob, planes = blob_of(game, blocks, filters), planes_of(game, 3, 3)
    want = per_layer_outputs(game, blocks, filters)[0][3]
    with make(game, blob, "f16r") as ev:
        assert ev.time_tower(3, 1)[1] == 1 + 2 * blocks
    for form in ("auto", "resident", "direct", "winograd", "winograd_f4", "direct_splitk", None):
        with make(game, blob, "f16r_resident", tower_form=form, tail_leaves=0 if form is None else 2) as ev:
            assert ev.tower_kernel() == STREAM, form
            assert ev.time_tower(3, 1)[1] == 1
            assert ev.tail_leaves() == 0
            assert same(ev.eval(planes), want), form
            assert ev.tail_batches() == 0


# ---- 7. edges ----
def test_what_the_form_does_not_cover_is_refused_under_the_dtypes_name(monkeypatch):
    small = blob_of("chess", 2, 16)
    wide = seeded_blob(NetDesc(**CHESS, blocks=2, filters=128, vhc=4, phc=4), 11)
    wide_heads = seeded_blob(NetDesc(**CHESS, blocks=1, filters=64, vhc=20, phc=20), 7)
    many_planes = seeded_blob(NetDesc(**dict(CHESS, planes=70), blocks=1, filters=64, vhc=4, phc=4), 7)
    refused = [("128 filters", wide, {}), ("vhc + phc > 32", wide_heads, {}), ("CATTUS_TOWER64=0", small, {"CATTUS_TOWER64": "0"}), ("70 planes", many_planes, {})]
    for label, blob, switches in refused:
        for form in ("auto", "resident"):
            with pytest.raises(CattusHipError) as ei:
                HipEvaluator(blob, 12, 1, dtype="f16r_resident", tower_form=form, switches=switches)
            assert ei.value.status == -2 and "f16r" in str(ei.value), (label, form, str(ei.value))  # CATTUS_E_UNSUPPORTED
    # ... and dtype f16 with tower_form resident draws the same line
    for label, blob, switches in refused:
        with pytest.raises(CattusHipError) as ei:
            HipEvaluator(blob, 12, 1, dtype="f16", tower_form="resident", switches=switches)
        assert ei.value.status == -2, label
    with HipEvaluator(seeded_blob(NetDesc(**dict(CHESS, planes=40), blocks=1, filters=64, vhc=4, phc=4), 7), 12, 1, dtype="f16r_resident", switches={}) as ev:
        assert ev.tower_kernel() == STREAM  # more than 32 planes, at most 64: the launch expands them itself
    monkeypatch.setitem(evaluator.TOWER_FORMS_RESIDENT, "six", 6)
    with pytest.raises(CattusHipError) as ei:
        HipEvaluator(small, 12, 1, dtype="f16r_resident", tower_form="six", switches={})
    assert ei.value.status == -1  # CATTUS_E_INVALID
    monkeypatch.setitem(evaluator._DTYPES_F16R_RESIDENT, "eight", 8)
    with pytest.raises(CattusHipError) as ei:
        HipEvaluator(small, 12, 1, dtype="eight", switches={})
    assert ei.value.status == -1


def test_forty_planes_run_the_launch_with_the_per_layer_towers_bits():
    """More than 32 planes: the per-layer tower packs them in a launch of its own, the resident launch expands up to 64 itself."""
    d = NetDesc(**dict(CHESS, planes=40), blocks=1, filters=64, vhc=4, phc=4)
    blob = seeded_blob(d, 7)
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, size=(5, 40, 64), dtype=np.uint64)
    planes = np.zeros((5, 40, 1), dtype=np.uint64)
    for i in range(64):
        planes[:, :, 0] |= bits[:, :, i] << np.uint64(i)
    out = {}
    for dtype, kernel in (("f16r", PER_LAYER), ("f16r_resident", STREAM)):
        with HipEvaluator(blob, 6, 1, dtype=dtype, switches={}) as ev:
            assert ev.tower_kernel() == kernel
            out[dtype] = ev.eval(planes)
    assert np.abs(out["f16r"][0]).max() > 0 and same(out["f16r_resident"], out["f16r"])


def test_a_simple_model_runs_in_f32_and_the_self_player_reaches_the_dtype(tmp_path, monkeypatch):
    sd = simple_desc(**TTT)
    tplanes = planes_of("ttt", 3, 3)
    out = {}
    for dtype in ("f32", "f16r_resident"):
        with HipEvaluator(seeded_blob(sd, 4), 4, 1, dtype=dtype, switches={}) as ev:
            assert ev.tower_kernel() == "policy_fc_kernel"
            out[dtype] = ev.eval(tplanes)
    assert same(out["f16r_resident"], out["f32"])

    from cattus_amd import selfplay as sp

    seen = []

    class Recording(evaluator.HipEvaluator):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            seen.append((kw.get("dtype"), self.tower_kernel()))

    monkeypatch.setattr(evaluator, "HipEvaluator", Recording)
    model = tmp_path / "model.cattus"
    model.write_bytes(seeded_blob(NetDesc(**TTT, blocks=1, filters=16, vhc=4, phc=4), 9))
    cfg = {
        "model": {"inference": {"engine": "hip", "device": 0, "dtype": "f16r_resident"}, "batch_size": 4},
        "mcts": {"sim_num": 8, "explore_factor": 1.41421, "temperature_policy": [[9999, 0.0]], "prior_noise_alpha": 0.0, "prior_noise_epsilon": 0.0, "cache_size": 1000},
        "threads": 1,
        "concurrent_games": 1,
    }
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    # (the self-player plays its games in pairs, one per colour: two is the fewest)
    sp.main(["--game", "tictactoe", "--model1-path", str(model), "--model2-path", str(model), "--games-num", "2", "--out-dir1", str(tmp_path / "o1"), "--out-dir2",
             str(tmp_path / "o2"), "--summary-file", str(tmp_path / "summary.json"), "--config-file", str(tmp_path / "cfg.json")])
    s = json.loads((tmp_path / "summary.json").read_text())
    assert s["player1_wins"] + s["player2_wins"] + s["draws"] == 2 and s["metrics"]["model.activation_count"] > 0
    assert seen and all(k == ("f16r_resident", STREAM) for k in seen), seen
