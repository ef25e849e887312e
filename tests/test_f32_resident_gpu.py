"""dtype "f32_resident" on the device: the exact f32 tower of a network with at most 64 filters and 32 planes in ONE LDS-resident launch
(tower64_f32_kernel<CH, BIG>), held bit for bit to the tower it is another way of launching -- dtype "f32", 1 + 2 * blocks launches of
conv3x3_mfma_v2_kernel<float>, whose bits are the CPU oracle's.  On the parent commit dtype 9 is CATTUS_E_INVALID (and the binding has no
such name) and every test here fails.  tests/test_t64f_rule.py checks, without a GPU, the header the kernel and the evaluator are written with.

`same` is bit equality; there is no tolerance anywhere.  The reference side of every comparison is dtype f32, per layer, on the same blob
(asserted by tower_kernel() and time_tower's launch count) -- never the code under test.  Its outputs are computed once per network, shared,
and never written to.  Seeded networks have vhc = phc = 4.

Workgroup shapes (the three instances of the kernel), each with 0, 1, 2 and 3 blocks (the stem as the last layer; one skip; a skip of a
value an earlier conv2 left in LDS) and 16, 32, 33 and 64 filters (the narrow walk and its edge; the first filter count that needs chunk 1;
all 64 live), on 1, 3 and 6 leaves of max_batch 6 (8 padded boards), then one leaf behind the full batch:

  chess        8x8          64 rows per workgroup, every pixel slot live
  hex7 / ttt   7x7 / 3x3    64 rows, padded pixel slots
  chess_ch2    8x8          CATTUS_T64_CH=2: 128-row workgroups, two boards each; 3 leaves leave one half empty
  hex9 / hex11 9x9 / 11x11  BIG: 128 pixel slots per board, two plane words"""

import ctypes as C
import functools
import json
import threading

import numpy as np
import pytest

from cattus_amd import evaluator, synth
from cattus_amd.evaluator import CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, TTT, NetDesc, hex_game, seeded_blob, simple_desc

from helpers import blob_for, golden_names, load_golden, outputs_equal_ref_tol

pytestmark = pytest.mark.gpu

RESIDENT, PER_LAYER = "tower64_f32_kernel", "conv3x3_mfma_v2_kernel"
GAMES = {"chess": CHESS, "ttt": TTT, "hex4": hex_game(4), "hex7": hex_game(7), "hex9": hex_game(9), "hex11": hex_game(11)}
# name: (game, switches)
SHAPES = {
    "chess": ("chess", {}),
    "hex7": ("hex7", {}),
    "ttt": ("ttt", {}),
    "chess_ch2": ("chess", {"CATTUS_T64_CH": "2"}),
    "hex9": ("hex9", {}),
    "hex11": ("hex11", {}),
}
MAX_BATCH, LEAVES = 6, (1, 3, 6)
UNSUPPORTED, INVALID = -2, -1


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


def is_per_layer_f32(ev, blocks):
    return ev.tower_kernel() == PER_LAYER and ev.time_tower(1, 1)[1] == 1 + 2 * blocks


def is_resident(ev):
    return ev.tower_kernel() == RESIDENT and ev.time_tower(1, 1)[1] == 1


@functools.lru_cache(maxsize=None)
def per_layer_outputs(game, blocks, filters):
    """dtype f32 on the net's blob: {n: (logits, values)} for the leaf counts of LEAVES."""
    out = {}
    with make(game, blob_of(game, blocks, filters), "f32") as ev:
        assert is_per_layer_f32(ev, blocks)
        for n in LEAVES:
            out[n] = ev.eval(planes_of(game, n, 3))
            for a in out[n]:
                a.setflags(write=False)
    return out


# ---- 1. bits, every instance ----
@pytest.mark.parametrize("filters", [16, 32, 33, 64])
@pytest.mark.parametrize("blocks", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_one_launch_tower_has_the_per_layer_f32_towers_bits(shape, blocks, filters):
    game, switches = SHAPES[shape]
    want = per_layer_outputs(game, blocks, filters)
    assert np.isfinite(want[MAX_BATCH][0]).all() and np.abs(want[MAX_BATCH][0]).max() > 0
    with make(game, blob_of(game, blocks, filters), "f32_resident", switches=switches) as ev:
        assert is_resident(ev)
        for n in LEAVES:
            assert same(ev.eval(planes_of(game, n, 3)), want[n]), n
        assert same(ev.eval(planes_of(game, LEAVES[0], 3)), want[LEAVES[0]]), "one leaf behind a full batch"
        assert ev.stats()["saturated"] == 0


# ---- 2. the narrow walk ----
@pytest.mark.parametrize("game", ["chess", "hex7", "hex9"])
@pytest.mark.parametrize("filters", [16, 32, 33])
def test_the_narrow_walk_changes_no_bit(game, filters):
    """At most 32 filters: hidden layers walk chunk 0 alone (3 steps instead of 6); CATTUS_T64F_NARROW=0 walks both.  Both are dtype f32's
    bits.  33 filters need chunk 1 either way.  (What the narrow walk saves is not asserted here: scripts/f32_resident_time.py measures it,
    0.56x the launch and 0.61x the step on chess 7x16.)"""
    blocks = 2
    want = per_layer_outputs(game, blocks, filters)
    got = {}
    for narrow in ("1", "0"):
        with make(game, blob_of(game, blocks, filters), "f32_resident", switches={"CATTUS_T64F_NARROW": narrow}) as ev:
            assert is_resident(ev)
            got[narrow] = {n: ev.eval(planes_of(game, n, 3)) for n in LEAVES}
    for n in LEAVES:
        assert same(got["1"][n], got["0"][n]) and same(got["1"][n], want[n]), n


# ---- 3. the shape switch under AUTO ----
def test_a_large_batch_takes_128_row_workgroups_and_a_small_one_behind_it_64():
    game, blocks, filters, big = "hex7", 1, 64, 260
    blob, planes = blob_of(game, blocks, filters), planes_of(game, big, 5)
    with make(game, blob, "f32", big) as ev:
        assert is_per_layer_f32(ev, blocks)
        want_big, want_small = ev.eval(planes), ev.eval(planes[:5])
    with make(game, blob, "f32_resident", big) as ev:
        assert is_resident(ev)
        assert same(ev.eval(planes), want_big), "260 padded boards: 128 rows per workgroup"
        assert same(ev.eval(planes[:5]), want_small), "8 padded boards on the same evaluator: 64 rows per workgroup"


# ---- 4. every entry point ----
def test_every_entry_point_returns_the_per_layer_towers_bits():
    torch = pytest.importorskip("torch")
    game, blocks, filters, n = "hex7", 2, 64, 5
    d = desc_of(game, blocks, filters)
    blob, planes = blob_of(game, blocks, filters), planes_of(game, n, 3)
    P = 2 + 2 * blocks
    rng = np.random.default_rng(5)
    legal_idx = np.stack([rng.choice(d.moves, size=12, replace=False) for _ in range(n)]).astype(np.uint16)
    legal_count = rng.integers(1, 13, size=n).astype(np.uint16)
    with make(game, blob, "f32", 8) as ev:
        assert is_per_layer_f32(ev, blocks) and ev.points() == P
        want = ev.eval(planes)
        want_probs, want_lv = ev.eval_legal(planes, legal_idx, legal_count)
        taps = [ev.tap(planes, point) for point in range(P)]
    assert same(want_lv, want[1])
    f32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    with make(game, blob, "f32_resident", 8) as ev:
        assert is_resident(ev) and ev.points() == P
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
        # submit + wait: one leaf each through the leaf server
        tickets = [ev.submit(planes[i]) for i in range(n)]
        for i, t in enumerate(tickets):
            p, v = ev.wait(t)
            assert same((p, np.float32(v)), (want[0][i], want[1][i])), i
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
        # taps at every point: the per-layer twin on the same buffers, dtype f32's taps; the pass's outputs too
        for point in range(P):
            x, tp, tv = ev.tap(planes, point, outputs=True)
            assert same(x, taps[point]), point
            assert same((tp, tv), want), point
        assert taps[0].shape == (n, filters, 7, 7)
        assert same(ev.eval(planes), want) and ev.tower_kernel() == RESIDENT, "behind observed passes"
        # the short-chain FC pair applies as under f32: on and off, the same bits
        ev.head_chain(8)
        assert ev.head_chain_leaves() == 8
        before = ev.head_chain_batches()
        assert same(ev.eval(planes), want) and ev.head_chain_batches() == before + 1
        ev.head_chain(0)
        assert same(ev.eval(planes), want) and ev.head_chain_batches() == before + 1
        assert ev.stats()["saturated"] == 0


# ---- 5. reference-made fixtures ----
def covered(name):
    d = load_golden(name)[0]
    return d.filters <= 64 and d.planes <= 32


@pytest.mark.parametrize("name", [n for n in golden_names() if covered(n)])
def test_reference_made_fixtures_go_through_with_dtype_f32s_bits(name):
    d, blob, z = blob_for(name)
    planes = z["planes"]
    with HipEvaluator(blob, batch_size=len(planes) + 3, plane_words=planes.shape[2], dtype="f32", switches={}) as ev:
        assert d.filters == 0 or is_per_layer_f32(ev, d.blocks)
        want = ev.eval(planes)
    with HipEvaluator(blob, batch_size=len(planes) + 3, plane_words=planes.shape[2], dtype="f32_resident", switches={}) as ev:
        assert ev.tower_kernel() == (RESIDENT if d.filters else "policy_fc_kernel")
        got = ev.eval(planes)
    assert same(got, want)
    assert outputs_equal_ref_tol(got[0], got[1], z["policy"], z["value"])


# ---- 6. edges ----
def test_what_the_form_does_not_cover_is_refused_under_the_dtypes_name(monkeypatch):
    small = blob_of("chess", 2, 16)
    wide = seeded_blob(NetDesc(**CHESS, blocks=2, filters=128, vhc=4, phc=4), 11)
    wide_heads = seeded_blob(NetDesc(**CHESS, blocks=1, filters=64, vhc=20, phc=20), 7)
    forty_planes = seeded_blob(NetDesc(**dict(CHESS, planes=40), blocks=1, filters=64, vhc=4, phc=4), 7)
    refused = [("128 filters", wide, {}), ("40 planes", forty_planes, {}), ("vhc + phc > 32", wide_heads, {}), ("CATTUS_TOWER64=0", small, {"CATTUS_TOWER64": "0"})]
    for label, blob, switches in refused:
        for form in ("auto", "resident"):
            with pytest.raises(CattusHipError) as ei:
                HipEvaluator(blob, 12, 1, dtype="f32_resident", tower_form=form, switches=switches)
            assert ei.value.status == UNSUPPORTED and "f32_resident" in str(ei.value), (label, form, str(ei.value))
    # ... and dtype f32 with tower_form resident stays refused
    with pytest.raises(CattusHipError) as ei:
        HipEvaluator(small, 12, 1, dtype="f32", tower_form="resident", switches={})
    assert ei.value.status == UNSUPPORTED
    # dtype 8 is unassigned
    monkeypatch.setitem(evaluator._DTYPES_F32_RESIDENT, "eight", 8)
    with pytest.raises(CattusHipError) as ei:
        HipEvaluator(small, 12, 1, dtype="eight", switches={})
    assert ei.value.status == INVALID


def test_the_forms_of_other_towers_are_ignored_and_the_exact_tower_has_no_shadow():
    game, blocks, filters = "chess", 2, 16
    blob, planes = blob_of(game, blocks, filters), planes_of(game, 3, 3)
    want = per_layer_outputs(game, blocks, filters)[3]
    for form in ("auto", "resident", "direct", "winograd", "winograd_f4", "direct_splitk"):
        with make(game, blob, "f32_resident", tower_form=form, tail_leaves=2) as ev:
            assert is_resident(ev), form
            assert ev.tail_leaves() == 0
            assert same(ev.eval(planes), want), form
    with make(game, blob, "f32_resident") as ev:
        for call in (lambda: ev.verify(1), lambda: ev.trace(planes), lambda: ev.stream_range(planes)):
            with pytest.raises(CattusHipError) as ei:
                call()
            assert ei.value.status == UNSUPPORTED
        assert same(ev.eval(planes), want)
    # nothing to calibrate: cattus_hip_create_calibrated is cattus_hip_create
    with make(game, blob, "f32_resident", calibration=planes_of(game, 6, 9)) as ev:
        assert is_resident(ev) and same(ev.eval(planes), want)


def test_a_simple_model_runs_in_f32():
    sd = simple_desc(**TTT)
    tplanes = planes_of("ttt", 3, 3)
    out = {}
    for dtype in ("f32", "f32_resident"):
        with HipEvaluator(seeded_blob(sd, 4), 4, 1, dtype=dtype, switches={}) as ev:
            assert ev.tower_kernel() == "policy_fc_kernel"
            out[dtype] = ev.eval(tplanes)
    assert same(out["f32_resident"], out["f32"])


def test_the_self_player_writes_dtype_f32s_records(tmp_path, monkeypatch):
    from cattus_amd import selfplay as sp

    seen = []

    class Recording(evaluator.HipEvaluator):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            seen.append((kw.get("dtype"), self.tower_kernel()))

    monkeypatch.setattr(evaluator, "HipEvaluator", Recording)
    model = tmp_path / "model.cattus"
    model.write_bytes(seeded_blob(NetDesc(**GAMES["hex4"], blocks=1, filters=16, vhc=4, phc=4), 9))
    records = {}
    for dtype in ("f32", "f32_resident"):
        cfg = {
            "model": {"inference": {"engine": "hip", "device": 0, "dtype": dtype}, "batch_size": 4},
            "mcts": {"sim_num": 8, "explore_factor": 1.41421, "temperature_policy": [[9999, 0.0]], "prior_noise_alpha": 0.0, "prior_noise_epsilon": 0.0, "cache_size": 1000},
            "threads": 1,
            "concurrent_games": 1,
        }
        out = tmp_path / dtype
        out.mkdir()
        (tmp_path / f"{dtype}.json").write_text(json.dumps(cfg))
        # (the self-player plays its games in pairs, one per colour: two is the fewest)
        sp.main(["--game", "hex4", "--model1-path", str(model), "--model2-path", str(model), "--games-num", "2", "--out-dir1", str(out / "o1"), "--out-dir2",
                 str(out / "o2"), "--summary-file", str(out / "summary.json"), "--config-file", str(tmp_path / f"{dtype}.json")])
        s = json.loads((out / "summary.json").read_text())
        assert s["player1_wins"] + s["player2_wins"] + s["draws"] == 2 and s["metrics"]["model.activation_count"] > 0
        records[dtype] = sorted(p.read_bytes() for p in out.rglob("*") if p.is_file() and p.name != "summary.json")
    assert seen == [("f32", PER_LAYER), ("f32_resident", RESIDENT)], seen
    assert len(records["f32"]) > 2 and records["f32_resident"] == records["f32"]
