"""The two 1x1 head convs in the tail of the resident f16 and f16r towers (cattus_hip_fused_heads; the HEADS instances of
tower64_lds_tower), held BIT FOR BIT -- uint32 views, no tolerance -- to a second evaluator that never had the setting on: logits, values,
priors and stats()["saturated"], through every entry point.  (dtype f32_resident keeps its head conv launch: the setting is ignored there.)

Nets of seeded_blob, max_batch 40, the smallest at which the tail can go wrong:

  ttt 3x3, 8 filters, vhc 4 / phc 8    ocn 12 < 32; 9 of 64 pixel rows valid
  hex7, 16 filters, vhc = phc = 16      ocn = 32
  chess, 16 filters, vhc = phc = 8      hw = 64 = slots: no masked row
  hex9, 16 filters, vhc = phc = 4       128-slot boards: the BIG instances
  hex7, 33 and 64 filters               a padded filter count, and none

with 0 (the stem's epilogue is the last), 1 and 2 blocks; 1, 3 (a pad board in a two-board workgroup), 40 leaves and 1 again behind 40; every
workgroup shape of every dtype (CATTUS_T64_CH = 2 | 4, one barrier per layer or three).  hv persists between passes, so a fused pass that
wrote nothing could be hidden by an earlier pass on the same planes: the fused evaluator evaluates OTHER random planes right before every
compared pass and never runs the compared planes unfused first."""

import ctypes as C
import functools
import json

import numpy as np
import pytest

from cattus_amd import evaluator as evaluator_module
from cattus_amd import synth
from cattus_amd.evaluator import HipEvaluator
from cattus_amd.weights import CHESS, TTT, NetDesc, hex_game, pack_tensors, seeded_blob, seeded_tensors

pytestmark = pytest.mark.gpu

MAX_BATCH = 40
LEAVES = (1, 3, 40, 1)
BLOCKS = (0, 1, 2)
# name: (game fields, filters, vhc, phc, plane words)
NETS = {
    "ttt": (TTT, 8, 4, 8, 1),
    "hex7": (hex_game(7), 16, 16, 16, 2),
    "chess": (CHESS, 16, 8, 8, 1),
    "hex9": (hex_game(9), 16, 4, 4, 2),
    "hex7_f33": (hex_game(7), 33, 16, 16, 2),
    "hex7_f64": (hex_game(7), 64, 16, 16, 2),
}
# dtype: constructor keywords, the resident kernel's name
DTYPES = {
    "f16": ({"tower_form": "resident"}, "tower64_lds_kernel"),
    "f16r_resident": ({}, "tower64_stream_kernel"),
}


def desc(name, blocks):
    game, filters, vhc, phc, _ = NETS[name]
    return NetDesc(**game, blocks=blocks, filters=filters, vhc=vhc, phc=phc)


@functools.lru_cache(maxsize=None)
def blob(name, blocks):
    return seeded_blob(desc(name, blocks), 77)


@functools.lru_cache(maxsize=None)
def planes(name, seed=9):
    d = desc(name, 0)
    if name == "ttt":
        return synth.random_ttt_planes(MAX_BATCH, seed)
    if name.startswith("hex"):
        return synth.random_hex_planes(MAX_BATCH, d.board, seed)
    return synth.random_chess_planes(MAX_BATCH, seed)


def shapes(name, dtype):
    """Every workgroup shape the net can take under the dtype, as diagnostic switches."""
    d = desc(name, 0)
    if d.board > 8:
        return [{}]  # 128-slot boards: 128-row workgroups, one board each
    out = [{"CATTUS_T64_CH": "2", "CATTUS_T64_LS": "0"}, {"CATTUS_T64_CH": "4", "CATTUS_T64_LS": "0"}]
    if d.board * d.board <= 63:
        out.append({"CATTUS_T64_CH": "4"})  # one barrier per layer
    return out


def make(name, blocks, dtype, switches=None, b=None, **kw):
    return HipEvaluator(b or blob(name, blocks), batch_size=MAX_BATCH, plane_words=NETS[name][4], dtype=dtype, switches=dict(switches or {}), **DTYPES[dtype][0], **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(NETS))
def test_the_fused_tail_has_the_head_conv_launchs_bits(name, dtype):
    pl, other = planes(name), planes(name, 21)
    for blocks in BLOCKS:
        for switches in shapes(name, dtype):
            with make(name, blocks, dtype, switches) as ref, make(name, blocks, dtype, switches, fused_heads=True) as ev:
                assert ev.tower_kernel() == ref.tower_kernel() == DTYPES[dtype][1]
                assert ev.fused_heads_effective() is True and ref.fused_heads_effective() is False
                for i, n in enumerate(LEAVES):
                    ev.eval(other[: max(n, 2)])  # hv now holds other leaves' head activations
                    want, got = ref.eval(pl[:n]), ev.eval(pl[:n])
                    print(name, dtype, blocks, switches, n, "logits differing:", int((bits(got[0]) != bits(want[0])).sum()), "values differing:", int((bits(got[1]) != bits(want[1])).sum()))
                    assert same(got, want), (name, dtype, blocks, switches, n)
                    assert ev.fused_heads_batches() == 2 * (i + 1)
                assert ref.fused_heads_batches() == 0
                assert ev.stats()["saturated"] == ref.stats()["saturated"]


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_every_entry_point_returns_the_same_bits(dtype):
    torch = pytest.importorskip("torch")
    name, blocks, n = "chess", 1, 5
    d, pl, other = desc(name, blocks), planes(name)[:5], planes(name, 21)
    rng = np.random.default_rng(3)
    legal_idx = np.stack([rng.choice(d.moves, size=24, replace=False) for _ in range(n)]).astype(np.uint16)
    legal_count = rng.integers(1, 25, size=n).astype(np.uint16)
    f32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    with make(name, blocks, dtype) as ref, make(name, blocks, dtype, fused_heads=True) as ev:
        want = ref.eval(pl)
        ev.eval(other[:7])
        assert same(ev.eval_legal(pl, legal_idx, legal_count), ref.eval_legal(pl, legal_idx, legal_count)), "eval_legal"
        # cattus_hip_apply: the leaf server
        ev.eval(other[:7])
        p, v = np.empty((n, d.moves), dtype=np.float32), np.empty((n,), dtype=np.float32)
        assert ev._lib.cattus_hip_apply(ev._h, np.ascontiguousarray(pl).ctypes.data_as(u64p), n, p.ctypes.data_as(f32p), v.ctypes.data_as(f32p)) == 0
        assert same((p, v), want), "apply"
        # submit + wait: one leaf each
        ev.eval(other[:7])
        tickets = [ev.submit(pl[i]) for i in range(n)]
        for i, t in enumerate(tickets):
            p1, v1 = ev.wait(t)
            assert same((p1, np.float32(v1)), (want[0][i], want[1][i])), ("wait", i)
        # device buffers, either lane
        dev = torch.device("cuda", 0)
        d_planes = torch.from_numpy(pl.copy().view(np.int64)).to(dev)
        d_other = torch.from_numpy(other[:7].copy().view(np.int64)).to(dev)
        for lane in (0, 1):
            pol = torch.zeros((7, d.moves), dtype=torch.float32, device=dev)
            val = torch.zeros((7,), dtype=torch.float32, device=dev)
            before = ev.fused_heads_batches()
            ev.eval_device(d_other.data_ptr(), 7, pol.data_ptr(), val.data_ptr(), ev.lane_stream(lane), lane=lane)
            ev.eval_device(d_planes.data_ptr(), n, pol.data_ptr(), val.data_ptr(), ev.lane_stream(lane), lane=lane)
            torch.cuda.synchronize()
            assert same((pol[:n].cpu().numpy(), val[:n].cpu().numpy()), want), ("eval_device_lane", lane)
            assert ev.fused_heads_batches() == before + 2
        assert ev.stats()["saturated"] == ref.stats()["saturated"] and ref.fused_heads_batches() == 0


def test_on_off_on_and_the_short_chain_pair_on_top():
    name, blocks = "hex7", 1
    pl, other = planes(name), planes(name, 21)
    for dtype in DTYPES:
        with make(name, blocks, dtype) as ref, make(name, blocks, dtype) as ev:
            want = ref.eval(pl[:17])
            assert ev.fused_heads_effective() is False
            for on, counted in ((True, 2), (False, 2), (True, 4)):
                ev.fused_heads(on)
                assert ev.fused_heads_effective() is on
                ev.eval(other[:17])
                assert same(ev.eval(pl[:17]), want), (dtype, on)
                assert ev.fused_heads_batches() == counted
            # cattus_hip_head_chain reads the hv the tail wrote
            ev.head_chain(MAX_BATCH)
            ev.eval(other[:17])
            assert same(ev.eval(pl[:17]), want) and ev.head_chain_batches() == 2 and ev.fused_heads_batches() == 6


@pytest.mark.parametrize("dtype", ["f16", "f16r_resident"])
def test_a_network_outside_the_f16_range_counts_the_same(dtype):
    """The stem's BatchNorm weight times 1e5 (tests/test_hip_parity.py's value, tests/test_f16r_resident_gpu.py's construction): activations leave
    the f16 range, are clamped and counted -- the same count, the same bits, with the heads in the tail."""
    name, blocks = "hex7", 2
    d = desc(name, blocks)
    t = seeded_tensors(d, 6)
    t["_conv1._bn.weight"] = t["_conv1._bn.weight"] * np.float32(1e5)
    t["_residual_blocks.0._conv1.weight"] = t["_residual_blocks.0._conv1.weight"] * np.float32(1e-3)
    b = pack_tensors(d, t)
    pl, other = planes(name), planes(name, 21)
    with make(name, blocks, dtype, b=b) as ref, make(name, blocks, dtype, b=b, fused_heads=True) as ev:
        ev.eval(other[:9])
        ref.eval(other[:9])
        assert same(ev.eval(pl[:9]), ref.eval(pl[:9]))
        assert ev.stats()["saturated"] == ref.stats()["saturated"] > 0


@pytest.mark.parametrize("dtype", ["f16", "f16r_resident"])
def test_observed_and_verified_passes_do_not_count_and_keep_their_outputs(dtype):
    name, blocks = "hex7", 1
    pl, other = planes(name)[:17], planes(name, 21)[:17]
    with make(name, blocks, dtype) as ref, make(name, blocks, dtype, fused_heads=True) as ev:
        point = ev.points() - 1
        ev.eval(other)
        a, pa, va = ev.tap(pl, point, outputs=True)
        b, pb, vb = ref.tap(pl, point, outputs=True)
        assert same((a, pa, va), (b, pb, vb)), "the head point"
        assert same(ev.tap(pl, point - 1, outputs=True), ref.tap(pl, point - 1, outputs=True)), "the tower's last layer"
        ra, tpa, tva = ev.trace(pl)
        rb, tpb, tvb = ref.trace(pl)
        assert ra.tobytes() == rb.tobytes() and same((tpa, tva), (tpb, tvb))
        assert ev.fused_heads_batches() == 1  # the one eval: an observed pass runs the per-layer twin and its head conv launch
        assert same(ev.eval(pl), (pa, va)) and ev.fused_heads_batches() == 2
        # a verified batch: its own pass is an ordinary one and counts once; the f32 shadow's pass does not
        ev.verify(1)
        ref.verify(1)
        ev.eval(other)
        assert same(ev.eval(pl), ref.eval(pl)) and ev.fused_heads_batches() == 4


def test_where_the_setting_does_nothing():
    # a per-layer plan, the resident towers that run the head convs in their tails always, and the resident f32 tower, which has no HEADS instance
    per_layer, f16r_layer = "conv3x3_mfma_v2_kernel", "conv3x3_f16r_kernel"
    cases = [(NetDesc(**CHESS, blocks=1, filters=128, vhc=8, phc=8), "f16r", f16r_layer), (desc("chess", 1), "bf16", "tower64_lds_kernel"),
             (desc("chess", 1), "f16x2", "tower64_split_kernel"), (desc("chess", 1), "f32_resident", "tower64_f32_kernel"),
             (desc("chess", 1), "f16", per_layer)]  # dtype f16 under tower_form auto: per layer
    pl = planes("chess")
    for d, dtype, kernel in cases:
        kw = {}
        b = seeded_blob(d, 77)
        args = dict(batch_size=MAX_BATCH, plane_words=1, dtype=dtype, switches={}, **kw)
        with HipEvaluator(b, **args) as ref, HipEvaluator(b, **args, fused_heads=True) as ev:
            assert ev.fused_heads_effective() is False, dtype
            before = ev.eval(pl[:17])
            ev.fused_heads(True)
            assert ev.fused_heads_effective() is False
            assert same(ev.eval(pl[:17]), before) and same(before, ref.eval(pl[:17])), dtype
            assert ev.fused_heads_batches() == 0
            assert ev.tower_kernel() == ref.tower_kernel() == kernel, dtype


def test_a_null_handle_is_refused_like_the_other_setters():
    lib = evaluator_module.load_library()
    k32, k64 = C.c_uint32(), C.c_uint64()
    want = lib.cattus_hip_head_chain(None, 1)
    assert want == -1  # CATTUS_E_INVALID
    assert lib.cattus_hip_fused_heads(None, 1) == want
    assert lib.cattus_hip_fused_heads_effective(None, C.byref(k32)) == want == lib.cattus_hip_head_chain_leaves(None, C.byref(k32))
    assert lib.cattus_hip_fused_heads_batches(None, C.byref(k64)) == want == lib.cattus_hip_head_chain_batches(None, C.byref(k64))
    with make("ttt", 0, "f16r_resident") as ev:
        assert lib.cattus_hip_fused_heads_effective(ev._h, None) == want and lib.cattus_hip_fused_heads_batches(ev._h, None) == want
    ev.close()
    with pytest.raises(Exception):
        ev.fused_heads(True)  # a closed evaluator: the binding's own refusal, as for every other method


def test_the_self_player_writes_the_same_records(tmp_path, monkeypatch):
    from cattus_amd import selfplay as sp

    seen = []

    class Recording(evaluator_module.HipEvaluator):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            seen.append((kw.get("fused_heads"), self.fused_heads_effective()))

    monkeypatch.setattr(evaluator_module, "HipEvaluator", Recording)
    model = tmp_path / "model.cattus"
    model.write_bytes(seeded_blob(NetDesc(**hex_game(4), blocks=1, filters=16, vhc=4, phc=4), 9))
    records = {}
    for fused in (False, True):
        cfg = {
            "model": {"inference": {"engine": "hip", "device": 0, "dtype": "f16r_resident", "fused_heads": fused}, "batch_size": 4},
            "mcts": {"sim_num": 8, "explore_factor": 1.41421, "temperature_policy": [[9999, 0.0]], "prior_noise_alpha": 0.0, "prior_noise_epsilon": 0.0, "cache_size": 1000},
            "threads": 1,
            "concurrent_games": 1,
        }
        out = tmp_path / str(fused)
        out.mkdir()
        (tmp_path / f"{fused}.json").write_text(json.dumps(cfg))
        sp.main(["--game", "hex4", "--model1-path", str(model), "--model2-path", str(model), "--games-num", "2", "--out-dir1", str(out / "o1"), "--out-dir2",
                 str(out / "o2"), "--summary-file", str(out / "summary.json"), "--config-file", str(tmp_path / f"{fused}.json")])
        s = json.loads((out / "summary.json").read_text())
        assert s["player1_wins"] + s["player2_wins"] + s["draws"] == 2 and s["metrics"]["model.activation_count"] > 0
        records[fused] = sorted(p.read_bytes() for p in out.rglob("*") if p.is_file() and p.name != "summary.json")
    assert seen == [(False, False), (True, True)], seen
    assert len(records[False]) > 2 and records[True] == records[False]
