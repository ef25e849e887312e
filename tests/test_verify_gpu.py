"""Live verification against a shadow f32 tower (cattus_hip_verify): the comparison kernel alone, the evaluator's sticky record, when a
batch is verified, what the caller must not notice, the refusals, and the self-player's key.

Everything here is deterministic, so every number is held to exact equality with test_verify_rule.py's float64 restatement
(records_restated: what the kernel writes per leaf; fold_restated: what the evaluator keeps), computed from this evaluator's outputs and
those of a separate dtype f32 evaluator of the same blob -- which is what the shadow is: the same create path, the same max_batch, so the
same plan and the same bits.  No bound on any difference is set here except the bar itself (leaves_outside), and that only where the
existing suite already holds the dtype to it (f16x2: 0) or shows it to fail it (bf16 on shape A: >= 1)."""

import ctypes as C
import json
import threading

import numpy as np
import pytest

from cattus_amd import selfplay as sp
from cattus_amd.evaluator import CattusHipError, HipEvaluator, compare_outputs
from cattus_amd.weights import CHESS, NetDesc, hex_game, pack_tensors, seeded_blob, seeded_tensors, simple_desc

import test_many_planes_gpu as many
from test_many_planes_gpu import random_planes
from test_verify_rule import F32_MIN, fold_restated, random_pairs, records_restated

pytestmark = pytest.mark.gpu

CATTUS_E_INVALID, CATTUS_E_UNSUPPORTED, CATTUS_E_STATE = -1, -2, -5
FLOATS = ("max_dlogit", "logit", "logit_ref", "max_dvalue", "value", "value_ref")


def assert_record(stats: dict, fold: dict):
    """The evaluator's sticky record equals the restated fold, floats by their bits."""
    for k in ("batches", "leaves", "leaves_outside", "move"):
        assert stats[k] == fold[k], (k, stats, fold)
    for k in FLOATS:
        assert np.float32(stats[k]).tobytes() == np.float32(fold[k]).tobytes(), (k, stats, fold)


def fold_batches(batches, into=None):
    """fold_restated over [(own outputs, f32 outputs)] in order."""
    for (p, v), (rp, rv) in batches:
        into = fold_restated(records_restated(p, rp, v, rv), p, rp, v, rv, into=into)
    return into


# ---------------------------------------------------------------------------------------- 1. the kernel alone


@pytest.mark.parametrize("n,M", [(1, 9), (5, 67), (3, 1880), (130, 52), (257, 1880)])
def test_comparison_kernel_writes_the_restated_records(n, M):
    """A wave-partial row (M = 9, 52), rows that do not start on a 16-byte boundary (M = 67 and 9: 268 and 36 bytes apart), whole rows of
    vectors (1880), more than one workgroup (130, 257 leaves: four leaves each); planted: one maximum at two indices (the lower is
    reported), NaN, inf, inf against inf, f32::MIN against itself and against a finite logit, identical rows, a NaN value, opposite
    values.  Every record equals the restatement's bytes, twice."""
    a, b = random_pairs(n * M, seed=1000 + n)
    pa, pb = a.reshape(n, M).copy(), b.reshape(n, M).copy()
    rng = np.random.default_rng(n * M)
    vb = np.tanh(rng.normal(size=n)).astype(np.float32)
    va = (vb.astype(np.float64) * (1 + 10.0 ** rng.uniform(-7, -3.5, n))).astype(np.float32)
    pa[0, [M - 1, M // 2]], pb[0, [M - 1, M // 2]] = 80.0, 0.0  # a tie: move M // 2
    pa[0, 0] = pb[0, 0] = F32_MIN
    pa[0, 2] = np.nan
    if n >= 3:
        pa[1, M - 1] = np.inf
        pa[2, 0] = pb[2, 0] = -np.inf
        pb[2, 1] = F32_MIN
    if n >= 5:
        pa[3] = pb[3]
        va[3] = vb[3]
        va[4] = np.nan
        pa[4] = pb[4]
    if n >= 130:
        va[n - 1], vb[n - 1] = 1.0, -1.0
        pa[n - 2, M - 1], pb[n - 2, M - 1] = F32_MIN, 3.0
    want = records_restated(pa, pb, va, vb)
    assert want["move"][0] == M // 2 and want["max_dlogit"][0] == 80.0 and want["flags"][0] & 1
    got = compare_outputs(pa, pb, va, vb)
    assert got.tobytes() == want.tobytes(), [(i, got[i], want[i]) for i in range(n) if got[i].tobytes() != want[i].tobytes()][:5]
    assert compare_outputs(pa, pb, va, vb).tobytes() == got.tobytes()
    if n >= 5:
        assert set(want["flags"]) >= {0, 1, 3}


# ---------------------------------------------------------------------------------------- 2. f16x2 against its shadow

NETS = {
    # id: (desc, plane words, n, max_batch, the kernel the issue names)
    "chess2x64": (NetDesc(**CHESS, blocks=2, filters=64, vhc=8, phc=8), 1, 9, 16, "tower64_split_kernel"),
    "chess1x128": (NetDesc(**CHESS, blocks=1, filters=128, vhc=8, phc=8), 1, 132, 132, "tower_wino4_kernel"),
    "hex11_2x8": (NetDesc(**hex_game(11), blocks=2, filters=8, vhc=4, phc=4), 2, 21, 21, None),
}


@pytest.mark.parametrize("net", sorted(NETS))
def test_f16x2_record_equals_the_restatement_and_the_caller_notices_nothing(net):
    d, words, n, max_batch, kernel = NETS[net]
    blob = seeded_blob(d, 23)
    planes = random_planes(d, words, n, 14)
    with HipEvaluator(blob, batch_size=max_batch, plane_words=words, dtype="f16x2", switches={}) as ev:
        plain, plain_kernel = ev.eval(planes), ev.tower_kernel()
    with HipEvaluator(blob, batch_size=max_batch, plane_words=words, dtype="f32", switches={}) as ev:
        ref = ev.eval(planes)
    with HipEvaluator(blob, batch_size=max_batch, plane_words=words, dtype="f16x2", switches={}, verify_every=1) as ev:
        with pytest.raises(CattusHipError) as err:
            ev.verify_worst_planes()
        assert err.value.status == CATTUS_E_STATE
        got = ev.eval(planes)
        assert ev.tower_kernel() == plain_kernel and (kernel is None or plain_kernel == kernel)
        vs, worst = ev.verify_stats(), ev.verify_worst_planes()
        assert ev.stats()["batches"] == 1 and ev.stats()["positions"] == n
    assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()
    fold = fold_batches([(got, ref)])
    print(net, vs)
    assert vs["every"] == 1 and vs["leaves"] == n and vs["leaves_outside"] == 0
    assert_record(vs, fold)
    assert (worst == planes[fold["leaf"]]).all()


# ---------------------------------------------------------------------------------------- 3. bf16, 4. f16 saturated


def test_bf16_on_many_planes_is_counted_outside_the_bar():
    d, blob, words, planes, _, _ = many.case("A")
    ref = many.f32_outputs("A")
    with HipEvaluator(blob, batch_size=len(planes), plane_words=words, dtype="bf16", switches={}, verify_every=1) as ev:
        got = ev.eval(planes)
        vs, worst = ev.verify_stats(), ev.verify_worst_planes()
    fold = fold_batches([(got, ref)])
    print("bf16 A", vs)
    assert_record(vs, fold)
    assert vs["leaves"] == len(planes) and vs["leaves_outside"] >= 1
    assert (worst == planes[fold["leaf"]]).all()


def test_f16_on_a_saturating_network_reports_both_counters():
    """test_f16_range_on_the_large_tile's network at stem BatchNorm scale 1e5: `saturated` fires, and the shadow says by how much the
    outputs are off.  The numbers are printed, none is bounded."""
    d = NetDesc(**CHESS, blocks=2, filters=64, vhc=8, phc=8)
    planes = random_planes(d, 1, 16, 6)
    t = seeded_tensors(d, 6)
    t["_conv1._bn.weight"] = t["_conv1._bn.weight"] * np.float32(1e5)
    t["_residual_blocks.0._conv1.weight"] = t["_residual_blocks.0._conv1.weight"] * np.float32(1e-3)
    blob = pack_tensors(d, t)
    with HipEvaluator(blob, batch_size=16, plane_words=1, dtype="f32", switches={}) as ev:
        ref = ev.eval(planes)
    with HipEvaluator(blob, batch_size=16, plane_words=1, dtype="f16", switches={"CATTUS_CONV_CB": "2"}, verify_every=1) as ev:
        got = ev.eval(planes)
        vs, sat = ev.verify_stats(), ev.stats()["saturated"]
    fold = fold_batches([(got, ref)])
    print("f16 saturating: saturated %d, %s" % (sat, vs))
    assert sat > 0
    assert_record(vs, fold)


# ---------------------------------------------------------------------------------------- 5. scheduling


@pytest.fixture(scope="module")
def small():
    """chess 2 x 64, 16 leaves, their f16x2 and f32 outputs: made once, shared, never written to."""
    d = NetDesc(**CHESS, blocks=2, filters=64, vhc=8, phc=8)
    blob = seeded_blob(d, 27)
    planes = random_planes(d, 1, 16, 15)
    outs = {}
    for dtype in ("f16x2", "f32"):
        with HipEvaluator(blob, batch_size=16, plane_words=1, dtype=dtype, switches={}) as ev:
            outs[dtype] = ev.eval(planes)
    for a in (planes, *outs["f16x2"], *outs["f32"]):
        a.setflags(write=False)
    return d, blob, planes, outs["f16x2"], outs["f32"]


def test_every_third_batch_is_verified_and_off_keeps_the_record(small):
    d, blob, planes, own, ref = small
    sizes = [4, 1, 7, 2, 5, 3, 6]
    part = lambda o, at, k: (o[0][at:at + k], o[1][at:at + k])
    with HipEvaluator(blob, batch_size=16, plane_words=1, dtype="f16x2", switches={}, verify_every=3) as ev:
        verified, at = [], 0
        for i, k in enumerate(sizes):
            p, v = ev.eval(planes[at:at + k])
            assert p.tobytes() == own[0][at:at + k].tobytes() and v.tobytes() == own[1][at:at + k].tobytes()
            if i % 3 == 0:
                verified.append((part(own, at, k), part(ref, at, k)))
            at = (at + k) % 9
        vs = ev.verify_stats()
        fold = fold_batches(verified)
        assert vs["every"] == 3 and vs["batches"] == 3 and vs["leaves"] == 4 + 2 + 6 and vs["leaves_outside"] == 0
        assert_record(vs, fold)
        st = ev.stats()
        assert st["batches"] == 7 and st["positions"] == sum(sizes) and st["full_batches"] == 0
        ev.verify(0)
        for k in (5, 16):
            ev.eval(planes[:k])
        off = ev.verify_stats()
        assert off["every"] == 0 and {k: off[k] for k in off if k != "every"} == {k: vs[k] for k in vs if k != "every"}
        assert (ev.verify_worst_planes() == ev.verify_worst_planes()).all()
        ev.verify(2)  # tickets go on from 7: of the next four batches the second and the fourth are verified
        for i, k in enumerate((2, 3, 4, 5)):
            ev.eval(planes[8:8 + k])
            if i % 2 == 1:
                verified.append((part(own, 8, k), part(ref, 8, k)))
        on = ev.verify_stats()
        assert on["every"] == 2 and on["batches"] == 5 and on["leaves"] == 12 + 3 + 5
        assert_record(on, fold_batches(verified))
        assert ev.stats()["batches"] == 13 and ev.stats()["full_batches"] == 1


def test_the_leaf_server_and_the_legal_softmax_are_verified_too(small):
    d, blob, planes, own, ref = small
    rng = np.random.default_rng(8)
    legal_idx = rng.integers(0, d.moves, size=(6, 8)).astype(np.uint16)
    legal_cnt = rng.integers(1, 9, size=6).astype(np.uint16)
    with HipEvaluator(blob, batch_size=6, plane_words=1, dtype="f16x2", switches={}) as ev:
        want_probs, want_v = ev.eval_legal(planes[:6], legal_idx, legal_cnt)
    # flush_us of five seconds: a batch runs when it is full, and apply() of max_batch leaves fills exactly one
    with HipEvaluator(blob, batch_size=6, plane_words=1, dtype="f16x2", switches={}, flush_us=5_000_000, verify_every=1) as ev:
        f32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
        batches = []
        for at in (0, 6):
            p, v = np.empty((6, d.moves), dtype=np.float32), np.empty(6, dtype=np.float32)
            chunk = np.ascontiguousarray(planes[at:at + 6])
            assert ev._lib.cattus_hip_apply(ev._h, chunk.ctypes.data_as(u64p), 6, p.ctypes.data_as(f32p), v.ctypes.data_as(f32p)) == 0
            assert p.tobytes() == own[0][at:at + 6].tobytes() and v.tobytes() == own[1][at:at + 6].tobytes()
            batches.append(((p, v), (ref[0][at:at + 6], ref[1][at:at + 6])))
        vs = ev.verify_stats()
        assert vs["batches"] == 2 and vs["leaves"] == 12 and vs["leaves_outside"] == 0
        assert_record(vs, fold_batches(batches))
        probs, v = ev.eval_legal(planes[:6], legal_idx, legal_cnt)
        assert probs.tobytes() == want_probs.tobytes() and v.tobytes() == want_v.tobytes()
        vs = ev.verify_stats()
        assert vs["batches"] == 3 and vs["leaves"] == 18 and vs["leaves_outside"] == 0
        assert_record(vs, fold_batches(batches + [batches[0]]))  # the logits stayed on the device and were compared there
        assert ev.stats()["batches"] == 3 and ev.stats()["positions"] == 18


def test_two_threads_on_the_two_lanes(small):
    d, blob, planes, own, ref = small
    errors = []
    with HipEvaluator(blob, batch_size=16, plane_words=1, dtype="f16x2", switches={}, verify_every=1) as ev:
        def work(at, k):
            try:
                for _ in range(6):
                    p, v = ev.eval(planes[at:at + k])
                    assert p.tobytes() == own[0][at:at + k].tobytes() and v.tobytes() == own[1][at:at + k].tobytes()
            except BaseException as exc:  # noqa: BLE001 - reported by the main thread
                errors.append(exc)

        threads = [threading.Thread(target=work, args=a) for a in ((0, 7), (5, 11))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        vs, st = ev.verify_stats(), ev.stats()
    assert not errors, errors
    assert st["batches"] == 12 and st["positions"] == 6 * (7 + 11)
    assert vs["batches"] == 12 and vs["leaves"] == st["positions"] and vs["leaves_outside"] == 0
    # whichever batch came first, the largest difference is the largest over the leaves 0 .. 15 that were evaluated
    whole = records_restated(own[0], ref[0], own[1], ref[1])
    assert np.float32(vs["max_dlogit"]) == whole["max_dlogit"].max() and np.float32(vs["max_dvalue"]) == whole["dvalue"].max()


# ---------------------------------------------------------------------------------------- 6. the one-launch tower's give-up path


@pytest.mark.parametrize("blocks,filters,n,must_give_up", [(1, 128, 132, False), (6, 256, 256, True)])
def test_a_batch_the_one_launch_tower_gives_up_on_is_counted_once(blocks, filters, n, must_give_up):
    """CATTUS_WINO_SPIN=1: a hand-off wait of the one-launch tower may give up, and that batch is run again on the per-layer launches.
    On the small shape (two layers, 66 workgroups) a wait need not give up; on test_hip_parity's shape for this path (12 layers x 256
    workgroups x 3 passes) one does, which the evaluator's kernel name shows afterwards.  Either way every batch is verified once, from
    the run whose outputs the caller gets, which are the per-layer bits."""
    d = NetDesc(**CHESS, blocks=blocks, filters=filters, vhc=8, phc=8)
    words, max_batch = 1, n
    blob = seeded_blob(d, 23)
    planes = random_planes(d, words, n, 14)
    with HipEvaluator(blob, batch_size=max_batch, plane_words=words, dtype="f16x2", switches={"CATTUS_WINO_PERSIST": "0"}) as ev:
        want = ev.eval(planes)
    with HipEvaluator(blob, batch_size=max_batch, plane_words=words, dtype="f32", switches={}) as ev:
        ref = ev.eval(planes)
    with HipEvaluator(blob, batch_size=max_batch, plane_words=words, dtype="f16x2", switches={"CATTUS_WINO_SPIN": "1"}, verify_every=1) as ev:
        for _ in range(3):
            got = ev.eval(planes)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        vs, st = ev.verify_stats(), ev.stats()
        print("give-up path: now on", ev.tower_kernel(), vs)
        assert not must_give_up or ev.tower_kernel() == "conv3x3_wino4_kernel"
    assert st["batches"] == 3 and st["positions"] == 3 * n
    assert vs["batches"] == 3 and vs["leaves"] == 3 * n and vs["leaves_outside"] == 0
    assert_record(vs, fold_batches([(want, ref)] * 3))


# ---------------------------------------------------------------------------------------- 7. refusals


def test_refusals(small):
    d, blob, planes, _, _ = small
    with HipEvaluator(blob, batch_size=4, plane_words=1, dtype="f32", switches={}) as ev:
        with pytest.raises(CattusHipError) as err:
            ev.verify(1)
        assert err.value.status == CATTUS_E_UNSUPPORTED
    with pytest.raises(CattusHipError) as err:
        HipEvaluator(blob, batch_size=4, plane_words=1, dtype="f32", switches={}, verify_every=2)
    assert err.value.status == CATTUS_E_UNSUPPORTED
    sd = simple_desc(3, 3, 9)
    with HipEvaluator(seeded_blob(sd, 2), batch_size=4, plane_words=1, dtype="f16x2", switches={}) as ev:
        with pytest.raises(CattusHipError) as err:
            ev.verify(1)
        assert err.value.status == CATTUS_E_UNSUPPORTED
    other_shape = NetDesc(**CHESS, blocks=1, filters=64, vhc=8, phc=8)
    with HipEvaluator(blob, batch_size=4, plane_words=1, dtype="f16x2", switches={}) as ev:
        for wrong in (seeded_blob(d, 28), seeded_blob(other_shape, 27)):
            with pytest.raises(CattusHipError) as err:
                ev.verify(1, blob=wrong)
            assert err.value.status == CATTUS_E_INVALID
        from cattus_amd.evaluator import VerifyStats

        assert ev._lib.cattus_hip_verify_stats(ev._h, C.byref(VerifyStats(struct_size=0))) == CATTUS_E_INVALID
        with pytest.raises(CattusHipError) as err:
            ev.verify_worst_planes()
        assert err.value.status == CATTUS_E_STATE
        assert ev.verify_stats()["every"] == 0 and ev.verify_stats()["leaves"] == 0
        ev.verify(1)  # and the right blob is taken
        ev.eval(planes[:3])
        assert ev.verify_stats()["leaves"] == 3


# ---------------------------------------------------------------------------------------- 8. the self-player


def test_self_player_reports_what_the_shadow_found(tmp_path, capsys):
    """model.inference.verify_every in the engine JSON: four more metrics; without the key exactly the old summary, and the same record
    files either way.  One search thread, one game at a time, one leaf in flight: no position is evaluated twice, so the leaves that
    were evaluated -- all verified -- are the cache's misses."""
    d = NetDesc(**hex_game(5), blocks=2, filters=16, vhc=4, phc=4)
    model = tmp_path / "model.cattus"
    model.write_bytes(seeded_blob(d, 9))
    summaries, files = {}, {}
    for tag, extra in (("plain", {}), ("verified", {"verify_every": 1})):
        cfg = {
            "model": {"inference": {"engine": "hip", "device": 0, "dtype": "f16x2", **extra}, "batch_size": 8},
            "mcts": {"sim_num": 10, "explore_factor": 1.41421, "temperature_policy": [[9999, 0.0]], "prior_noise_alpha": 0.0,
                     "prior_noise_epsilon": 0.0, "cache_size": 1000},
            "threads": 1,
            "concurrent_games": 1,
        }
        (tmp_path / f"{tag}.json").write_text(json.dumps(cfg))
        sp.main(["--game", "hex5", "--model1-path", str(model), "--model2-path", str(model), "--games-num", "2", "--out-dir1", str(tmp_path / tag / "o1"),
                 "--out-dir2", str(tmp_path / tag / "o2"), "--summary-file", str(tmp_path / f"{tag}_summary.json"), "--config-file", str(tmp_path / f"{tag}.json")])
        summaries[tag] = json.loads((tmp_path / f"{tag}_summary.json").read_text())
        files[tag] = {f"{o}/{f.name}": f.read_bytes() for o in ("o1", "o2") for f in sorted((tmp_path / tag / o).iterdir())}
    old_keys = {"model.activation_count", "model.run_duration", "mcts.search_duration", "cache.hits", "cache.misses", "node_evals", "evals_per_sec",
                "games_seconds", "model.saturated"}
    new_keys = {"model.verified_leaves", "model.leaves_outside_bar", "model.max_dlogit", "model.max_dvalue"}
    assert set(summaries["plain"]) == set(summaries["verified"]) == {"player1_wins", "player2_wins", "draws", "metrics"}
    assert set(summaries["plain"]["metrics"]) == old_keys
    m = summaries["verified"]["metrics"]
    assert set(m) == old_keys | new_keys
    print("self-player:", {k: m[k] for k in sorted(new_keys)}, "cache.misses", m["cache.misses"])
    assert m["model.verified_leaves"] == m["cache.misses"] > 0
    assert m["model.leaves_outside_bar"] == 0
    assert files["plain"] and files["plain"] == files["verified"]
    assert "outside" not in capsys.readouterr().err
