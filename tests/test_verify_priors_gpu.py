"""The priors part of live verification (cattus_hip_verify_prior_stats): the comparison kernel alone, the evaluator's sticky record, what
the caller must not notice, the paths without legal moves, two lanes, the refusals, the one-launch tower's give-up path and the
self-player's key.

Everything here is deterministic, so every number is held to exact equality with test_prior_rule.py's restatement (records_restated: what
the kernel writes per leaf; fold_restated: what the evaluator keeps), computed from the eval_legal outputs of two independent evaluators:
one of this dtype with verification off and a dtype f32 one of the same blob -- which is what the shadow is.  No bound on any difference
is set here: the issue sets none."""

import ctypes as C
import functools
import json
import subprocess
import threading

import numpy as np
import pytest

from cattus_amd import selfplay as sp
from cattus_amd.evaluator import CattusHipError, HipEvaluator, PriorStats, compare_priors
from cattus_amd.weights import CHESS, TTT, NetDesc, hex_game, seeded_blob, simple_desc

import test_verify_rule as logit_rule
from test_many_planes_gpu import random_planes
from test_prior_rule import edge_rows, fold_restated, fold_values_restated, records_restated, softmax_rows

pytestmark = pytest.mark.gpu

CATTUS_E_INVALID, CATTUS_E_UNSUPPORTED, CATTUS_E_STATE = -1, -2, -5
INTS = ("batches", "batches_without_legal", "leaves", "top1_flips", "nonfinite", "empty", "value_leaves", "tv_hist")


def f32_bits(x) -> bytes:
    return np.float32(x).tobytes()


class Restated:
    """The sticky prior record restated on the host, batch by batch."""

    def __init__(self):
        self.s, self.values, self.batches, self.without_legal, self.worst = None, (0, 0.0), 0, 0, None

    def legal_batch(self, planes, legal_idx, legal_cnt, own, ref):
        (pa, va), (pb, vb) = own, ref
        rec = records_restated(pa, pb, legal_cnt, va, vb)
        self.values = fold_values_restated(va, vb, self.values)
        self.s = fold_restated(rec, into=self.s)
        self.batches += 1
        if self.s["holder"] is not None:
            i = self.s["holder"]
            self.worst = dict(planes=planes[i].copy(), legal_idx=legal_idx[i, : rec[i]["count"]].copy(), top=int(rec[i]["top_a"]), top_ref=int(rec[i]["top_b"]))
        return rec

    def plain_batch(self, va, vb):
        self.values = fold_values_restated(va, vb, self.values)
        self.without_legal += 1

    def check(self, stats: dict):
        s = self.s or fold_restated([])
        want = dict(batches=self.batches, batches_without_legal=self.without_legal, leaves=s["leaves"], top1_flips=s["top1_flips"], nonfinite=s["nonfinite"],
                    empty=s["empty"], value_leaves=self.values[0], tv_hist=s["tv_hist"])
        assert {k: stats[k] for k in INTS} == want, (stats, want)
        for k in ("max_tv", "max_regret"):
            assert f32_bits(stats[k]) == f32_bits(s[k]), (k, stats, s)
        # float64 sums, folded leaf by leaf in the order the evaluator folds them: the same bits
        assert (stats["sum_tv"], stats["sum_regret"], stats["sum_dvalue"]) == (s["sum_tv"], s["sum_regret"], self.values[1]), (stats, s, self.values)
        summed = s["leaves"] - s["nonfinite"] - s["empty"]
        assert stats["tv_mean"] == (s["sum_tv"] / summed if summed else 0.0) and stats["regret_mean"] == (s["sum_regret"] / summed if summed else 0.0)
        assert stats["dvalue_mean"] == (self.values[1] / self.values[0] if self.values[0] else 0.0)


# ---------------------------------------------------------------------------------------- 1. the kernel alone


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("L", [1, 9, 25, 64, 224, 1024])
def test_prior_kernel_writes_the_restated_records(n, L):
    """Less than a workgroup, exactly one, one leaf and one whole workgroup more (four leaves each); rows of one float, odd rows that do
    not start on a 16-byte boundary (9, 25), whole waves (64), several strides of the lanes (224, 1024).  The CPU test's edge rows first,
    random rows behind them.  Every record equals the restatement's bytes, twice."""
    rng = np.random.default_rng(100 * n + L)
    edges = edge_rows(L, seed=n)
    pick = [edges[i % len(edges)] for i in rng.permutation(len(edges))[: max(1, n - 1)]]
    pa, pb = softmax_rows(rng, n, L)
    cnt = rng.integers(0, L + 1, size=n).astype(np.uint16)
    vb = np.tanh(rng.normal(size=n)).astype(np.float32)
    va = (vb * (1 + 2.0 ** -9)).astype(np.float32)
    for i, (_, ea, eb, c, ua, ub) in enumerate(pick[:n]):
        pa[i], pb[i], cnt[i], va[i], vb[i] = ea, eb, c, ua, ub
    want = records_restated(pa, pb, cnt, va, vb)
    got = compare_priors(pa, pb, cnt, va, vb)
    assert got.dtype.itemsize == 32
    assert got.tobytes() == want.tobytes(), [(i, got[i], want[i]) for i in range(n) if got[i].tobytes() != want[i].tobytes()][:5]
    assert compare_priors(pa, pb, cnt, va, vb).tobytes() == got.tobytes()


def test_prior_kernel_on_every_edge_row():
    """All of test_prior_rule.py's edge rows of one stride in one launch, so that every named case runs on the device whatever the
    parametrised test drew."""
    for L in (25, 224):
        edges = edge_rows(L)
        pa, pb = np.stack([e[1] for e in edges]), np.stack([e[2] for e in edges])
        cnt = np.array([e[3] for e in edges], dtype=np.uint16)
        va, vb = np.array([e[4] for e in edges], dtype=np.float32), np.array([e[5] for e in edges], dtype=np.float32)
        want = records_restated(pa, pb, cnt, va, vb)
        assert {int(f) & 7 for f in want["flags"]} >= {0, 1, 2, 4}
        got = compare_priors(pa, pb, cnt, va, vb)
        assert got.tobytes() == want.tobytes(), [(edges[i][0], got[i], want[i]) for i in range(len(edges)) if got[i].tobytes() != want[i].tobytes()][:5]


# ---------------------------------------------------------------------------------------- 2., 3. through the evaluator

NETS = {
    # id: (desc, plane words, legal stride, max_batch)
    "hex5_1x32": (NetDesc(**hex_game(5), blocks=1, filters=32, vhc=4, phc=4), 2, 25, 8),  # 2 plane words, M = 25, an odd stride
    "chess1x64": (NetDesc(**CHESS, blocks=1, filters=64, vhc=8, phc=8), 1, 40, 8),  # M = 1880: logit rows start on 128-byte lines
    "ttt1x32": (NetDesc(**TTT, blocks=1, filters=32, vhc=4, phc=4), 1, 9, 8),  # M = 9
}


def legal_batches(d, words, L, max_batch, seed):
    """[(planes, legal_idx, legal_count)]: batch sizes 1, 5 and max_batch; counts all 1, all 2, all L, and mixed per leaf (0 among them)."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (n, counts) in enumerate([(1, "L"), (5, 1), (max_batch, 2), (5, "L"), (max_batch, "mixed"), (1, 1)]):
        idx = np.stack([rng.permutation(d.moves)[:L] for _ in range(n)]).astype(np.uint16)
        if counts == "mixed":
            cnt = rng.integers(1, L + 1, size=n).astype(np.uint16)
            cnt[1], cnt[2] = 0, L
        else:
            cnt = np.full(n, L if counts == "L" else counts, dtype=np.uint16)
        out.append((random_planes(d, words, n, seed + k), idx, cnt))
    return out


@functools.lru_cache(maxsize=None)
def through_the_evaluator(net, dtype):
    """Every batch of legal_batches through a plain evaluator of `dtype`, a dtype f32 one and a verifying one: computed once, shared."""
    d, words, L, max_batch = NETS[net]
    blob = seeded_blob(d, 31)
    batches = legal_batches(d, words, L, max_batch, 40)
    out = dict(batches=batches)
    for tag, dt, every in (("plain", dtype, 0), ("f32", "f32", 0), ("verified", dtype, 1)):
        with HipEvaluator(blob, batch_size=max_batch, plane_words=words, dtype=dt, switches={}, verify_every=every) as ev:
            if every:
                with pytest.raises(CattusHipError) as err:
                    ev.verify_worst_prior()
                out["before"] = err.value.status
            out[tag] = [ev.eval_legal(*b) for b in batches]
            if every:
                out.update(prior_stats=ev.verify_prior_stats(), worst=ev.verify_worst_prior(), verify_stats=ev.verify_stats(), stats=ev.stats())
                with pytest.raises(CattusHipError) as err:
                    ev.verify_worst_prior(cap=len(out["worst"]["legal_idx"]) - 1)
                out["short_cap"] = err.value.status
            else:
                out[tag + "_logits"] = [ev.eval(b[0]) for b in batches]
                out[tag + "_stats"] = ev.stats()
    return out


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("net", sorted(NETS))
def test_prior_record_equals_the_fold_of_restated_records(net, dtype):
    r = through_the_evaluator(net, dtype)
    restated = Restated()
    for b, own, ref in zip(r["batches"], r["plain"], r["f32"]):
        restated.legal_batch(*b, own, ref)
    print(net, dtype, r["prior_stats"])
    restated.check(r["prior_stats"])
    assert r["prior_stats"]["leaves"] == sum(len(b[0]) for b in r["batches"]) and r["prior_stats"]["empty"] == 1 and r["prior_stats"]["nonfinite"] == 0
    assert r["before"] == CATTUS_E_STATE and r["short_cap"] == CATTUS_E_INVALID
    w, want = r["worst"], restated.worst
    assert (w["planes"] == want["planes"]).all() and w["legal_idx"].tolist() == want["legal_idx"].tolist() and (w["top"], w["top_ref"]) == (want["top"], want["top_ref"])


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("net", sorted(NETS))
def test_nothing_else_moves(net, dtype):
    """probs and value of every verified batch are the plain evaluator's bits; verify_stats is what the logit rule alone makes of the same
    batches (test_verify_rule.py's restatement, on the logits the two plain evaluators return); cattus_stats counts what it counted."""
    r = through_the_evaluator(net, dtype)
    for got, plain in zip(r["verified"], r["plain"]):
        assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()
    fold = None
    for (p, v), (rp, rv) in zip(r["plain_logits"], r["f32_logits"]):
        fold = logit_rule.fold_restated(logit_rule.records_restated(p, rp, v, rv), p, rp, v, rv, into=fold)
    vs = r["verify_stats"]
    for k in ("batches", "leaves", "leaves_outside", "move"):
        assert vs[k] == fold[k], (k, vs, fold)
    for k in ("max_dlogit", "logit", "logit_ref", "max_dvalue", "value", "value_ref"):
        assert f32_bits(vs[k]) == f32_bits(fold[k]), (k, vs, fold)
    n_batches, n_leaves = len(r["batches"]), sum(len(b[0]) for b in r["batches"])
    assert (r["stats"]["batches"], r["stats"]["positions"]) == (n_batches, n_leaves)
    assert (r["plain_stats"]["batches"], r["plain_stats"]["positions"]) == (2 * n_batches, 2 * n_leaves)  # eval_legal and eval of each


# ---------------------------------------------------------------------------------------- 4. paths without legal moves


def test_batches_without_legal_moves_feed_the_value_part_alone():
    d, words, _, _ = NETS["chess1x64"]
    blob = seeded_blob(d, 31)
    planes = random_planes(d, words, 11, 77)
    vals = {}
    for dt in ("bf16", "f32"):
        with HipEvaluator(blob, batch_size=4, plane_words=words, dtype=dt, switches={}) as ev:
            vals[dt] = np.concatenate([ev.eval(planes[at:at + 4])[1] for at in (0, 4, 8)])
    restated = Restated()
    # flush_us of five seconds: a server batch runs when it is full, and max_batch leaves fill exactly one
    with HipEvaluator(blob, batch_size=4, plane_words=words, dtype="bf16", switches={}, flush_us=5_000_000, verify_every=1) as ev:
        ev.eval(planes[:3])
        restated.plain_batch(vals["bf16"][:3], vals["f32"][:3])
        f32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
        p, v = np.empty((4, d.moves), dtype=np.float32), np.empty(4, dtype=np.float32)
        chunk = np.ascontiguousarray(planes[3:7])
        assert ev._lib.cattus_hip_apply(ev._h, chunk.ctypes.data_as(u64p), 4, p.ctypes.data_as(f32p), v.ctypes.data_as(f32p)) == 0
        assert v.tobytes() == vals["bf16"][3:7].tobytes()
        restated.plain_batch(vals["bf16"][3:7], vals["f32"][3:7])
        tickets = [ev.submit(planes[i]) for i in range(7, 11)]
        waited = [ev.wait(t)[1] for t in tickets]
        assert np.array(waited, dtype=np.float32).tobytes() == vals["bf16"][7:11].tobytes()
        restated.plain_batch(vals["bf16"][7:11], vals["f32"][7:11])
        ps = ev.verify_prior_stats()
        with pytest.raises(CattusHipError) as err:
            ev.verify_worst_prior()
        assert err.value.status == CATTUS_E_STATE
    print("without legal moves:", ps)
    assert ps["batches_without_legal"] == 3 and ps["value_leaves"] == 11 and ps["leaves"] == 0 and ps["batches"] == 0
    restated.check(ps)


# ---------------------------------------------------------------------------------------- 5. every third batch, two lanes


def test_every_third_batch_from_two_threads():
    """Thread A sends its batch of 3 leaves six times, thread B its batch of 5: twelve tickets, four verified, which four is the
    scheduler's.  verify_stats' leaves = 3 a + 5 b with a + b = 4 names the mix; the prior record must be that mix: integers and maxima
    exactly, float64 sums within one ulp per batch folded of the per-batch sums (the one place order is free)."""
    d, words, L, _ = NETS["hex5_1x32"]
    blob = seeded_blob(d, 31)
    rng = np.random.default_rng(5)
    work = {}
    for name, n in (("a", 3), ("b", 5)):
        idx = np.stack([rng.permutation(d.moves)[:L] for _ in range(n)]).astype(np.uint16)
        work[name] = (random_planes(d, words, n, 60 + n), idx, rng.integers(1, L + 1, size=n).astype(np.uint16))
    outs = {}
    for dt in ("bf16", "f32"):
        with HipEvaluator(blob, batch_size=8, plane_words=words, dtype=dt, switches={}) as ev:
            outs[dt] = {name: ev.eval_legal(*w) for name, w in work.items()}
    errors = []
    with HipEvaluator(blob, batch_size=8, plane_words=words, dtype="bf16", switches={}, verify_every=3) as ev:
        def run(name):
            try:
                for _ in range(6):
                    p, v = ev.eval_legal(*work[name])
                    assert p.tobytes() == outs["bf16"][name][0].tobytes() and v.tobytes() == outs["bf16"][name][1].tobytes()
            except BaseException as exc:  # noqa: BLE001 - reported by the main thread
                errors.append(exc)

        threads = [threading.Thread(target=run, args=(name,)) for name in work]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        ps, vs, st = ev.verify_prior_stats(), ev.verify_stats(), ev.stats()
    assert not errors, errors
    assert st["batches"] == 12 and vs["batches"] == 4 and ps["batches"] == 4 and ps["batches_without_legal"] == 0
    assert ps["leaves"] == vs["leaves"] and (vs["leaves"] - 12) % 2 == 0 and 12 <= vs["leaves"] <= 20
    nb = (vs["leaves"] - 12) // 2
    mix = {"a": 4 - nb, "b": nb}
    per = {}
    for name, w in work.items():
        rec = records_restated(outs["bf16"][name][0], outs["f32"][name][0], w[2], outs["bf16"][name][1], outs["f32"][name][1])
        per[name] = (fold_restated(rec), fold_values_restated(outs["bf16"][name][1], outs["f32"][name][1]))
    print("two lanes: mix", mix, ps)
    present = [name for name in mix if mix[name]]
    for k in ("leaves", "top1_flips", "nonfinite", "empty"):
        assert ps[k] == sum(mix[name] * per[name][0][k] for name in mix), k
    assert ps["value_leaves"] == sum(mix[name] * per[name][1][0] for name in mix)
    assert ps["tv_hist"] == [sum(mix[name] * per[name][0]["tv_hist"][i] for name in mix) for i in range(8)]
    for k in ("max_tv", "max_regret"):
        assert f32_bits(ps[k]) == f32_bits(max(per[name][0][k] for name in present)), k
    for k, want in (("sum_tv", sum(mix[name] * per[name][0]["sum_tv"] for name in mix)), ("sum_regret", sum(mix[name] * per[name][0]["sum_regret"] for name in mix)),
                    ("sum_dvalue", sum(mix[name] * per[name][1][1] for name in mix))):
        assert abs(ps[k] - want) <= 4 * np.spacing(max(abs(want), abs(ps[k]))), (k, ps[k], want)


# ---------------------------------------------------------------------------------------- 6. refusals and state


def test_refusals_and_state():
    d, words, L, _ = NETS["ttt1x32"]
    blob = seeded_blob(d, 31)
    with HipEvaluator(blob, batch_size=4, plane_words=words, dtype="f32", switches={}) as ev:
        for call in (ev.verify_prior_stats, ev.verify_worst_prior):
            with pytest.raises(CattusHipError) as err:
                call()
            assert err.value.status == CATTUS_E_UNSUPPORTED
    sd = simple_desc(3, 3, 9)
    with HipEvaluator(seeded_blob(sd, 2), batch_size=4, plane_words=1, dtype="bf16", switches={}) as ev:
        for call in (ev.verify_prior_stats, ev.verify_worst_prior):
            with pytest.raises(CattusHipError) as err:
                call()
            assert err.value.status == CATTUS_E_UNSUPPORTED
    with HipEvaluator(blob, batch_size=4, plane_words=words, dtype="bf16", switches={}) as ev:
        assert ev._lib.cattus_hip_verify_prior_stats(ev._h, C.byref(PriorStats(struct_size=0))) == CATTUS_E_INVALID
        ps = ev.verify_prior_stats()  # before verification was ever on: an empty record, not an error
        assert ps["leaves"] == 0 and ps["batches"] == 0 and ps["value_leaves"] == 0 and ps["tv_mean"] == 0.0
        with pytest.raises(CattusHipError) as err:
            ev.verify_worst_prior()
        assert err.value.status == CATTUS_E_STATE
        ev.verify(1)
        planes = random_planes(d, words, 2, 3)
        idx = np.tile(np.arange(L, dtype=np.uint16), (2, 1))
        ev.eval_legal(planes, idx, np.array([0, 0], dtype=np.uint16))  # compared, but no leaf entered the sums: still no worst leaf
        with pytest.raises(CattusHipError) as err:
            ev.verify_worst_prior()
        assert err.value.status == CATTUS_E_STATE and ev.verify_prior_stats()["empty"] == 2
        ev.eval_legal(planes, idx, np.array([L, 4], dtype=np.uint16))
        count = len(ev.verify_worst_prior()["legal_idx"])
        assert count in (L, 4)
        with pytest.raises(CattusHipError) as err:
            ev.verify_worst_prior(cap=count - 1)
        assert err.value.status == CATTUS_E_INVALID
        assert len(ev.verify_worst_prior(cap=count)["legal_idx"]) == count


# ---------------------------------------------------------------------------------------- 7. behind the one-launch Winograd tower


def test_a_batch_the_one_launch_tower_gives_up_on_is_folded_once():
    """chess 1 x 128 with max_batch 132: the plan is tower_wino4_kernel.  CATTUS_WINO_SPIN=1 as test_verify_gpu.py sets it: a hand-off wait
    may give up, and that batch is run again on the per-layer launches; either way the batch is folded once, from the run whose outputs
    the caller gets, which are the per-layer bits."""
    d = NetDesc(**CHESS, blocks=1, filters=128, vhc=8, phc=8)
    n, L = 132, 33
    blob = seeded_blob(d, 23)
    rng = np.random.default_rng(9)
    planes = random_planes(d, 1, n, 14)
    idx = np.stack([rng.permutation(d.moves)[:L] for _ in range(n)]).astype(np.uint16)
    cnt = rng.integers(1, L + 1, size=n).astype(np.uint16)
    with HipEvaluator(blob, batch_size=n, plane_words=1, dtype="f16x2", switches={"CATTUS_WINO_PERSIST": "0"}) as ev:
        own = ev.eval_legal(planes, idx, cnt)
    with HipEvaluator(blob, batch_size=n, plane_words=1, dtype="f32", switches={}) as ev:
        ref = ev.eval_legal(planes, idx, cnt)
    with HipEvaluator(blob, batch_size=n, plane_words=1, dtype="f16x2", switches={"CATTUS_WINO_SPIN": "1"}, verify_every=1) as ev:
        assert ev.tower_kernel() == "tower_wino4_kernel"
        got = ev.eval_legal(planes, idx, cnt)
        ps, worst, vs, st = ev.verify_prior_stats(), ev.verify_worst_prior(), ev.verify_stats(), ev.stats()
        print("give-up path: now on", ev.tower_kernel(), ps)
    assert got[0].tobytes() == own[0].tobytes() and got[1].tobytes() == own[1].tobytes()
    restated = Restated()
    restated.legal_batch(planes, idx, cnt, own, ref)
    restated.check(ps)
    assert ps["batches"] == 1 and ps["leaves"] == n and vs["batches"] == 1 and vs["leaves"] == n and st["batches"] == 1
    assert (worst["planes"] == restated.worst["planes"]).all() and worst["legal_idx"].tolist() == restated.worst["legal_idx"].tolist()
    assert (worst["top"], worst["top_ref"]) == (restated.worst["top"], restated.worst["top_ref"])


# ---------------------------------------------------------------------------------------- 8. the self-player


def test_self_player_reports_the_priors_it_searched_on(tmp_path):
    """model.inference.device_softmax in the engine JSON: with verify_every the summary gains five metrics (bin/tictactoe_self_player, as
    the trainer launches it); without the key exactly the old summary keys, and the record files of a run without verify_every."""
    d = NetDesc(**TTT, blocks=1, filters=32, vhc=4, phc=4)
    model = tmp_path / "model.cattus"
    model.write_bytes(seeded_blob(d, 9))
    summaries, files = {}, {}
    for tag, extra in (("plain", {}), ("verified", {"verify_every": 1}), ("priors", {"verify_every": 1, "device_softmax": True})):
        cfg = {
            "model": {"inference": {"engine": "hip", "device": 0, "dtype": "bf16", **extra}, "batch_size": 8},
            "mcts": {"sim_num": 10, "explore_factor": 1.41421, "temperature_policy": [[9999, 0.0]], "prior_noise_alpha": 0.0,
                     "prior_noise_epsilon": 0.0, "cache_size": 1000},
            "threads": 1,
            "concurrent_games": 1,
        }
        (tmp_path / f"{tag}.json").write_text(json.dumps(cfg))
        args = ["--model1-path", str(model), "--model2-path", str(model), "--games-num", "2", "--out-dir1", str(tmp_path / tag / "o1"),
                "--out-dir2", str(tmp_path / tag / "o2"), "--summary-file", str(tmp_path / f"{tag}_summary.json"), "--config-file", str(tmp_path / f"{tag}.json")]
        if tag == "priors":
            subprocess.check_call([str(sp._PKG.parent / "bin" / "tictactoe_self_player"), *args], cwd=str(tmp_path))
        else:
            sp.main(["--game", "tictactoe", *args])
        summaries[tag] = json.loads((tmp_path / f"{tag}_summary.json").read_text())
        files[tag] = {f"{o}/{f.name}": f.read_bytes() for o in ("o1", "o2") for f in sorted((tmp_path / tag / o).iterdir())}
    old_keys = {"model.activation_count", "model.run_duration", "mcts.search_duration", "cache.hits", "cache.misses", "node_evals", "evals_per_sec",
                "games_seconds", "model.saturated"}
    verify_keys = {"model.verified_leaves", "model.leaves_outside_bar", "model.max_dlogit", "model.max_dvalue"}
    new_keys = {"model.prior_leaves", "model.prior_top1_flips", "model.prior_tv_mean", "model.prior_tv_max", "model.value_abs_diff_mean"}
    assert set(summaries["plain"]["metrics"]) == old_keys
    assert set(summaries["verified"]["metrics"]) == old_keys | verify_keys
    m = summaries["priors"]["metrics"]
    assert set(m) == old_keys | verify_keys | new_keys
    print("self-player:", {k: m[k] for k in sorted(new_keys)})
    assert m["model.prior_leaves"] == m["model.verified_leaves"] > 0
    assert 0 <= m["model.prior_tv_mean"] <= m["model.prior_tv_max"] <= 1 and m["model.value_abs_diff_mean"] >= 0
    assert files["plain"] and files["plain"] == files["verified"]
