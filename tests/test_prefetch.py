"""Speculative leaf prefetch (cattus_sp_config.prefetch; include/cattus_selfplay.h) on the CPU, with the stand-in network.

A sequential search that stops for the network also names the leaves it is likely to ask for next (MctsPlayer::nominate: the
leaves that leaves_in_flight = k + 1 would have taken, found with virtual losses that are all rolled back); those ride in the
rows a batch has free, and their results go into the evaluation cache only.  The search is untouched, so what is held here is:
records and visit counts are exactly those of prefetch = 0; a nomination leaves the tree as it found it; the counters add up;
and what the feature rests on (the cache, the sequential search) is demanded, not assumed."""

import ctypes as C
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from cattus_amd import selfplay as sp

ROOT = Path(__file__).resolve().parent.parent
GAMES = {"tictactoe": dict(sim_num=30), "hex5": dict(sim_num=30), "chess": dict(sim_num=12, max_game_plies=10)}
N_GAMES = 4


def _cfg(game, **kw):
    base = dict(temperature_policy=[(9999, 0.0)], cache_size=100000, batch_size=1, threads=1, **GAMES[game])
    base.update(kw)
    return sp.make_config(**base)


def _same_records(a, b):
    return a["record_meta"].shape == b["record_meta"].shape and (a["record_meta"] == b["record_meta"]).all() and (a["record_bytes"] == b["record_bytes"]).all()


_OFF = {}


def _off(game):
    """The games without prefetch, played once per game and shared (one thread, batch_size 1: the reference's schedule)."""
    if game not in _OFF:
        _OFF[game] = sp.run_self_play(game, _cfg(game), sp.Net.stub(game), None, N_GAMES)
        assert _OFF[game]["positions"] > 0 and _OFF[game]["prefetch_nominated"] == 0
    return _OFF[game]


# ------------------------------------------------------------------------------------------ records


@pytest.mark.parametrize("game", sorted(GAMES))
@pytest.mark.parametrize("prefetch", [1, 4, 15])
def test_records_are_those_of_the_sequential_search(game, prefetch):
    """Byte-identical records off against on, at two thread counts, with batch_size 1 (no row is ever free) and with a
    batch_size above the number of games (every batch has free rows)."""
    off = _off(game)
    for threads, batch in ((1, 1), (3, 16), (3, 1), (1, 16)):
        on = sp.run_self_play(game, _cfg(game, prefetch=prefetch, threads=threads, batch_size=batch, concurrent_games=N_GAMES), sp.Net.stub(game), None, N_GAMES)
        assert _same_records(on, off), (threads, batch)
        assert [on[k] for k in ("player1_wins", "player2_wins", "draws", "positions")] == [off[k] for k in ("player1_wins", "player2_wins", "draws", "positions")]
        assert on["prefetch_nominated"] > 0 and on["prefetch_nominated"] == on["prefetch_evaluated"] + on["prefetch_dropped"]
        if batch == 1:
            assert on["prefetch_evaluated"] == 0 and on["node_evals"] == on["activation_count"]
        else:
            assert on["prefetch_hits"] > 0 and on["activation_count"] < off["activation_count"]


def test_noisy_games_with_prefetch_are_those_without():
    """Dirichlet noise and temperature on, seeded per game as in test_noisy_games_do_not_depend_on_schedule_or_sharding: a nomination
    draws nothing from the game's random stream, so the same games come out."""
    kw = dict(sim_num=20, temperature_policy=[(4, 1.0), (9999, 0.0)], prior_noise_alpha=0.3, prior_noise_epsilon=0.25, cache_size=10000)
    ref = sp.run_self_play("hex5", _cfg("hex5", **kw), sp.Net.stub("hex5"), None, 12)
    for extra in (dict(threads=4, batch_size=8, concurrent_games=5, prefetch=4), dict(threads=3, batch_size=16, concurrent_games=12, eval_threads=1, prefetch=15),
                  dict(threads=2, batch_size=8, concurrent_games=6, prefetch=2, prefetch_fill=5)):
        got = sp.run_self_play("hex5", _cfg("hex5", **kw, **extra), sp.Net.stub("hex5"), None, 12)
        assert _same_records(got, ref), extra
        assert got["prefetch_hits"] > 0
    firsts = {ref["record_bytes"][i].tobytes() for i in range(len(ref["record_bytes"])) if ref["record_meta"][i][1] == 1}
    assert len(firsts) > 1  # the noise is really on


def test_two_models_prefetch_for_their_own_network():
    """Each network of a two-model run has its own queue of nominees: both are asked for speculative rows, every row either network
    sees is a real leaf or an evaluated nominee, and the games are those without prefetch."""
    calls = {"a": 0, "b": 0}

    def mk(tag, bias):
        def net(planes):
            calls[tag] += len(planes)
            h = (planes.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).sum(axis=1)
            pol = ((h[:, None] >> (np.arange(9, dtype=np.uint64)[None, :] * np.uint64(5))) & np.uint64(15)).astype(np.float32) * np.float32(bias)
            return pol, np.zeros(len(planes), dtype=np.float32)

        return net

    kw = dict(sim_num=20, batch_size=8, threads=2, concurrent_games=4)
    off = sp.run_self_play("tictactoe", _cfg("tictactoe", **kw), sp.Net.python(mk("a", 0.2)), sp.Net.python(mk("b", -0.2)), 4)
    real = dict(calls)
    assert off["node_evals"] == real["a"] + real["b"]
    calls.update(a=0, b=0)
    on = sp.run_self_play("tictactoe", _cfg("tictactoe", prefetch=4, **kw), sp.Net.python(mk("a", 0.2)), sp.Net.python(mk("b", -0.2)), 4)
    assert _same_records(on, off)
    assert calls["a"] + calls["b"] == on["node_evals"] + on["prefetch_evaluated"]
    assert on["prefetch_evaluated"] > 0 and on["prefetch_hits"] > 0 and calls["a"] > 0 and calls["b"] > 0


def test_legal_move_network_sees_the_nominees_legal_moves():
    """With a network that does calc_moves_probs itself (the host side of cattus_hip_eval_legal) a speculative row carries its own
    legal-move list, and its result reaches the cache through finish_legal: same records as the plain network without prefetch."""
    moves = 1880

    def logits(planes):
        h = (planes.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).sum(axis=1)
        k = np.arange(moves, dtype=np.uint64)[None, :]
        x = (h[:, None] ^ (k * np.uint64(0xC2B2AE3D27D4EB4F))) * np.uint64(0xD6E8FEB86659FD93)
        pol = ((x >> np.uint64(40)).astype(np.float32) / np.float32(1 << 24) - 0.5) * 6.0
        return pol.astype(np.float32), ((h >> np.uint64(40)).astype(np.float32) / np.float32(1 << 24) - 0.5).astype(np.float32) * np.float32(0.6)

    def legal(planes, idx, cnt):
        pol, val = logits(planes)
        probs = np.zeros(idx.shape, dtype=np.float32)
        for i in range(len(planes)):
            c = int(cnt[i])
            assert 0 < c <= idx.shape[1] and len(set(idx[i, :c].tolist())) == c
            x = pol[i, idx[i, :c].astype(np.int64)]
            e = np.exp(x - x.max(), dtype=np.float32)
            probs[i, :c] = e / e.sum(dtype=np.float32)
        return probs, val

    kw = dict(sim_num=12, max_game_plies=6, batch_size=8, threads=2, concurrent_games=2)
    off = sp.run_self_play("chess", _cfg("chess", **kw), sp.Net.python_legal(legal), None, 2)
    on = sp.run_self_play("chess", _cfg("chess", prefetch=4, **kw), sp.Net.python_legal(legal), None, 2)
    assert _same_records(on, off)
    assert on["prefetch_evaluated"] > 0 and on["prefetch_hits"] > 0 and on["activation_count"] < off["activation_count"]


# ------------------------------------------------------------------------------------------ visit counts


@pytest.mark.parametrize("game,plies", [("tictactoe", 9), ("hex5", 6), ("chess", 4)])
def test_visit_counts_of_a_traced_game_do_not_notice(game, plies):
    """cattus_sp_trace_game honours the field: every stop nominates, rolls back and evaluates the nominees into the cache, and the
    root visit counts of every ply are those of the trace without prefetch."""
    sims = 60 if game != "chess" else 24
    off = sp.trace_game(game, sp.make_config(sim_num=sims, cache_size=100000), sp.Net.stub(game), max_plies=plies)
    seen = {"rows": 0}

    def counting(planes):
        seen["rows"] += len(planes)
        info = sp.game_info(game)
        ctx = (C.c_uint32 * 2)(info["moves"], info["planes"] * info["plane_words"])
        pol, val = np.zeros((len(planes), info["moves"]), dtype=np.float32), np.zeros(len(planes), dtype=np.float32)
        sp.load_library().cattus_sp_stub_net(ctx, planes.ctypes.data_as(C.POINTER(C.c_uint64)), len(planes), pol.ctypes.data_as(C.POINTER(C.c_float)), val.ctypes.data_as(C.POINTER(C.c_float)))
        return pol, val

    plain = sp.trace_game(game, sp.make_config(sim_num=sims, cache_size=100000), sp.Net.python(counting), max_plies=plies)
    rows_off = seen["rows"]
    assert plain == off
    for k in (1, 4, 15):
        seen["rows"] = 0
        on = sp.trace_game(game, sp.make_config(sim_num=sims, cache_size=100000, prefetch=k), sp.Net.python(counting), max_plies=plies)
        assert on == off, k
        assert seen["rows"] >= rows_off  # a nominee's row saves at most the one row of the leaf it named
    assert seen["rows"] > rows_off  # fifteen nominees per stop do not all get asked for: the hook did run the feature


# ------------------------------------------------------------------------------------------ rollback


TTT_POSITIONS = [None, "____x____o", "x___o____x", "xo__x____o", "x_o_o_x__x", "xox_o____x"]


def _behind_the_first(leaves):
    """The leaves a tree with several in flight took behind its first, each position once."""
    want = []
    for s in leaves[1:]:
        if s not in want and s != leaves[0]:
            want.append(s)
    return want


@pytest.mark.parametrize("k", [1, 3, 8, 15])
def test_nomination_rolls_everything_back_and_names_what_leaves_in_flight_would_take(k):
    """After a nomination no edge holds a virtual loss, exactly one node is pending (the search's own leaf), and simulation count,
    root visit counts, the random stream and the pending position are what they were; the pending leaf then takes its
    evaluation as ever.  No nominee is finished, the pending position, or named twice.  And on hand-built positions, at every
    point of the search where the copy with leaves_in_flight = k + 1 finished no terminal simulation on the way (it backs those
    up, which a nomination must not), the nominees are exactly the leaves the copy took behind the first -- a position the copy
    holds twice, by transposition, named once."""
    compared = most = 0
    for pos in TTT_POSITIONS:
        for sims in (1, 2, 3, 5, 8, 13, 21, 34):
            r = sp.nominate_kat("tictactoe", pos, sims, k)
            assert r["vl_held"] == 0 and r["pending_nodes"] == 1 and r["state_unchanged"] and r["nominees_clean"], (pos, sims, r)
            assert len(r["nominees"]) <= k and len(r["lif_leaves"]) <= k + 1
            if r["lif_finished"] == 0:
                assert r["nominees"] == _behind_the_first(r["lif_leaves"]), (pos, sims, r)
                compared += 1
                most = max(most, len(r["nominees"]))
    assert compared >= 10 and most >= min(k, 3), (compared, most)  # the comparison was made, and on more than one nominee
    for game, sims in (("hex5", 30), ("chess", 20)):
        r = sp.nominate_kat(game, None, sims, k)
        assert r["vl_held"] == 0 and r["pending_nodes"] == 1 and r["state_unchanged"] and r["nominees_clean"]
        assert r["lif_finished"] == 0 and r["nominees"] == _behind_the_first(r["lif_leaves"]) and len(r["nominees"]) >= 1


# ------------------------------------------------------------------------------------------ counters


@pytest.mark.parametrize("game", ["hex5", "chess"])
def test_counters_with_one_game_at_a_time_add_up_exactly(game):
    """One slot, so nothing races: a nominee's row returns with the leaf its search waits for and is in the cache before the search
    goes on.  Then every hit is one leaf that did not go to the network: node_evals is the count without prefetch minus the hits.
    The leaves the searches asked for (cache hits + misses) are the same in both runs."""
    kw = dict(concurrent_games=1, threads=1, batch_size=16, eval_threads=1)
    off = sp.run_self_play(game, _cfg(game, **kw), sp.Net.stub(game), None, 2)
    on = sp.run_self_play(game, _cfg(game, prefetch=4, **kw), sp.Net.stub(game), None, 2)
    assert _same_records(on, off)
    assert on["prefetch_hits"] > 0 and on["prefetch_evaluated"] <= on["prefetch_nominated"]
    assert on["prefetch_nominated"] == on["prefetch_evaluated"] + on["prefetch_dropped"]
    assert on["node_evals"] == off["node_evals"] - on["prefetch_hits"]
    assert on["cache_hits"] + on["cache_misses"] == off["cache_hits"] + off["cache_misses"]
    assert on["cache_misses"] == on["node_evals"]  # a speculative row is nobody's miss
    assert on["activation_count"] == on["node_evals"] < off["activation_count"]  # one real leaf per batch, and fewer batches


def test_counters_with_many_games_and_threads():
    off = sp.run_self_play("hex5", _cfg("hex5", threads=3, batch_size=16, concurrent_games=8), sp.Net.stub("hex5"), None, 8)
    on = sp.run_self_play("hex5", _cfg("hex5", threads=3, batch_size=16, concurrent_games=8, prefetch=4), sp.Net.stub("hex5"), None, 8)
    assert _same_records(on, off)
    assert on["prefetch_hits"] > 0 and on["prefetch_evaluated"] <= on["prefetch_nominated"]
    assert on["prefetch_nominated"] == on["prefetch_evaluated"] + on["prefetch_dropped"]
    assert on["cache_hits"] + on["cache_misses"] == off["cache_hits"] + off["cache_misses"]
    assert on["activation_count"] < off["activation_count"]
    assert on["steady_node_evals"] <= on["node_evals"] <= on["cache_hits"] + on["cache_misses"]  # speculative rows are in neither


def test_a_batch_with_prefetch_fill_real_leaves_carries_no_nominee():
    """prefetch_fill 1: every batch has at least one real leaf, so none is topped up -- nominees are named and all dropped, and the
    run costs what it costs without prefetch."""
    off = sp.run_self_play("hex5", _cfg("hex5", concurrent_games=1, batch_size=4, eval_threads=1), sp.Net.stub("hex5"), None, 2)
    on = sp.run_self_play("hex5", _cfg("hex5", concurrent_games=1, batch_size=4, eval_threads=1, prefetch=4, prefetch_fill=1), sp.Net.stub("hex5"), None, 2)
    assert _same_records(on, off)
    assert on["prefetch_nominated"] > 0 and on["prefetch_evaluated"] == 0 and on["prefetch_hits"] == 0
    assert on["prefetch_dropped"] == on["prefetch_nominated"]
    assert on["node_evals"] == off["node_evals"] and on["activation_count"] == off["activation_count"]
    # and with 4 games in 4 slots a fill of 2 is reached by some batches and not by others
    some = sp.run_self_play("hex5", _cfg("hex5", concurrent_games=4, batch_size=8, threads=2, prefetch=4, prefetch_fill=2), sp.Net.stub("hex5"), None, 4)
    assert _same_records(some, _off("hex5"))


# ------------------------------------------------------------------------------------------ configuration


def test_what_prefetch_rests_on_is_demanded_not_clamped():
    net = sp.Net.stub("tictactoe")
    with pytest.raises(RuntimeError, match="cache_size"):
        sp.run_self_play("tictactoe", _cfg("tictactoe", prefetch=4, cache_size=0), net, None, 2)
    with pytest.raises(RuntimeError, match="leaves_in_flight"):
        sp.run_self_play("tictactoe", _cfg("tictactoe", prefetch=4, leaves_in_flight=2), net, None, 2)
    with pytest.raises(RuntimeError, match="0..15"):
        sp.run_self_play("tictactoe", _cfg("tictactoe", prefetch=16), net, None, 2)
    with pytest.raises(RuntimeError, match="prefetch_fill"):
        sp.run_self_play("tictactoe", _cfg("tictactoe", prefetch=4, batch_size=4, prefetch_fill=5), net, None, 2)
    with pytest.raises(RuntimeError, match="cache_size"):
        sp.trace_game("tictactoe", sp.make_config(sim_num=10, cache_size=0, prefetch=1), net)
    # none of it matters with prefetch off
    sp.run_self_play("tictactoe", _cfg("tictactoe", cache_size=0, leaves_in_flight=2, prefetch_fill=99), net, None, 2)
    sp.run_self_play("tictactoe", _cfg("tictactoe", prefetch=15, leaves_in_flight=0, batch_size=4, prefetch_fill=4), net, None, 2)


def test_a_config_of_the_old_length_is_accepted_and_means_off():
    """struct_size versions the configuration: the length before the two fields were appended is still taken, and whatever lies
    behind it is not read."""
    assert sp.SP_CONFIG_SIZE_V1 == C.sizeof(sp.SpConfig) - 8
    cfg = _cfg("hex5", prefetch=4, prefetch_fill=77, batch_size=8, concurrent_games=4)
    cfg.struct_size = sp.SP_CONFIG_SIZE_V1
    old = sp.run_self_play("hex5", cfg, sp.Net.stub("hex5"), None, N_GAMES)
    assert _same_records(old, _off("hex5"))
    assert [old[k] for k in ("prefetch_nominated", "prefetch_evaluated", "prefetch_hits", "prefetch_dropped")] == [0, 0, 0, 0]
    assert sp.trace_game("hex5", cfg, sp.Net.stub("hex5"), max_plies=2) == sp.trace_game("hex5", _cfg("hex5"), sp.Net.stub("hex5"), max_plies=2)
    cfg.struct_size = sp.SP_CONFIG_SIZE_V1 + 4
    with pytest.raises(RuntimeError, match="bad config struct"):
        sp.run_self_play("hex5", cfg, sp.Net.stub("hex5"), None, N_GAMES)


def test_engine_json_and_summary(tmp_path):
    engine = {
        "model": {"batch_size": 8},
        "mcts": {"sim_num": 12, "explore_factor": 1.41421, "temperature_policy": [[9999, 0.0]], "prior_noise_alpha": 0.0, "prior_noise_epsilon": 0.0, "cache_size": 1000},
        "threads": 2,
    }
    plain = sp.config_from_engine_json(engine)
    assert (plain.prefetch, plain.prefetch_fill) == (0, 0)
    cfg = sp.config_from_engine_json({**engine, "prefetch": 4, "prefetch_fill": 6, "concurrent_games": 4}, concurrent_games=4)
    assert (cfg.prefetch, cfg.prefetch_fill) == (4, 6)
    res = sp.run_self_play("tictactoe", cfg, sp.Net.stub("tictactoe"), None, 4)
    sp.write_summary(tmp_path / "on.json", res)
    m = json.loads((tmp_path / "on.json").read_text())["metrics"]
    assert m["mcts.prefetch_evaluated"] == res["prefetch_evaluated"] > 0 and m["mcts.prefetch_hits"] == res["prefetch_hits"] > 0
    sp.write_summary(tmp_path / "off.json", sp.run_self_play("tictactoe", plain, sp.Net.stub("tictactoe"), None, 4))
    assert not [k for k in json.loads((tmp_path / "off.json").read_text())["metrics"] if "prefetch" in k]  # off: exactly the old summary


# ------------------------------------------------------------------------------------------ sanitizers


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_the_runner_with_prefetch_under_sanitizers(sanitizer, tmp_path):
    """tests/prefetch_check.cpp, a program of its own around the driver (worker threads, evaluation threads, both queues, the
    sharded cache with marked entries), built with the sanitizer and run as a program: records equal off against on in every
    case, and no report."""
    exe = tmp_path / "prefetch_check"
    # -O0 -g1: the instrumented build of the whole host library takes a third of the time of -O1 -g, and a report still has its lines
    subprocess.check_call(["g++", "-O0", "-g1", "-std=c++17", f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all", "-pthread", "-o", str(exe),
                           str(ROOT / "tests" / "prefetch_check.cpp"), str(ROOT / "cattus_amd" / "csrc" / "host" / "cabi.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert p.stdout.rstrip().endswith("prefetch ok") and "DIFFER" not in p.stdout
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
