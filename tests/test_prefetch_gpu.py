"""Speculative leaf prefetch (cattus_sp_config.prefetch) on the real kernels: a speculative row is evaluated by the same launch
as the real leaves beside it, a leaf's output bits do not depend on the batch it came in, and so the search that finds a nominee's
result in the cache plays the game it would have played.  Chess 2 x 128 in f16x2, 8 games of 6 plies at 48 simulations: records
byte-identical off against on, real leaves served from speculative rows, and strictly fewer batches -- on the per-layer direct
kernels, behind the one-launch Winograd tower, and through the device softmax (cattus_hip_eval_legal).  tests/test_prefetch.py
holds the search's side on the CPU."""

import pytest

from cattus_amd import selfplay as sp
from cattus_amd.evaluator import HipEvaluator
from cattus_amd.weights import CHESS, NetDesc, seeded_blob

pytestmark = pytest.mark.gpu

WINOGRAD_KERNELS = ("conv3x3_wino_kernel", "conv3x3_wino4_kernel", "tower_wino4_kernel", "conv3x3_wino8_kernel")
GAMES, PREFETCH = 8, 4


@pytest.fixture(scope="module")
def blob():
    return seeded_blob(NetDesc(**CHESS, blocks=2, filters=128, vhc=8, phc=8), 17)


def _off_and_on(ev, batch_size, device_softmax=False):
    runs = []
    for prefetch in (0, PREFETCH):
        cfg = sp.make_config(sim_num=48, batch_size=batch_size, threads=4, concurrent_games=GAMES, cache_size=4096, max_game_plies=6, prefetch=prefetch)
        runs.append(sp.run_self_play("chess", cfg, sp.Net.hip(ev, device_softmax), None, GAMES))
    off, on = runs
    print("prefetch off: %d leaves in %d batches; on: %d leaves + %d speculative rows in %d batches, %d nominated, %d hits (%.0f%% of the rows), %d dropped"
          % (off["node_evals"], off["activation_count"], on["node_evals"], on["prefetch_evaluated"], on["activation_count"], on["prefetch_nominated"],
             on["prefetch_hits"], 100.0 * on["prefetch_hits"] / max(on["prefetch_evaluated"], 1), on["prefetch_dropped"]))
    assert off["positions"] == GAMES * 6
    assert off["prefetch_nominated"] == off["prefetch_evaluated"] == off["prefetch_hits"] == 0
    assert (on["record_meta"] == off["record_meta"]).all()
    assert (on["record_bytes"] == off["record_bytes"]).all()
    assert on["prefetch_hits"] > 0
    assert on["activation_count"] < off["activation_count"]
    assert on["prefetch_evaluated"] <= on["prefetch_nominated"] == on["prefetch_evaluated"] + on["prefetch_dropped"]
    # the leaves the searches asked for are the same in both runs (how many of them went to the network depends on timing in
    # both: games in step ask for the same position at once)
    assert on["cache_hits"] + on["cache_misses"] == off["cache_hits"] + off["cache_misses"]
    return off, on


def test_records_on_the_direct_kernels(blob):
    with HipEvaluator(blob, batch_size=32, plane_words=1, dtype="f16x2") as ev:
        print("tower kernel at max_batch 32:", ev.tower_kernel())
        assert ev.tower_kernel() not in WINOGRAD_KERNELS
        _off_and_on(ev, 32)
        st = ev.stats()
    assert st["saturated"] == 0


def test_records_behind_the_one_launch_winograd_tower(blob):
    with HipEvaluator(blob, batch_size=132, plane_words=1, dtype="f16x2") as ev:
        assert ev.tower_kernel() == "tower_wino4_kernel"  # what AUTO chooses at this size
        off, on = _off_and_on(ev, 132)
        print("tower kernel after the runs:", ev.tower_kernel())
    # 8 games give at most 8 real leaves a batch; the rows behind them are what the nominees ride in
    assert off["node_evals"] / off["activation_count"] <= GAMES
    assert (on["node_evals"] + on["prefetch_evaluated"]) / on["activation_count"] > off["node_evals"] / off["activation_count"]


@pytest.mark.parametrize("max_batch", [32, 132])
def test_records_through_the_device_softmax(blob, max_batch):
    """cattus_hip_eval_legal: a speculative row brings its own legal-move list, and its priors reach the cache through finish_legal."""
    with HipEvaluator(blob, batch_size=max_batch, plane_words=1, dtype="f16x2") as ev:
        if max_batch == 132:
            assert ev.tower_kernel() == "tower_wino4_kernel"
        _off_and_on(ev, max_batch, device_softmax=True)
