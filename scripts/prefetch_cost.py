#!/usr/bin/env python3
"""What speculative leaf prefetch (cattus_sp_config.prefetch; include/cattus_selfplay.h) buys or costs where batches run half empty:
chess 20x256, dtype f16x2, the reference's self-play settings (temperature 1.0 for 30 moves, Dirichlet noise 0.03 / 0.25, so that games
differ), every game cut at --plies plies (max_game_plies), as many games as slots so that every run is one fixed-size round.

    shape a   64 games, 800 sims, batch_size 64 on a max_batch 64 evaluator: BASELINE.json config 4's per-GPU shape (per-layer direct kernels,
              whose cost grows with the rows of a batch)
    shape b   the same 64 games on a max_batch 256 evaluator (the one-launch Winograd tower, flat up to 128 rows), prefetch_fill 128
    shape c   a tail, 8 games: on a max_batch 32 evaluator (direct kernels, prefetch_fill 32) and on the max_batch 256 one (prefetch_fill 128)

Per shape the settings alternate inside one process on one evaluator -- off, then each --prefetch value, --repeats times over -- so that all
see the same box, clocks and neighbours and the run-to-run spread stands next to the difference.  The games are the same in every run of
a shape (prefetch does not change the search); what differs is how many network round trips they take.

    python scripts/prefetch_cost.py [--out profiles/prefetch.txt]
"""
import argparse
import os
import subprocess
import sys
import time
from pathlib import Path

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from cattus_amd import selfplay as sp  # noqa: E402
from cattus_amd.evaluator import HipEvaluator  # noqa: E402
from cattus_amd.weights import CHESS, NetDesc, seeded_blob  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sims", type=int, default=800)
ap.add_argument("--plies", type=int, default=6)
ap.add_argument("--prefetch", default="2,4,8", help="nominees per blocked search, comma separated; each is run against off")
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--threads", type=int, default=max(1, min(16, sp.available_cpus()) - 2))
ap.add_argument("--blocks", type=int, default=20)
ap.add_argument("--filters", type=int, default=256)
ap.add_argument("--shapes", default="a,b,c")
ap.add_argument("--tail-leaves", type=int, default=0, help="cattus_eval_config.tail_leaves of the evaluators (capped at their max_batch; ignored on the direct plan)")
ap.add_argument("--out")
args = ap.parse_args()

d = NetDesc(**CHESS, blocks=args.blocks, filters=args.filters, vhc=8, phc=8)
blob = seeded_blob(d, 2)
settings = [0] + [int(k) for k in args.prefetch.split(",")]
# name, games, evaluator max_batch = batch_size, prefetch_fill
SHAPES = {"a": [("a", 64, 64, 0)], "b": [("b", 64, 256, 128)], "c": [("c/32", 8, 32, 0), ("c/256", 8, 256, 128)]}
rows, records = [], {}
for key in args.shapes.split(","):
    for name, games, max_batch, fill in SHAPES[key]:
        with HipEvaluator(blob, batch_size=max_batch, plane_words=1, dtype="f16x2", tail_leaves=min(args.tail_leaves, max_batch)) as ev:
            kernel = ev.tower_kernel() + ("+tail%d" % ev.tail_leaves() if ev.tail_leaves() else "")
            for rep in range(args.repeats):
                for k in settings:
                    cfg = sp.make_config(sim_num=args.sims, batch_size=max_batch, max_game_plies=args.plies, threads=args.threads, concurrent_games=games,
                                         cache_size=1000000, temperature_policy=[(30, 1.0), (9999, 0.0)], prior_noise_alpha=0.03, prior_noise_epsilon=0.25,
                                         prefetch=k, prefetch_fill=fill if k else 0)
                    t = time.time()
                    res = sp.run_self_play("chess", cfg, sp.Net.hip(ev), None, games)
                    dt = time.time() - t
                    same = records.setdefault(name, res["record_bytes"]).tobytes() == res["record_bytes"].tobytes()
                    rows.append(dict(shape=name, kernel=kernel, prefetch=k, fill=fill if k else 0, evals_per_s=res["node_evals"] / dt, batches=res["activation_count"],
                                     real_fill=res["node_evals"] / max(1, res["activation_count"]),
                                     rows_fill=(res["node_evals"] + res["prefetch_evaluated"]) / max(1, res["activation_count"]), spec_rows=res["prefetch_evaluated"],
                                     hits=res["prefetch_hits"], hit_rate=res["prefetch_hits"] / max(1, res["prefetch_evaluated"]), plies_per_s=res["positions"] / dt,
                                     seconds=dt, same=same))
                    print(rows[-1], flush=True)
                    if not same:
                        raise SystemExit("the records of shape %s with prefetch %d are not those of its first run" % (name, k))

try:
    commit = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, cwd=ROOT).stdout.strip() or "unknown"
except OSError:
    commit = "unknown"
lines = ["command: python scripts/prefetch_cost.py " + " ".join(sys.argv[1:]), "on top of commit: " + commit,
         "chess %dx%d, f16x2, %d sims, games cut at %d plies, temperature 1.0 / noise 0.03 0.25, %d worker threads, 2 batches in flight, cache 1000000; "
         "settings alternate in one process per shape; the records of every run of a shape are byte-identical (checked)" % (args.blocks, args.filters, args.sims, args.plies, args.threads),
         "evals/s: real leaves per second (speculative rows are not in it); fill: real leaves per batch; rows: real + speculative per batch; hit rate: hits / speculative rows",
         "%-6s %-28s %-8s %-5s %-9s %-8s %-6s %-6s %-10s %-8s %-8s %-8s %s" % ("shape", "kernel", "prefetch", "fill", "evals/s", "batches", "fill", "rows", "spec_rows", "hits", "hit_rate", "plies/s", "seconds")]
for r in rows:
    lines.append("%-6s %-28s %-8d %-5d %-9.0f %-8d %-6.1f %-6.1f %-10d %-8d %-8.2f %-8.2f %.2f" % (r["shape"], r["kernel"], r["prefetch"], r["fill"], r["evals_per_s"], r["batches"],
                                                                                             r["real_fill"], r["rows_fill"], r["spec_rows"], r["hits"], r["hit_rate"], r["plies_per_s"], r["seconds"]))
best = {}
for r in rows:
    best.setdefault((r["shape"], r["prefetch"]), []).append(r["plies_per_s"])
lines.append("plies/s, min .. max over the repeats: " + "; ".join("%s prefetch %d: %.2f .. %.2f" % (s, k, min(v), max(v)) for (s, k), v in best.items()))
print("\n".join(lines))
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
