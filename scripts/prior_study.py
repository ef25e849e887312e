#!/usr/bin/env python
"""What does a throughput dtype cost per leaf, in the quantities a search consumes?  Runs every position of a file through a bf16, an f16
and an f16x2 evaluator of one blob with verify_every=1 and prints HipEvaluator.verify_prior_stats(), one line per dtype: how often the
favourite move differs from the exact network's, the total-variation distance of the legal-move priors, the prior mass the exact
favourite loses, the mean |dvalue|.  The per-leaf counterpart of scripts/agreement_study.py, on positions of your own.

    python scripts/prior_study.py model.cattus positions.npz [--batch 256] [--out FILE]
    python scripts/prior_study.py --collect chess --workload chess20x256 positions.npz
                                    writes such a file: the leaves (planes and legal lists) that a few self-play games on the f32
                                    evaluator of bench.py's seeded network hand to the network

positions.npz: planes uint64 [n, C, plane_words], legal_idx uint16 [n, L], legal_count uint16 [n].
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from cattus_amd.evaluator import HipEvaluator  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("blob", nargs="?")
ap.add_argument("positions")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--out")
ap.add_argument("--collect", metavar="GAME", help="write the positions file instead: self-play of GAME on the f32 evaluator")
ap.add_argument("--workload", default="chess20x256", help="--collect: a network of bench.py's make_workload")
ap.add_argument("--games", type=int, default=4)
ap.add_argument("--sims", type=int, default=100)
ap.add_argument("--plies", type=int, default=40)
args = ap.parse_args()

if args.collect:
    import bench
    from cattus_amd import selfplay as sp

    d, blob, _ = bench.make_workload(args.workload)
    info = sp.game_info(args.collect)
    seen = []
    with HipEvaluator(blob, batch_size=64, plane_words=info["plane_words"], dtype="f32", switches={}) as ev:
        def net(planes, idx, cnt):
            planes = planes.reshape(len(planes), info["planes"], info["plane_words"])
            seen.append((planes, idx, cnt))
            return ev.eval_legal(planes, idx, cnt)

        cfg = sp.make_config(sim_num=args.sims, batch_size=64, threads=4, concurrent_games=args.games, max_game_plies=args.plies, cache_size=100000)
        sp.run_self_play(args.collect, cfg, sp.Net.python_legal(net), None, args.games, keep_records=False)
    planes, idx, cnt = (np.concatenate([s[i] for s in seen]) for i in range(3))
    _, first = np.unique(planes.reshape(len(planes), -1), axis=0, return_index=True)  # every position once, in the order met
    first.sort()
    np.savez_compressed(args.positions, planes=planes[first], legal_idx=idx[first], legal_count=cnt[first])
    print(f"{len(first)} distinct leaves of {len(planes)} ({args.collect}, {args.games} games, {args.sims} sims, {args.plies} plies) -> {args.positions}")
    sys.exit(0)

if not args.blob:
    ap.error("a blob is needed")
blob = Path(args.blob).read_bytes()
pos = np.load(args.positions)
planes, idx, cnt = pos["planes"].astype(np.uint64), pos["legal_idx"].astype(np.uint16), pos["legal_count"].astype(np.uint16)
lines = [f"command: python scripts/prior_study.py {' '.join(sys.argv[1:])}",
         f"{len(planes)} leaves, legal moves per leaf {int(cnt.min())}..{int(cnt.max())} (mean {cnt.mean():.1f}), batches of {args.batch}, verify_every=1"]
for dtype in ("bf16", "f16", "f16x2"):
    with HipEvaluator(blob, batch_size=args.batch, plane_words=planes.shape[2], dtype=dtype, switches={}, verify_every=1) as ev:
        for at in range(0, len(planes), args.batch):
            ev.eval_legal(planes[at:at + args.batch], idx[at:at + args.batch], cnt[at:at + args.batch])
        ps, vs, kernel = ev.verify_prior_stats(), ev.verify_stats(), ev.tower_kernel()
    keep = ("leaves", "top1_flips", "tv_mean", "max_tv", "regret_mean", "max_regret", "dvalue_mean", "tv_hist", "nonfinite", "empty")
    lines.append(f"{dtype:<6} {kernel}: " + json.dumps({k: ps[k] for k in keep} | {"leaves_outside_bar": vs["leaves_outside"], "max_dlogit": vs["max_dlogit"]}))
print("\n".join(lines))
if args.out:
    Path(args.out).write_text("\n".join(lines) + "\n")
