#!/usr/bin/env python
"""Where does an evaluator leave the exact network on a given leaf?  Prints HipEvaluator.trace as a table, one line per point.

    python scripts/trace_leaf.py model.cattus planes.npy [--dtype f16x2] [--leaf 0]

planes.npy: uint64 [n, C, plane_words] (or [C, plane_words]), e.g. numpy.save of HipEvaluator.verify_worst_planes().
"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from cattus_amd.evaluator import HipEvaluator  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("blob")
ap.add_argument("planes")
ap.add_argument("--dtype", default="f16x2", choices=["f16x2", "f16", "bf16"])
ap.add_argument("--leaf", type=int, default=0)
args = ap.parse_args()
blob = Path(args.blob).read_bytes()
planes = np.load(args.planes).astype(np.uint64)
planes = planes[None] if planes.ndim == 2 else planes
leaf = planes[args.leaf:args.leaf + 1]
with HipEvaluator(blob, batch_size=max(len(planes), 1), plane_words=planes.shape[2], dtype=args.dtype, switches={}) as ev:
    rec, _, value = ev.trace(leaf)
    d, hw = ev.desc, ev.desc.board ** 2
    print(f"{ev.tower_kernel()}, dtype {args.dtype}, leaf {args.leaf}: value {value[0]:.6f}, saturated {ev.stats()['saturated']}")
    print(f"{'point':>5} {'tensor':<16} {'rms_diff/rms_ref':>16} {'max_diff':>12} {'channel':>7} {'pixel':>5} {'x':>14} {'ref':>14} flags")
    for p, r in enumerate(rec[:, 0]):
        what = "stem" if p == 0 else "heads" if p == len(rec) - 1 else f"block {(p - 1) // 2} " + ("conv1" if p % 2 else "output")
        ratio = r["rms_diff"] / r["rms_ref"] if r["rms_ref"] else float("nan")
        print(f"{p:>5} {what:<16} {ratio:>16.3e} {r['max_diff']:>12.4e} {r['at'] // hw:>7} {r['at'] % hw:>5} {r['x']:>14.6e} {r['ref']:>14.6e} {r['flags']}")
