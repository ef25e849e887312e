#!/usr/bin/env python3
"""What a leaf costs through the leaf server, with the legal-move softmax on the host and on the device: builds
integration/c/consumer_legal.c and runs it on chess 20x256, dtype f16x2, 16 threads with one leaf per call each, at max_batch 16 and 64.

    mode A   cattus_hip_apply + the softmax on the calling thread (all 1880 logits cross to the host): the path before
             cattus_hip_apply_legal existed, unchanged by it -- the figure B is read against
    mode B   cattus_hip_apply_legal (the ragged softmax on the device; the leaf's probabilities cross)

The two modes alternate inside one process on one evaluator (A B A B ..., --rounds times each over the same --leaves leaves), so both see
the same box, clocks and neighbours; every max_batch is run --repeats times so that the run-to-run spread is on the page next to the
difference.  Legal lists: 20..40 seeded distinct moves per leaf.

    python scripts/server_legal_cost.py [--out profiles/server_legal_cost.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from cattus_amd import synth  # noqa: E402
from cattus_amd.weights import CHESS, NetDesc, seeded_blob  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--leaves", type=int, default=8192)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--blocks", type=int, default=20)
ap.add_argument("--filters", type=int, default=256)
ap.add_argument("--out")
args = ap.parse_args()

d = NetDesc(**CHESS, blocks=args.blocks, filters=args.filters, vhc=8, phc=8)
libdir = ROOT / "cattus_amd"
rows = []
with tempfile.TemporaryDirectory() as tmp:
    tmp = Path(tmp)
    exe = tmp / "consumer_legal"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-D_POSIX_C_SOURCE=200809L", f"-I{ROOT / 'include'}", str(ROOT / "integration" / "c" / "consumer_legal.c"),
                           "-o", str(exe), f"-L{libdir}", "-lcattus_hip", "-lpthread", "-lm", f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib"])
    (tmp / "model.cattus").write_bytes(seeded_blob(d, 1))
    synth.write_legal_leaves(tmp / "leaves.bin", synth.random_chess_planes(args.leaves, 1), synth.random_legal_lists(args.leaves, d.moves, 20, 40, 1))
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    for rep in range(args.repeats):
        for max_batch in (16, 64):
            run = subprocess.run([str(exe), str(tmp / "model.cattus"), str(tmp / "leaves.bin"), "2", str(max_batch), str(args.threads), "1", str(args.rounds)],
                                 capture_output=True, text=True, env=env, timeout=300)
            if run.returncode != 0:
                raise SystemExit("consumer_legal failed (%d): %s" % (run.returncode, run.stderr[-2000:]))
            rows.append(json.loads(run.stdout.strip().splitlines()[-1]))
            print(rows[-1], flush=True)

try:
    commit = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, cwd=ROOT).stdout.strip() or "unknown"
except OSError:
    commit = "unknown"
lines = ["command: python scripts/server_legal_cost.py " + " ".join(sys.argv[1:]), "on top of commit: " + commit,
         "chess %dx%d, f16x2, %d threads x one leaf per call, %d leaves x %d rounds per mode and process, modes alternating A B A B in one process, 20..40 legal moves"
         % (args.blocks, args.filters, args.threads, args.leaves, args.rounds),
         "A: cattus_hip_apply + host softmax    B: cattus_hip_apply_legal    (d2h: bytes copied device -> host per leaf, from the sizes the entry points copy)",
         "max_batch  mode  leaves/s   batch_fill  d2h_bytes/leaf   (processes in the order run)"]
for r in rows:
    for m in "AB":
        lines.append("%-10d %-5s %-10.1f %-11.2f %.1f" % (r["max_batch"], m, r[m]["leaves_per_s"], r[m]["batch_fill"], r[m]["d2h_bytes_per_leaf"]))
summary = {}
for r in rows:
    for m in "AB":
        summary.setdefault("%d%s" % (r["max_batch"], m), []).append(r[m]["leaves_per_s"])
lines.append("summary leaves/s: " + json.dumps({k: {"min": min(v), "max": max(v)} for k, v in summary.items()}))
lines.append("largest |A - B| of a probability: %.3g (libm's expf on the host, the evaluator's own exp on the device)" % max(r["max_prob_diff"] for r in rows))
print("\n".join(lines))
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
