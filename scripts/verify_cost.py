#!/usr/bin/env python3
"""What cattus_hip_verify costs: ms per blocking cattus_hip_eval call (page-locked buffers, 200 calls a figure, one process) of the f16x2
evaluator on chess 20x256 at batch 256 with verification off, every 64th, 8th and every batch; off / 64 alternate three times so that
the comparison sees the run-to-run spread.  The first `off` figures are taken before the shadow exists.

    python scripts/verify_cost.py                 this tree
    python scripts/verify_cost.py --lib PATH      the same `off` loop on another build of the library (a commit without the entry
                                                  points, say), through nothing but the calls that build has
    python scripts/verify_cost.py --mode eval_legal   the same table through cattus_hip_eval_legal (a seeded legal list of 20..40 moves per
                                                  leaf, stride 64): verified batches then also compare the priors (cattus_hip_verify_prior_stats)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
sys.path.insert(0, ".")
import numpy as np  # noqa: E402

import bench  # noqa: E402
from cattus_amd.evaluator import EvalConfig, LIB_PATH  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=str(LIB_PATH))
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--mode", choices=["eval", "eval_legal"], default="eval")
ap.add_argument("--off-only", action="store_true", help="the `off` figures alone (four of them)")
ap.add_argument("--out")
ap.add_argument("--commit", help="what to write as the commit (default: git rev-parse HEAD)")
args = ap.parse_args()

d, blob, planes = bench.make_workload("chess20x256")
n = len(planes)
L = C.CDLL(args.lib)
vp = C.c_void_p
L.cattus_hip_create.argtypes = [vp, C.c_size_t, C.POINTER(EvalConfig), C.POINTER(vp)]
L.cattus_hip_eval.argtypes = [vp, vp, C.c_uint32, vp, vp]
L.cattus_hip_host_alloc.argtypes = [C.c_size_t]
L.cattus_hip_host_alloc.restype = vp
L.cattus_hip_destroy.argtypes = [vp]
L.cattus_hip_destroy.restype = None
L.cattus_hip_last_error.restype = C.c_char_p
can_verify = hasattr(L, "cattus_hip_verify")
if can_verify:
    L.cattus_hip_verify.argtypes = [vp, vp, C.c_size_t, C.c_uint32]


def check(rc):
    if rc:
        raise SystemExit("status %d: %s" % (rc, L.cattus_hip_last_error().decode()))


cfg = EvalConfig(C.sizeof(EvalConfig), 0, n, planes.shape[2], 2, 200, 0)  # dtype f16x2, tower_form auto
h = vp()
check(L.cattus_hip_create(blob, len(blob), C.byref(cfg), C.byref(h)))
h_planes, h_policy, h_value = (L.cattus_hip_host_alloc(b) for b in (planes.nbytes, n * d.moves * 4, n * 4))
C.memmove(h_planes, planes.ctypes.data, planes.nbytes)


if args.mode == "eval_legal":
    L.cattus_hip_eval_legal.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp]
    rng = np.random.default_rng(1)
    legal_idx = np.stack([rng.permutation(d.moves)[:64] for _ in range(n)]).astype(np.uint16)
    legal_cnt = rng.integers(20, 41, size=n).astype(np.uint16)
    h_probs = L.cattus_hip_host_alloc(n * 64 * 4)
    one_call = lambda: L.cattus_hip_eval_legal(h, h_planes, n, legal_idx.ctypes.data, legal_cnt.ctypes.data, 64, h_probs, h_value)
else:
    one_call = lambda: L.cattus_hip_eval(h, h_planes, n, h_policy, h_value)


def ms_per_call(calls):
    for _ in range(20):
        check(one_call())
    t0 = time.perf_counter()
    for _ in range(calls):
        check(one_call())
    return (time.perf_counter() - t0) / calls * 1e3


rows = [("off", round(ms_per_call(args.calls), 4)) for _ in range(4 if args.off_only else 2)]  # before any shadow exists
if can_verify and not args.off_only:
    for every in (64, 0, 64, 0, 64, 0, 8, 1, 0):
        check(L.cattus_hip_verify(h, blob, len(blob), every))
        rows.append((str(every) if every else "off", round(ms_per_call(args.calls), 4)))
commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
lines = ["command: python scripts/verify_cost.py " + " ".join(sys.argv[1:]), "library: " + args.lib, "commit: " + commit,
         "chess 20x256, f16x2, batch %d, %d blocking cattus_hip_%s calls per figure from page-locked buffers, 20 warm-up calls each" % (n, args.calls, args.mode),
         "every  ms_per_batch   (in the order measured)"]
lines += ["%-6s %.4f" % r for r in rows]
by = {}
for k, v in rows:
    by.setdefault(k, []).append(v)
lines.append("summary: " + json.dumps({k: {"min": min(v), "max": max(v)} for k, v in by.items()}))
print("\n".join(lines))
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
L.cattus_hip_destroy(h)
