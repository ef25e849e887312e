#!/usr/bin/env python3
"""Batches of a few leaves on the direct form and on the split-K direct form (tower_form direct | direct_splitk): whole step and launch.

f16x2 evaluators of one network in one process, max_batch = n, alternating window by window:
  (d)  direct          conv3x3_splitw_kernel, the default at these sizes -- the yardstick
  (s)  direct_splitk   conv3x3_splitk_kernel at the rule's way count W (8 from 256 filters on, 4 below)
  (sW) direct_splitk under CATTUS_SPLITK_WAYS = 1, 2, 4, 8 wherever that is another count than the rule's (other bits: A/B only)
step_ms: cattus_hip_eval_device with planes, logits and values resident in HBM, HIP events around windows of STEPS steps; median over the
REPEATS windows and their spread (max - min) / median.  launch_us: cattus_hip_time_tower, the mean over the stem and the tower's layers.
served: leaves per second of THREADS host threads that each block in cattus_hip_apply with one leaf per call (the reference's threading
model through the leaf server; Python threads around the C call, so orientation, not a host-side figure), max_batch = THREADS.

    python scripts/splitk_time.py [blocks filters] [n ...]  > profiles/splitk_latency.txt   (both networks when none is named)"""
import ctypes
import os
import statistics
import sys
import threading
import time

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cattus_amd import synth  # noqa: E402
from cattus_amd.evaluator import HipEvaluator  # noqa: E402
from cattus_amd.weights import CHESS, NetDesc, seeded_blob  # noqa: E402

STEPS, WARMUP, REPEATS = 200, 100, 5
THREADS, SERVE_SECONDS, SERVE_ROUNDS = 16, 1.0, 2
args = [int(a) for a in sys.argv[1:]]
nets = [(args[0], args[1])] if len(args) >= 2 else [(20, 256), (4, 128)]
batches = args[2:] or [1, 4, 8, 16, 32, 64, 128]
if not torch.cuda.is_available():
    raise SystemExit("splitk_time.py measures on the GPU and there is none")
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
planes = synth.random_chess_planes(128, 2)
d_planes = torch.from_numpy(planes.view("int64")).to(dev)


def window(ev, n, pol, val, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(steps):
        ev.eval_device(d_planes.data_ptr(), n, pol.data_ptr(), val.data_ptr(), stream.cuda_stream)
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / steps


def served(ev, d):
    """Leaves per second of THREADS threads blocking in cattus_hip_apply, one leaf per call, for SERVE_SECONDS."""
    lib, h = ev._lib, ev._h
    lib.cattus_hip_apply.restype = ctypes.c_int
    stop = threading.Event()
    counts = [0] * THREADS

    def worker(i):
        leaf = np.ascontiguousarray(planes[i % len(planes)])
        policy, value = np.empty((d.moves,), dtype=np.float32), np.empty((1,), dtype=np.float32)
        lp, pp, vp = leaf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), policy.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), value.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        while not stop.is_set():
            if lib.cattus_hip_apply(h, lp, 1, pp, vp) != 0:
                raise RuntimeError("cattus_hip_apply failed")
            counts[i] += 1

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(THREADS)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    time.sleep(SERVE_SECONDS)
    stop.set()
    for t in ts:
        t.join()
    return sum(counts) / (time.perf_counter() - t0)


print(f"# {STEPS} steps per window, {REPEATS} windows per evaluator, alternating; step_ms = median (spread = (max - min) / median); launch_us = cattus_hip_time_tower, 50 passes")
for blocks, filters in nets:
    d = NetDesc(**CHESS, blocks=blocks, filters=filters, vhc=8, phc=8)
    blob = seeded_blob(d, 2)
    chunks = filters // 32
    rule = 8 if chunks >= 8 else 4
    forced = [w for w in (1, 2, 4, 8) if w != rule and w <= chunks]
    print(f"# chess {blocks}x{filters}, f16x2, seeded weights; the rule's W = {rule}")
    print("#   n | (d) direct: step_ms spread launch_us | (s) direct_splitk: step_ms spread launch_us | s / d step, launch | "
          + " | ".join(f"W={w}: step_ms launch_us" for w in forced))
    for n in batches:
        pol = torch.empty((n, d.moves), dtype=torch.float32, device=dev)
        val = torch.empty((n,), dtype=torch.float32, device=dev)
        evs = {
            "d": HipEvaluator(blob, batch_size=n, plane_words=1, dtype="f16x2", tower_form="direct", switches={}),
            "s": HipEvaluator(blob, batch_size=n, plane_words=1, dtype="f16x2", tower_form="direct_splitk", switches={}),
        }
        for w in forced:
            evs[f"s{w}"] = HipEvaluator(blob, batch_size=n, plane_words=1, dtype="f16x2", tower_form="direct_splitk", switches={"CATTUS_SPLITK_WAYS": str(w)})
        assert evs["d"].tower_kernel() == "conv3x3_splitw_kernel" and evs["s"].tower_kernel() == "conv3x3_splitk_kernel" and evs["s"].splitk_plan()[0] == rule
        outs = {}
        for k, ev in evs.items():  # warm-up, and what each of them computes
            window(ev, n, pol, val, WARMUP)
            outs[k] = (pol.cpu().numpy().copy(), val.cpu().numpy().copy())
        assert np.array_equal(outs["d"][0], outs["s1"][0]) and np.array_equal(outs["d"][1], outs["s1"][1])  # one way is the direct form
        ms = {k: [] for k in evs}
        for _ in range(REPEATS):
            for k, ev in evs.items():
                ms[k].append(window(ev, n, pol, val, STEPS))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        us = {k: evs[k].time_tower(n, 50)[0] for k in evs}
        print(f"{n:5d} | {med['d']:.4f} {spread['d']:.3f} {us['d']:7.2f} | {med['s']:.4f} {spread['s']:.3f} {us['s']:7.2f} | {med['s'] / med['d']:.3f} {us['s'] / us['d']:.3f} | "
              + " | ".join(f"{med[f's{w}']:.4f} {us[f's{w}']:7.2f}" for w in forced), flush=True)
        for ev in evs.values():
            ev.close()
    # the reference's threading model: THREADS blocking threads, one leaf per call, max_batch = THREADS
    rates = {"direct": [], "direct_splitk": []}
    for _ in range(SERVE_ROUNDS):
        for form in rates:
            with HipEvaluator(blob, batch_size=THREADS, plane_words=1, dtype="f16x2", tower_form=form, switches={}) as ev:
                served(ev, d)  # warm-up
                rates[form].append(served(ev, d))
                st = ev.stats()
        per_batch = st["positions"] / max(1, st["batches"])
    print(f"# served, {THREADS} blocking threads x one leaf per call, max_batch {THREADS}, {SERVE_ROUNDS} rounds alternating (leaves/s): "
          + "; ".join(f"{form} " + " ".join(f"{r:.0f}" for r in v) for form, v in rates.items()) + f"; last run: {per_batch:.1f} leaves per batch", flush=True)
