#!/usr/bin/env python3
"""Short batches of the Winograd tower with and without cattus_eval_config.tail_leaves: whole step and tower launches by batch size.

Three f16x2 evaluators of one network in one process, alternating repeat by repeat:
  (a) default       max_batch 256, tail_leaves 0: tower_wino4_kernel, 4 boards x 64 couts per workgroup -- the baseline
  (b) tail_leaves   the same with tail_leaves = n: conv3x3_wino4s_kernel, 2 boards x 32 couts per workgroup, one launch per layer; the same bits
  (c) direct        max_batch = n, tower_form direct: other bits, another evaluator -- for orientation only
step_ms: cattus_hip_eval_device with planes, logits and values resident in HBM, HIP events around windows of STEPS steps; median over the
REPEATS windows and their spread (max - min) / median.  launch_us: cattus_hip_time_tower, the mean over the stem and the tower's layers.

    python scripts/short_batch_time.py [blocks filters] [n ...]  > profiles/wino_short_batches.txt   (both networks when none is named)"""
import os
import statistics
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cattus_amd import synth  # noqa: E402
from cattus_amd.evaluator import HipEvaluator  # noqa: E402
from cattus_amd.weights import CHESS, NetDesc, seeded_blob  # noqa: E402

STEPS, WARMUP, REPEATS = 200, 100, 7
args = [int(a) for a in sys.argv[1:]]
nets = [(args[0], args[1])] if len(args) >= 2 else [(20, 256), (4, 128)]
batches = args[2:] or [1, 8, 16, 32, 64, 96, 128]
if not torch.cuda.is_available():
    raise SystemExit("short_batch_time.py measures on the GPU and there is none")
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
planes = synth.random_chess_planes(256, 2)
d_planes = torch.from_numpy(planes.view("int64")).to(dev)


def window(ev, n, pol, val, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(steps):
        ev.eval_device(d_planes.data_ptr(), n, pol.data_ptr(), val.data_ptr(), stream.cuda_stream)
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / steps


print(f"# {STEPS} steps per window, {REPEATS} windows per evaluator, alternating; step_ms = median (spread = (max - min) / median); launch_us = cattus_hip_time_tower, 50 passes")
for blocks, filters in nets:
    d = NetDesc(**CHESS, blocks=blocks, filters=filters, vhc=8, phc=8)
    blob = seeded_blob(d, 2)
    print(f"# chess {blocks}x{filters}, f16x2, seeded weights")
    print("#   n | (a) default: step_ms spread launch_us | (b) tail_leaves = n: step_ms spread launch_us | (c) direct, max_batch n: step_ms spread | b / a | same bits")
    for n in batches:
        pol = torch.empty((n, d.moves), dtype=torch.float32, device=dev)
        val = torch.empty((n,), dtype=torch.float32, device=dev)
        evs = {
            "a": HipEvaluator(blob, batch_size=256, plane_words=1, dtype="f16x2", switches={}),
            "b": HipEvaluator(blob, batch_size=256, plane_words=1, dtype="f16x2", switches={}, tail_leaves=n),
            "c": HipEvaluator(blob, batch_size=n, plane_words=1, dtype="f16x2", tower_form="direct", switches={}),
        }
        assert evs["a"].tower_kernel() == evs["b"].tower_kernel() == "tower_wino4_kernel" and evs["b"].tail_leaves() == n
        outs = {}
        for k, ev in evs.items():  # warm-up, and what each of them computes
            window(ev, n, pol, val, WARMUP)
            outs[k] = (pol.cpu().numpy().copy(), val.cpu().numpy().copy())
        same = np.array_equal(outs["a"][0], outs["b"][0]) and np.array_equal(outs["a"][1], outs["b"][1])
        ms = {k: [] for k in evs}
        for _ in range(REPEATS):
            for k, ev in evs.items():
                ms[k].append(window(ev, n, pol, val, STEPS))
        assert evs["b"].tail_batches() == WARMUP + REPEATS * STEPS and evs["a"].tail_batches() == 0
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        us = {k: evs[k].time_tower(n, 50)[0] for k in ("a", "b")}
        print(f"{n:5d} | {med['a']:.4f} {spread['a']:.3f} {us['a']:7.2f} | {med['b']:.4f} {spread['b']:.3f} {us['b']:7.2f} | {med['c']:.4f} {spread['c']:.3f} | "
              f"{med['b'] / med['a']:.3f} | {'yes' if same else 'NO'}", flush=True)
        for ev in evs.values():
            ev.close()
