#!/usr/bin/env python3
"""The f32 heads' FC pair as short chains (cattus_hip_head_chain) against the MFMA pair: whole step by net, dtype and batch size.

One process, ONE evaluator per (net, dtype, leaves); the setting alternates off / on round by round on that evaluator, so both sides
share weights, buffers, clocks and whatever else the box is doing.  step_ms: cattus_hip_eval_device with planes, logits and values
resident in HBM, ROUNDS rounds of STEPS steps per setting behind a warm-up, wall clock around a drained stream, the MINIMUM over the
rounds (and the rounds' spread (max - min) / min).  The outputs of both settings are compared bit for bit.

    python scripts/head_chain_time.py NET DTYPE [leaves ...]  >> profiles/head_chain.txt
    NET: hex7_6x64 | chess7x16 | chess20x256
One call per (net, dtype): a caller gives each its own time limit."""
import os
import sys
import time

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cattus_amd import synth  # noqa: E402
from cattus_amd.evaluator import HipEvaluator  # noqa: E402
from cattus_amd.weights import CHESS, NetDesc, hex_game, seeded_blob  # noqa: E402

STEPS, WARMUP, ROUNDS = 300, 100, 3
NETS = {
    "hex7_6x64": (NetDesc(**hex_game(7), blocks=6, filters=64, vhc=16, phc=16), 2, (32, 128, 512)),
    "chess7x16": (NetDesc(**CHESS, blocks=7, filters=16, vhc=8, phc=8), 1, (1, 8, 64, 256)),
    "chess20x256": (NetDesc(**CHESS, blocks=20, filters=256, vhc=8, phc=8), 1, (1, 16, 64, 256)),
}
name, dtype = sys.argv[1], sys.argv[2]
d, words, batches = NETS[name]
batches = [int(a) for a in sys.argv[3:]] or batches
if not torch.cuda.is_available():
    raise SystemExit("head_chain_time.py measures on the GPU and there is none")
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
blob = seeded_blob(d, 1)
planes = synth.random_hex_planes(max(batches), d.board, 1) if name.startswith("hex") else synth.random_chess_planes(max(batches), 1)
d_planes = torch.from_numpy(planes.view("int64")).to(dev)


def window(ev, n, pol, val, steps):
    for _ in range(steps):
        ev.eval_device(d_planes.data_ptr(), n, pol.data_ptr(), val.data_ptr(), stream.cuda_stream)
    stream.synchronize()


print(f"# {name} {dtype}: {ROUNDS} rounds x {STEPS} steps per setting, alternating on one evaluator; step_ms = min over the rounds (spread = (max - min) / min)")
print("#   n | off (head_fc_pair_kernel<float>): step_ms spread | on (head_fc_chain_kernel): step_ms spread | on / off | same bits")
for n in batches:
    pol = torch.empty((n, d.moves), dtype=torch.float32, device=dev)
    val = torch.empty((n,), dtype=torch.float32, device=dev)
    with HipEvaluator(blob, batch_size=n, plane_words=words, dtype=dtype, switches={}) as ev:
        ms, outs = {0: [], n: []}, {}
        for k in (0, n):  # warm-up, and what each setting computes
            ev.head_chain(k)
            assert ev.head_chain_leaves() == k, "the setting is ignored on this evaluator"
            window(ev, n, pol, val, WARMUP)
            outs[k] = (pol.cpu().numpy().copy(), val.cpu().numpy().copy())
        same = np.array_equal(outs[0][0].view(np.uint32), outs[n][0].view(np.uint32)) and np.array_equal(outs[0][1].view(np.uint32), outs[n][1].view(np.uint32))
        for _ in range(ROUNDS):
            for k in (0, n):
                ev.head_chain(k)
                window(ev, n, pol, val, 20)
                t0 = time.perf_counter()
                window(ev, n, pol, val, STEPS)
                ms[k].append((time.perf_counter() - t0) / STEPS * 1e3)
        assert ev.head_chain_batches() == WARMUP + ROUNDS * (STEPS + 20)
        lo = {k: min(v) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / min(v) for k, v in ms.items()}
        print(f"{n:5d} | {lo[0]:.4f} {spread[0]:.3f} | {lo[n]:.4f} {spread[n]:.3f} | {lo[n] / lo[0]:.3f} | {'yes' if same else 'NO'}", flush=True)
