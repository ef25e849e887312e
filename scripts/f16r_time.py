#!/usr/bin/env python3
"""dtype f16r beside the towers it is an alternative to, on one box, alternating in one process (as scripts/f16w_time.py does):
microseconds per conv launch from cattus_hip_time_tower and milliseconds per whole step (planes, logits, values resident in HBM)
through cattus_hip_eval_device.

  f16r    conv3x3_f16r_kernel for the stem and every conv2, the f16 layer for every conv1: one launch per layer
  f16     the direct single-term f16 tower: conv3x3_mfma_v2_kernel
  f16w    conv3x3_wino_f16_kernel, one launch per layer (8x8 boards, >= 128 filters: not on hex7 6x64)
  f16x2   the default tower as tower_form auto gives it (Winograd in one launch from 129 leaves on chess, direct below; resident on hex7 6x64)

Cases: chess 20x256 (the bench weights, seed 2) at 64 / 128 / 256 leaves, chess 4x128 at 256, hex7 6x64 at 128.

    python scripts/f16r_time.py > profiles/f16r_first_build.txt
"""
import json
import os
import sys
import time

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
sys.path.insert(0, ".")
import torch  # noqa: E402

from cattus_amd import synth  # noqa: E402
from cattus_amd.evaluator import HipEvaluator  # noqa: E402
from cattus_amd.weights import CHESS, NetDesc, hex_game, seeded_blob  # noqa: E402

WAYS = (("f16r", "f16r"), ("f16", "f16"), ("f16w", "f16w"), ("f16x2", "f16x2"))
CASES = (("chess", 20, 256, 2, 64), ("chess", 20, 256, 2, 128), ("chess", 20, 256, 2, 256), ("chess", 4, 128, 1, 256), ("hex7", 6, 64, 1, 128))
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
print("# launch_us: mean over the stem and the tower layers of a pass (cattus_hip_time_tower, 50 passes); ms_per_step: 300 steps back to back through")
print("# cattus_hip_eval_device; three rounds, the ways alternating in one process; ratios are min over min")
for game, blocks, filters, seed, n in CASES:
    chess = game == "chess"
    d = NetDesc(**(CHESS if chess else hex_game(7)), blocks=blocks, filters=filters, vhc=8 if chess else 16, phc=8 if chess else 16)
    blob = seeded_blob(d, seed)
    planes = synth.random_chess_planes(n, seed) if chess else synth.random_hex_planes(n, 7, seed)
    d_planes = torch.from_numpy(planes.view("int64")).to(dev)
    pol = torch.empty((n, d.moves), dtype=torch.float32, device=dev)
    val = torch.empty((n,), dtype=torch.float32, device=dev)
    ways = [w for w in WAYS if chess or w[0] != "f16w"]
    evs = {name: HipEvaluator(blob, batch_size=n, plane_words=planes.shape[2], dtype=dtype, tower_form="auto", switches={}) for name, dtype in ways}
    rows = {name: {"kernel": ev.tower_kernel(), "launches": ev.time_tower(n, 1)[1], "launch_us": [], "ms_per_step": []} for name, ev in evs.items()}
    for rep in range(3):
        for name, ev in evs.items():
            ev.time_tower(n, 20)  # warm
            rows[name]["launch_us"].append(round(ev.time_tower(n, 50)[0], 2))
            for _ in range(100):
                ev.eval_device(d_planes.data_ptr(), n, pol.data_ptr(), val.data_ptr(), stream.cuda_stream)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(300):
                ev.eval_device(d_planes.data_ptr(), n, pol.data_ptr(), val.data_ptr(), stream.cuda_stream)
            torch.cuda.synchronize()
            rows[name]["ms_per_step"].append(round((time.perf_counter() - t0) / 300 * 1e3, 4))
    print("## %s %dx%d (seed %d), %d leaves" % (game, blocks, filters, seed, n))
    for name, r in rows.items():
        r["saturated"] = evs[name].stats()["saturated"]
        print(name.ljust(8), json.dumps(r))
    w = rows["f16r"]
    for other in [name for name, _ in ways if name != "f16r"]:
        o = rows[other]
        # (a one-launch tower's launch_us is per layer for the Winograd tower and per launch for the resident one: compare steps there)
        print("f16r / %s: %.2fx the time per launch, %.2fx the time per step" % (other, min(w["launch_us"]) / min(o["launch_us"]), min(w["ms_per_step"]) / min(o["ms_per_step"])))
    sys.stdout.flush()
    for ev in evs.values():
        ev.close()
