#!/usr/bin/env python3
"""dtype f32w beside the exact tower it is an alternative to, on one box, alternating in one process (as scripts/f16w_time.py does):
microseconds per conv launch from cattus_hip_time_tower and milliseconds per whole step (planes, logits, values resident in HBM)
through cattus_hip_eval_device.

  f32                    the exact tower: conv3x3_mfma_v2_kernel<float>, the baseline (measured here, in the same process)
  f32w                   conv3x3_wino_f32_kernel, one launch per layer (the first build)
  f16x2, one launch      tower_form winograd as shipped: tower_wino4_kernel (time_tower reports its duration per layer), for orientation

Cases: chess 20x256 (the bench weights, seed 2) at 64 / 128 / 256 leaves, and chess 4x128 at 256.  The estimate this build was begun on:
about 55 us per 256 -> 256 layer at 256 leaves (wino_f32_rule.h's step of 32 NCB MFMAs of 64 cycles, 16 steps, 512 workgroups in two
rounds); the last lines say what was measured against it.

    python scripts/f32w_time.py > profiles/f32w_first_build.txt
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
from cattus_amd.weights import CHESS, NetDesc, seeded_blob  # noqa: E402

WAYS = (("f32", "f32", "auto", {}), ("f32w", "f32w", "auto", {}), ("f16x2, one launch", "f16x2", "winograd", {}))
CASES = ((20, 256, 2, 64), (20, 256, 2, 128), (20, 256, 2, 256), (4, 128, 1, 256))
ESTIMATE_US = 55.0
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
print("# launch_us: mean over the stem and the tower layers of a pass (cattus_hip_time_tower, 50 passes); ms_per_step: 300 steps back to back through")
print("# cattus_hip_eval_device; three rounds, the ways alternating in one process; ratios are min over min; node-evals/s = leaves / min ms_per_step")
for blocks, filters, seed, n in CASES:
    d = NetDesc(**CHESS, blocks=blocks, filters=filters, vhc=8, phc=8)
    blob, planes = seeded_blob(d, seed), synth.random_chess_planes(n, seed)
    d_planes = torch.from_numpy(planes.view("int64")).to(dev)
    pol = torch.empty((n, d.moves), dtype=torch.float32, device=dev)
    val = torch.empty((n,), dtype=torch.float32, device=dev)
    evs = {name: HipEvaluator(blob, batch_size=n, plane_words=planes.shape[2], dtype=dtype, tower_form=form, switches=sw) for name, dtype, form, sw in WAYS}
    rows = {name: {"kernel": ev.tower_kernel(), "launch_us": [], "ms_per_step": []} for name, ev in evs.items()}
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
    print("## chess %dx%d (seed %d), %d leaves" % (blocks, filters, seed, n))
    for name, r in rows.items():
        r["saturated"] = evs[name].stats()["saturated"]
        r["node_evals_per_s"] = round(n / (min(r["ms_per_step"]) * 1e-3))
        print(name.ljust(20), json.dumps(r))
    w = rows["f32w"]
    for other in ("f32", "f16x2, one launch"):
        o = rows[other]
        print("f32w / %s: %.2fx the time per launch, %.2fx the time per step" % (other, min(w["launch_us"]) / min(o["launch_us"]), min(w["ms_per_step"]) / min(o["ms_per_step"])))
    if (blocks, filters, n) == (20, 256, 256):
        print("estimate: %.0f us per layer; measured: %.2f us per launch (mean over the stem and the 40 layers), %.2fx the estimate" % (ESTIMATE_US, min(w["launch_us"]), min(w["launch_us"]) / ESTIMATE_US))
    sys.stdout.flush()
    for ev in evs.values():
        ev.close()
