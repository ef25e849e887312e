#!/usr/bin/env python3
"""The f16x2 tower's three Winograd ways on one box, alternating in one process (as scripts/by_batch_forms.py does): microseconds per conv
launch from cattus_hip_time_tower and milliseconds per whole step (planes, logits, values resident in HBM).

  winograd, per layer   tower_form winograd with CATTUS_WINO_PERSIST=0: conv3x3_wino4_kernel, one launch per layer -- the fair twin of
  winograd, one launch  tower_form winograd as shipped: tower_wino4_kernel (time_tower reports its duration per layer)
  winograd_f4           tower_form winograd_f4: conv3x3_winof4_kernel, one launch per layer (the first build)

    python scripts/winof4_time.py [workload] [batch] > profiles/winof4_first_build.txt
"""
import json
import os
import sys
import time

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
sys.path.insert(0, ".")
import torch  # noqa: E402

import bench  # noqa: E402
from cattus_amd.evaluator import HipEvaluator  # noqa: E402

workload = sys.argv[1] if len(sys.argv) > 1 else "chess20x256"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 256
d, blob, planes = bench.make_workload(workload)
dev = torch.device("cuda", 0)
d_planes = torch.from_numpy(planes.view("int64")).to(dev)
stream = torch.cuda.Stream(device=dev)
pol = torch.empty((n, d.moves), dtype=torch.float32, device=dev)
val = torch.empty((n,), dtype=torch.float32, device=dev)
WAYS = (("winograd, per layer", "winograd", {"CATTUS_WINO_PERSIST": "0"}), ("winograd, one launch", "winograd", {}), ("winograd_f4", "winograd_f4", {}))
evs = {name: HipEvaluator(blob, batch_size=n, plane_words=planes.shape[2], dtype="f16x2", tower_form=form, switches=sw) for name, form, sw in WAYS}
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
print("# %s, %d leaves, f16x2; launch_us: mean over the stem and the %d tower layers of a pass (cattus_hip_time_tower, 50 passes);" % (workload, n, 2 * d.blocks))
print("# ms_per_step: 300 steps back to back; three rounds, the ways alternating in one process")
for name, r in rows.items():
    r["saturated"] = evs[name].stats()["saturated"]
    print(name.ljust(22), json.dumps(r))
twin, f4 = rows["winograd, per layer"], rows["winograd_f4"]
print("winograd_f4 / winograd per layer: %.2fx the time per launch, %.2fx the time per step" %
      (min(f4["launch_us"]) / min(twin["launch_us"]), min(f4["ms_per_step"]) / min(twin["ms_per_step"])))
print("winograd_f4 / winograd one launch: %.2fx the time per step" % (min(f4["ms_per_step"]) / min(rows["winograd, one launch"]["ms_per_step"])))
for ev in evs.values():
    ev.close()
