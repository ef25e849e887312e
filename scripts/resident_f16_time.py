#!/usr/bin/env python3
"""dtype f16 with tower_form "resident" beside the towers it is an alternative to on networks of at most 64 filters, on one box, alternating in
one process: milliseconds per whole step (planes, logits, values resident in HBM) through cattus_hip_eval_device, and launches per pass and
microseconds per tower launch from cattus_hip_time_tower.

  f16 auto        conv3x3_mfma_v2_kernel<_Float16>, 1 + 2 * blocks launches, then the two f32 head launches
  f16 resident    tower64_lds_kernel<_Float16>, one launch, then the two f32 head launches
  bf16            tower64_lds_kernel<__bf16> with the head convs in its tail, then the FC launch
  f16x2           tower64_split_kernel with the head convs in its tail, then the FC launch

Cases: hex7 6x64 (BASELINE config 2) at 32 / 128 / 512 leaves, chess 7x16 (chess_dev.yaml) at 64 / 256 leaves.

RECOMMENDATION (the project's rule: only where resident beats f16 auto in the same process by more than the 12 % two boxes differ by).
Measured on one MI355X (profiles/resident_f16.txt; the script derives the verdicts in its last lines from its own figures): RECOMMENDED FOR
dtype f16 ON ALL FIVE SHAPES -- hex7 6x64 at 32 / 128 / 512 leaves 0.040 / 0.041 / 0.057 ms per step against 0.072 / 0.075 / 0.104 (44-45 % less
time), chess 7x16 at 64 / 256 leaves 0.049 / 0.052 against 0.083 / 0.091 (41-43 %).  No shape was measured on which it is not.  Beside the
other towers: 16-36 % faster than f16x2, 1.5-1.7x bf16's time.  Not measured: in-kernel stamps or counters, filter counts other than 64
and 16 (padded to 64), two evaluators sharing a device.

    python scripts/resident_f16_time.py > profiles/resident_f16.txt
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

WAYS = (("f16 auto", "f16", "auto"), ("f16 resident", "f16", "resident"), ("bf16", "bf16", "auto"), ("f16x2", "f16x2", "auto"))
# (label, game, blocks, filters, leaves)
CASES = (("hex7 6x64", hex_game(7), 6, 64, (32, 128, 512)), ("chess 7x16", CHESS, 7, 16, (64, 256)))
ROUNDS, WARM, STEPS = 3, 100, 300
SPREAD = 0.12  # what two boxes differ by on one binary
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
print("# ms_per_step: %d steps back to back through cattus_hip_eval_device after %d warm ones; launch_us: mean over a pass's tower launches" % (STEPS, WARM))
print("# (cattus_hip_time_tower, 50 passes); %d rounds, the ways alternating in one process; ratios are min over min" % ROUNDS)
verdicts = []
for label, game, blocks, filters, sizes in CASES:
    d = NetDesc(**game, blocks=blocks, filters=filters, vhc=8, phc=8)
    blob = seeded_blob(d, 2)
    for n in sizes:
        planes = synth.random_chess_planes(n, 2) if game is CHESS else synth.random_hex_planes(n, d.board, 2)
        d_planes = torch.from_numpy(planes.view("int64")).to(dev)
        pol = torch.empty((n, d.moves), dtype=torch.float32, device=dev)
        val = torch.empty((n,), dtype=torch.float32, device=dev)
        evs = {name: HipEvaluator(blob, batch_size=n, plane_words=planes.shape[2], dtype=dtype, tower_form=form, switches={}) for name, dtype, form in WAYS}
        rows = {name: {"kernel": ev.tower_kernel(), "launches": ev.time_tower(n, 1)[1], "launch_us": [], "ms_per_step": []} for name, ev in evs.items()}
        for rep in range(ROUNDS):
            for name, ev in evs.items():
                ev.time_tower(n, 20)  # warm
                rows[name]["launch_us"].append(round(ev.time_tower(n, 50)[0], 2))
                for _ in range(WARM):
                    ev.eval_device(d_planes.data_ptr(), n, pol.data_ptr(), val.data_ptr(), stream.cuda_stream)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(STEPS):
                    ev.eval_device(d_planes.data_ptr(), n, pol.data_ptr(), val.data_ptr(), stream.cuda_stream)
                torch.cuda.synchronize()
                rows[name]["ms_per_step"].append(round((time.perf_counter() - t0) / STEPS * 1e3, 4))
        print("## %s (seed 2), %d leaves" % (label, n))
        for name, r in rows.items():
            r["saturated"] = evs[name].stats()["saturated"]
            print(name.ljust(14), json.dumps(r))
        res = min(rows["f16 resident"]["ms_per_step"])
        for other in ("f16 auto", "bf16", "f16x2"):
            print("f16 resident / %s: %.2fx the time per step" % (other, res / min(rows[other]["ms_per_step"])))
        gain = 1.0 - res / min(rows["f16 auto"]["ms_per_step"])
        verdicts.append("%s at %d leaves: resident is %.0f %% %s per step than f16 auto: %s" % (
            label, n, abs(gain) * 100, "faster" if gain >= 0 else "slower", "RECOMMENDED" if gain > SPREAD else "not recommended (inside the %.0f %% two boxes differ by)" % (SPREAD * 100) if gain >= 0 else "NOT RECOMMENDED"))
        sys.stdout.flush()
        for ev in evs.values():
            ev.close()
print("## recommendation (resident against f16 auto, same process; recommended only beyond the %.0f %% two boxes differ by)" % (SPREAD * 100))
for v in verdicts:
    print(v)
print("# not measured: in-kernel stamps or counters of the f16 instantiations, filter counts other than 64 and 16 (padded to 64), two evaluators sharing a device")
