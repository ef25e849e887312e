#!/usr/bin/env python3
"""dtype f16r_resident beside the towers it is an alternative to on networks of at most 64 filters, on one box, alternating in one process:
milliseconds per whole step (planes, logits, values resident in HBM) through cattus_hip_eval_device, and launches per pass and
microseconds per tower launch from cattus_hip_time_tower.

  f16r_resident   tower64_stream_kernel, one launch (the f32 stream in registers), then the two f32 head launches
  f16r            conv3x3_f16r_kernel / conv3x3_mfma_v2_kernel<_Float16>, 1 + 2 * blocks launches, then the two f32 head launches: the same bits
  f16 resident    tower64_lds_kernel<_Float16>, one launch, then the two f32 head launches
  f16x2           tower64_split_kernel with the head convs in its tail, then the FC launch
  bf16            tower64_lds_kernel<__bf16> with the head convs in its tail, then the FC launch

Cases: hex7 6x64 (BASELINE config 2) at 32 / 128 / 512 leaves, chess 7x16 (chess_dev.yaml) at 64 / 256 leaves.

RECOMMENDATION (the project's rule: only where f16r_resident beats f16r in the same process by more than the 12 % two boxes differ by;
its step beside f16 resident's, the less accurate tower in the same form, and f16x2's, the more accurate one, is reported).
Measured on one MI355X (profiles/f16r_resident.txt; the script derives the verdicts in its last lines from its own figures): RECOMMENDED
OVER f16r ON ALL FIVE SHAPES -- hex7 6x64 at 32 / 128 / 512 leaves 0.042 / 0.043 / 0.059 ms per step against 0.072 / 0.075 / 0.110 (42-47 %
less time), chess 7x16 at 64 / 256 leaves 0.050 / 0.053 against 0.083 / 0.094 (40-43 %).  No shape was measured on which it is not.  Beside
the other towers: 1.02-1.04x f16 resident's step (inside the spread: the same speed), 0.67-0.86x f16x2's, 1.6-1.7x bf16's.  Not measured:
in-kernel stamps or counters, filter counts other than 64 and 16 (padded to 64), two evaluators sharing a device.

    python scripts/f16r_resident_time.py > profiles/f16r_resident.txt
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

NEW = "f16r_resident"
WAYS = ((NEW, "f16r_resident", "auto"), ("f16r", "f16r", "auto"), ("f16 resident", "f16", "resident"), ("f16x2", "f16x2", "auto"), ("bf16", "bf16", "auto"))
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
        # the two f16r towers are one arithmetic: the figures below are of the same bits
        outs = {name: evs[name].eval(planes) for name in (NEW, "f16r")}
        same_bits = all((a.view("uint32") == b.view("uint32")).all() for a, b in zip(outs[NEW], outs["f16r"]))
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
        print("## %s (seed 2), %d leaves; f16r_resident and f16r: %s" % (label, n, "the same bits" if same_bits else "DIFFERENT BITS"))
        for name, r in rows.items():
            r["saturated"] = evs[name].stats()["saturated"]
            print(name.ljust(14), json.dumps(r))
        res = min(rows[NEW]["ms_per_step"])
        for other in ("f16r", "f16 resident", "f16x2", "bf16"):
            print("%s / %s: %.2fx the time per step" % (NEW, other, res / min(rows[other]["ms_per_step"])))
        gain = 1.0 - res / min(rows["f16r"]["ms_per_step"])
        verdicts.append("%s at %d leaves: f16r_resident is %.0f %% %s per step than f16r: %s; %.2fx f16 resident's step, %.2fx f16x2's" % (
            label, n, abs(gain) * 100, "faster" if gain >= 0 else "slower",
            "RECOMMENDED" if gain > SPREAD else "not recommended (inside the %.0f %% two boxes differ by)" % (SPREAD * 100) if gain >= 0 else "NOT RECOMMENDED",
            res / min(rows["f16 resident"]["ms_per_step"]), res / min(rows["f16x2"]["ms_per_step"])))
        sys.stdout.flush()
        for ev in evs.values():
            ev.close()
print("## recommendation (f16r_resident against f16r, same process, same bits; recommended only beyond the %.0f %% two boxes differ by)" % (SPREAD * 100))
for v in verdicts:
    print(v)
print("# not measured: in-kernel stamps or counters of tower64_stream_kernel, filter counts other than 64 and 16 (padded to 64), two evaluators sharing a device")
