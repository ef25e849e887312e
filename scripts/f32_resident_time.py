#!/usr/bin/env python3
"""dtype f32_resident beside the tower it is another way of launching and the resident towers of the other arithmetics on networks of at
most 64 filters, on one box, alternating in one process: milliseconds per whole step (planes, logits, values resident in HBM) through
cattus_hip_eval_device, and launches per pass and microseconds per tower launch from cattus_hip_time_tower.

  f32_resident    tower64_f32_kernel, one launch, then the two f32 head launches
  f32             conv3x3_mfma_v2_kernel<float>, 1 + 2 * blocks launches, then the two f32 head launches: the same bits (the yardstick)
  f16x2           tower64_split_kernel with the head convs in its tail, then the FC launch
  f16r_resident   tower64_stream_kernel, one launch, then the two f32 head launches

On the 16-filter network also f32_resident with CATTUS_T64F_NARROW=0 (both chunks of every hidden layer walked: the same bits).

Cases: hex7 6x64 (BASELINE config 2) at 32 / 128 / 512 leaves, chess 7x16 (chess_dev.yaml) at 64 / 256 leaves.

RECOMMENDATION (the project's rule: only where f32_resident beats f32 in the same process, on the same binary, by more than the 12 % two
boxes differ by; the script derives the verdicts in its last lines from its own figures).  Measured on one MI355X
(profiles/f32_resident.txt): RECOMMENDED OVER f32 ON ALL FIVE SHAPES -- hex7 6x64 at 32 / 128 / 512 leaves 0.142 / 0.143 / 0.250 ms per step
against 0.168 / 0.171 / 0.309 (16-19 % less time: narrowly), chess 7x16 at 64 / 256 leaves 0.100 / 0.102 against 0.195 / 0.206 (49-51 %; with
both chunks walked 0.164 / 0.166).  It stays 1.6-2.8x f16x2's step and 1.9-4.3x f16r_resident's.  The estimate of DESIGN.md (K1rf: 0.115-0.125
ms at hex7 6x64, 128 leaves) was missed.  Not measured: in-kernel stamps or counters, the clock under this load, filter counts other than
64 and 16, two evaluators sharing a device, self-play.

    python scripts/f32_resident_time.py > profiles/f32_resident.txt
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

NEW, WIDE = "f32_resident", "f32_resident, both chunks"
# (name, dtype, switches)
WAYS = ((NEW, "f32_resident", {}), ("f32", "f32", {}), ("f16x2", "f16x2", {}), ("f16r_resident", "f16r_resident", {}))
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
    ways = WAYS + (((WIDE, "f32_resident", {"CATTUS_T64F_NARROW": "0"}),) if filters <= 32 else ())
    for n in sizes:
        planes = synth.random_chess_planes(n, 2) if game is CHESS else synth.random_hex_planes(n, d.board, 2)
        d_planes = torch.from_numpy(planes.view("int64")).to(dev)
        pol = torch.empty((n, d.moves), dtype=torch.float32, device=dev)
        val = torch.empty((n,), dtype=torch.float32, device=dev)
        evs = {name: HipEvaluator(blob, batch_size=n, plane_words=planes.shape[2], dtype=dtype, switches=dict(sw)) for name, dtype, sw in ways}
        rows = {name: {"kernel": ev.tower_kernel(), "launches": ev.time_tower(n, 1)[1], "launch_us": [], "ms_per_step": []} for name, ev in evs.items()}
        # the f32 towers are one arithmetic: the figures below are of the same bits
        f32_ways = [name for name, dtype, _ in ways if dtype.startswith("f32")]
        outs = {name: evs[name].eval(planes) for name in f32_ways}
        same_bits = all((a.view("uint32") == b.view("uint32")).all() for name in f32_ways for a, b in zip(outs[name], outs["f32"]))
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
        print("## %s (seed 2), %d leaves; the f32 towers: %s" % (label, n, "the same bits" if same_bits else "DIFFERENT BITS"))
        for name, r in rows.items():
            r["saturated"] = evs[name].stats()["saturated"]
            print(name.ljust(26), json.dumps(r))
        res = min(rows[NEW]["ms_per_step"])
        for other in [name for name in rows if name != NEW]:
            print("%s / %s: %.2fx the time per step" % (NEW, other, res / min(rows[other]["ms_per_step"])))
        gain = 1.0 - res / min(rows["f32"]["ms_per_step"])
        verdicts.append("%s at %d leaves: f32_resident is %.0f %% %s per step than f32 (%.4f against %.4f ms): %s; %.2fx f16x2's step, %.2fx f16r_resident's" % (
            label, n, abs(gain) * 100, "faster" if gain >= 0 else "slower", res, min(rows["f32"]["ms_per_step"]),
            "RECOMMENDED" if gain > SPREAD else "no difference (inside the %.0f %% two boxes differ by)" % (SPREAD * 100) if abs(gain) <= SPREAD else "NOT RECOMMENDED",
            res / min(rows["f16x2"]["ms_per_step"]), res / min(rows["f16r_resident"]["ms_per_step"])))
        if WIDE in rows:
            verdicts.append("%s at %d leaves: the narrow walk takes %.2fx the step of both chunks (%.4f against %.4f ms; one launch of %.1f against %.1f us)" % (
                label, n, res / min(rows[WIDE]["ms_per_step"]), res, min(rows[WIDE]["ms_per_step"]), min(rows[NEW]["launch_us"]), min(rows[WIDE]["launch_us"])))
        sys.stdout.flush()
        for ev in evs.values():
            ev.close()
print("## recommendation (f32_resident against f32, same process, same binary, same bits; recommended only beyond the %.0f %% two boxes differ by)" % (SPREAD * 100))
for v in verdicts:
    print(v)
print("# not measured: in-kernel stamps or counters of tower64_f32_kernel, filter counts other than 64 and 16 (padded to 64), two evaluators sharing a device, self-play")
