#!/usr/bin/env python3
"""cattus_hip_fused_heads (the head convs in the tail of the resident f16 and f16r towers) beside the parent commit's build, on one box:
milliseconds per whole step (planes, logits, values resident in HBM) through cattus_hip_eval_device.

Columns per dtype ("f16" under tower_form resident, "f16r_resident"):

  parent      the parent commit's library (CATTUS_HIP_PARENT_LIB, default cattus_amd/libcattus_hip_parent.so: build the parent commit and copy
              its libcattus_hip.so there), selected with CATTUS_HIP_LIB as scripts/step_time.py / ab_step_libs.sh do
  parent'     the same file once more: parent' / parent is the method's run-to-run spread
  off         this build, the setting off: must lie within that spread of the parent
  on          this build, the setting on: the same bits (a sha256 of logits and values per case, compared across the four ways)

Cases: hex7 6x64 at 32 / 128 / 512 leaves, chess 7x16 at 64 / 256 leaves, hex7 7x16 at 128 leaves.  A way runs in a process of its own (one
library per process); the four ways alternate, three rounds; a round times every case once, 300 steps behind 100 warm ones; the minimum of
the three rounds counts.  RECOMMENDED for a shape only where `on` beats the parent by more than the 12 % two boxes differ by on one
binary; otherwise "not recommended", as for cattus_hip_head_chain.  Not measured: in-kernel stamps, hardware counters, the tower launch
alone, two evaluators sharing a device.

    python scripts/fused_heads_time.py > profiles/fused_heads.txt
    python scripts/fused_heads_time.py --worker on          # one way, one round: a JSON line (what the first form starts twelve times)
"""
import hashlib
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
WAYS = ("parent", "parent'", "off", "on")
DTYPES = (("f16 resident", "f16", "resident"), ("f16r_resident", "f16r_resident", "auto"))
# (label, game, blocks, filters, leaves)
CASES = (("hex7 6x64", "hex7", 6, 64, (32, 128, 512)), ("chess 7x16", "chess", 7, 16, (64, 256)), ("hex7 7x16", "hex7", 7, 16, (128,)))
ROUNDS, WARM, STEPS = 3, 100, 300
SPREAD = 0.12  # what two boxes differ by on one binary
WORKER_TIMEOUT = 150  # seconds: twelve evaluators and 4,800 steps of at most a few hundred microseconds


def worker(way):
    """Every case under every dtype once, in this process's library: {"case | leaves | dtype": [ms per step, sha256 of the outputs]}."""
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
    sys.path.insert(0, str(ROOT))
    import torch

    from cattus_amd import synth
    from cattus_amd.evaluator import HipEvaluator
    from cattus_amd.weights import CHESS, NetDesc, hex_game, seeded_blob

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    out = {}
    for label, game, blocks, filters, sizes in CASES:
        d = NetDesc(**(CHESS if game == "chess" else hex_game(7)), blocks=blocks, filters=filters, vhc=8, phc=8)
        blob = seeded_blob(d, 2)
        for n in sizes:
            planes = synth.random_chess_planes(n, 2) if game == "chess" else synth.random_hex_planes(n, d.board, 2)
            d_planes = torch.from_numpy(planes.view("int64")).to(dev)
            pol = torch.empty((n, d.moves), dtype=torch.float32, device=dev)
            val = torch.empty((n,), dtype=torch.float32, device=dev)
            for name, dtype, form in DTYPES:
                with HipEvaluator(blob, batch_size=n, plane_words=planes.shape[2], dtype=dtype, tower_form=form, switches={}) as ev:
                    if way == "on":
                        ev.fused_heads(True)
                        assert ev.fused_heads_effective()
                    p, v = ev.eval(planes)
                    digest = hashlib.sha256(p.tobytes() + v.tobytes()).hexdigest()[:16]
                    for _ in range(WARM):
                        ev.eval_device(d_planes.data_ptr(), n, pol.data_ptr(), val.data_ptr(), stream.cuda_stream)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(STEPS):
                        ev.eval_device(d_planes.data_ptr(), n, pol.data_ptr(), val.data_ptr(), stream.cuda_stream)
                    torch.cuda.synchronize()
                    out["%s | %d | %s" % (label, n, name)] = [round((time.perf_counter() - t0) / STEPS * 1e3, 4), digest]
    print(json.dumps(out))


def main():
    parent_lib = Path(os.environ.get("CATTUS_HIP_PARENT_LIB", ROOT / "cattus_amd" / "libcattus_hip_parent.so"))
    if not parent_lib.exists():
        raise SystemExit(f"{parent_lib} is missing: build the parent commit and copy its libcattus_hip.so there (or set CATTUS_HIP_PARENT_LIB)")
    ms, digests = {}, {}
    for rep in range(ROUNDS):
        for way in WAYS:
            env = dict(os.environ)
            env.pop("CATTUS_HIP_LIB", None)
            if way.startswith("parent"):
                env["CATTUS_HIP_LIB"] = str(parent_lib)
            run = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--worker", way], env=env, capture_output=True, text=True, timeout=WORKER_TIMEOUT)
            if run.returncode != 0:  # a way that failed ends the measurement: nothing more is started on the device
                raise SystemExit("way %r, round %d: exit status %d\n%s" % (way, rep, run.returncode, run.stderr[-3000:]))
            print("round %d, way %s: done" % (rep, way), file=sys.stderr, flush=True)
            for key, (t, digest) in json.loads(run.stdout.strip().splitlines()[-1]).items():
                ms.setdefault(key, {}).setdefault(way, []).append(t)
                digests.setdefault(key, set()).add(digest)
    best = {key: {way: min(v) for way, v in by_way.items()} for key, by_way in ms.items()}
    method_spread = max(abs(b["parent'"] / b["parent"] - 1.0) for b in best.values())
    print("# method spread (parent' against parent, the same file in processes of their own, worst of all rows): %.1f %%" % (method_spread * 100))
    print("# ms per whole step through cattus_hip_eval_device: %d steps back to back after %d warm ones; %d rounds, the four ways alternating, a process each; the minimum" % (STEPS, WARM, ROUNDS))
    for key, b in best.items():
        rel = {way: (b[way] / b["parent"] - 1.0) * 100 for way in WAYS}
        print("%-36s parent %.4f  parent' %.4f (%+.1f %%)  off %.4f (%+.1f %%)  on %.4f (%+.1f %%)  %s  rounds %s" % (
            key, b["parent"], b["parent'"], rel["parent'"], b["off"], rel["off"], b["on"], rel["on"], "the same bits" if len(digests[key]) == 1 else "DIFFERENT BITS",
            json.dumps(ms[key])))
    print("## the off path (this build with the setting off against the parent; must lie within the method spread of %.1f %%)" % (method_spread * 100))
    for key, b in best.items():
        off = b["off"] / b["parent"] - 1.0
        print("%s: off is %+.1f %% of the parent: %s" % (key, off * 100, "within the spread" if abs(off) <= method_spread else "OUTSIDE THE SPREAD"))
    print("## recommendation (on against the parent; recommended only beyond the %.0f %% two boxes differ by)" % (SPREAD * 100))
    for key, b in best.items():
        on = b["on"] / b["parent"] - 1.0
        print("%s: on is %.1f %% %s per step than the parent: %s" % (key, abs(on) * 100, "faster" if on <= 0 else "slower",
                                                                  "RECOMMENDED" if -on > SPREAD else "not recommended" if on <= 0 else "NOT RECOMMENDED"))
    print("# not measured: in-kernel stamps, hardware counters, the tower launch alone, two evaluators sharing a device")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--worker" and sys.argv[2] in WAYS:
        worker(sys.argv[2])
    elif len(sys.argv) == 1:
        main()
    else:
        raise SystemExit(__doc__)
