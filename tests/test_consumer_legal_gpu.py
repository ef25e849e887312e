"""integration/c/consumer_legal.c on the GPU box: T threads, one leaf per call, through cattus_hip_apply + a host softmax (mode A) and
through cattus_hip_apply_legal (mode B), from plain C.  Both modes must report the same number of leaves and the program must exit 0; the
rates it prints are scripts/server_legal_cost.py's business, not this test's."""

import json
import os
import subprocess
from pathlib import Path

import pytest

from cattus_amd import synth
from cattus_amd.weights import CHESS, NetDesc, seeded_blob

from test_many_planes_gpu import random_planes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_c_consumer_legal_runs_both_modes(tmp_path):
    exe = tmp_path / "consumer_legal"
    libdir = ROOT / "cattus_amd"
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-D_POSIX_C_SOURCE=200809L", f"-I{ROOT / 'include'}", str(ROOT / "integration" / "c" / "consumer_legal.c"),
                           "-o", str(exe), f"-L{libdir}", "-lcattus_hip", "-lpthread", "-lm", f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib"])
    d = NetDesc(**CHESS, blocks=1, filters=16, vhc=4, phc=4)
    n = 40
    lists = synth.random_legal_lists(n, d.moves, 0, 60, 5)
    lists[3] = lists[3][:0]  # a position without a legal move
    (tmp_path / "model.cattus").write_bytes(seeded_blob(d, 41))
    synth.write_legal_leaves(tmp_path / "leaves.bin", random_planes(d, 1, n, 43), lists)
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([str(exe), str(tmp_path / "model.cattus"), str(tmp_path / "leaves.bin"), "0", "8", "4", "1", "1"],
                         capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    assert res["A"]["leaves"] == res["B"]["leaves"] == n and res["threads"] == 4 and res["moves"] == d.moves
    assert res["A"]["d2h_bytes_per_leaf"] == 4 * d.moves + 4 and res["B"]["d2h_bytes_per_leaf"] < res["A"]["d2h_bytes_per_leaf"]
