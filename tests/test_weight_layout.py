"""The host-side weight layouts (cattus_amd/csrc/weight_layout.h) without a GPU: tests/weight_layout_check.cpp fills a folded layer
with distinct codes and checks, for the f32 / bf16 / f16 rows, the f16x2 rows and fragment order and the Winograd U, that every weight
sits exactly once at the index the kernel-side helpers name (split_frag_index, wino_frag_index, the row formulas of kernels.h),
that every other element is zero, that hi + lo times the inverse scale gives the weight back exactly, and that one-hot 3x3 filters
give the known rows of G g G^T -- on the smallest shapes that reach every index term (cout 3 -> 64; cin 5 -> 32 and 70 -> 96; U:
128 -> 128 and 130 -> 192).  The header uses _Float16, so the program is built with the clang++ that hipcc drives as its host compiler."""

import shutil
import subprocess
from pathlib import Path

from cattus_amd.build import CSRC, _hipcc

HERE = Path(__file__).resolve().parent


def host_compiler() -> str:
    beside_hipcc = Path(_hipcc()).resolve().parent
    for cand in (shutil.which("clang++"), beside_hipcc / "clang++", beside_hipcc.parent / "llvm" / "bin" / "clang++",
                 beside_hipcc.parent / "lib" / "llvm" / "bin" / "clang++", shutil.which("amdclang++")):
        if cand and Path(cand).exists():
            return str(cand)
    raise RuntimeError("no host C++ compiler with _Float16 found")


def test_every_layout_places_every_weight_once_and_nothing_else(tmp_path):
    exe = tmp_path / "weight_layout_check"
    # -ffp-contract=off: as the library itself is built (cattus_amd/build.py)
    subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", f"-I{CSRC}", str(HERE / "weight_layout_check.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "weight layouts ok" in run.stdout, run.stdout[-4000:] + run.stderr[-2000:]
