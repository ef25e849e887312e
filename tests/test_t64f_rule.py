"""The one-launch LDS-resident form of the exact f32 tower (dtype f32_resident) without a GPU: cattus_amd/csrc/t64f_rule.h, which
tower64_f32_kernel and the evaluator's layer table, chunk count and workgroup-shape choice are written with.

tests/t64f_rule_check.cpp is a stand-alone program around the header.  It is built with the host compiler twice -- plain, and with
-fsanitize=address,undefined -- and both are run as programs.  In the program: the LDS regions of the three instances (disjoint, 16-byte
aligned, at most 163,840 B); the step table of towers of 0 .. 6 blocks at 16 / 32 / 33 / 64 filters beside the per-layer walk, its ring
slots within the look-ahead of two, its source offsets inside the layer's weight rows, the narrow walk; the ownership map as a bijection
onto rows x 64 channels; the offset the epilogue stores to against the offset the next layer's fragment read takes (row, k) from; the
bank slots of the fragment reads and of the epilogue's stores; the resident dataflow beside the per-layer f32 plan, every tensor tagged
with the layer that wrote it.

Here also: the kernel and the evaluator call the header, header and file are part of the build, the dtype has one number everywhere and
the older tables are what they were, the library holds exactly three instances of the new kernel without scratch or spills, and the
eight resident, four stream and eighteen f16r instances are still there."""

import re
import subprocess
import sys
from pathlib import Path

import pytest

from cattus_amd.build import CSRC, HIP_DEPS, HIP_SOURCES, build_hip

from test_weight_layout import host_compiler

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


@pytest.fixture(scope="module")
def rule_checks(tmp_path_factory):
    """The stand-alone program, plain and under AddressSanitizer + UBSan (run as programs: no preloading of anything)."""
    d = tmp_path_factory.mktemp("t64f_rule")
    exes = []
    for name, extra in (("t64f_rule_check", []), ("t64f_rule_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / name
        subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *extra, f"-I{CSRC}", str(HERE / "t64f_rule_check.cpp"), "-o", str(exe)])
        exes.append(exe)
    return exes


def test_lds_plan_steps_ownership_banks_and_dataflow_plain_and_under_sanitizers(rule_checks):
    for exe in rule_checks:
        run = subprocess.run([str(exe)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.rstrip().endswith("t64f rule ok"), run.stdout[-3000:] + run.stderr[-3000:]


def test_the_kernel_and_the_evaluator_are_written_with_the_rule():
    k = (CSRC / "kernels_t64f.hip").read_text()
    # the kernel takes every LDS offset, the step table, the ownership map, the tap rows and the layer table from the header
    for name in ("t64f_rows", "t64f_npb", "t64f_lds", "t64f_steps", "t64f_step", "t64f_ring_slot", "t64f_slab_src", "t64f_row_bytes", "t64f_piece_src", "t64f_piece_dst",
                 "t64f_own", "t64f_lds_offset", "t64f_out_index", "t64f_tap", "t64f_wfrag_offset", "t64f_layer", "t64f_blocks", "t64f_layer_chunks", "T64F_AHEAD", "T64F_SLAB"):
        assert re.search(rf"\b{name}\b", k), name
    assert not re.search(r"\b(73728|24576|107008|139776|16640|33024)\b", k), "an LDS offset restated as a number"
    # the shared pieces come from device_common.h; the loaders use LDS-DMA only
    assert '#include "device_common.h"' in k and "glds16(" in k and "wait_vm_barrier<" in k and "Mfma<float>::mac(" in k
    assert len(re.findall(r"__global__", k)) == 1 and "tower64_f32_kernel(Tower64F32Args A)" in k
    for other in ("tower64_lds_kernel<", "tower64_stream_kernel<", "conv3x3_f16r"):
        assert other not in k, other
    assert "nch = (int)A.nch" in k and not re.search(r"template <[^>]*NCH", k), "the chunk count is a kernel argument, not a template parameter"
    e = (CSRC / "evaluator.hip").read_text()
    for name in ("t64f_layer", "t64f_layers", "t64f_hidden_chunks", "t64f_ch", "launch_tower64_f32", "Resident64F32", "CATTUS_DTYPE_F32_RESIDENT", "CATTUS_T64F_NARROW"):
        assert re.search(rf"\b{name}\b", e), name
    assert e.count("fpad == 64 && !sw.starts(\"CATTUS_TOWER64\", '0')") == 1, "resolve_plan's resident predicate, one copy"
    assert "if (!(resident && cpad0 == 32))" in e and '"tower64_f32_kernel"' in e
    assert CSRC / "t64f_rule.h" in HIP_DEPS and CSRC / "kernels_t64f.hip" in HIP_SOURCES
    assert '#include "t64f_rule.h"' in (CSRC / "kernels.h").read_text()
    assert "prepare_tower64_f32()" in (CSRC / "kernels.hip").read_text(), "the dynamic-LDS opt-in, once per device at create"


def test_the_dtype_has_one_number_and_the_older_tables_are_what_they_were():
    from cattus_amd import evaluator

    assert evaluator.DTYPE_F32_RESIDENT == 9
    assert evaluator._DTYPES_F32_RESIDENT == {"f32_resident": 9}
    assert evaluator._DTYPES == {"f32": 0, "bf16": 1, "f16x2": 2, "f16": 3, "f16w": 4}
    assert evaluator._DTYPES_WINO_F32 == {"f32w": 5} and evaluator._DTYPES_F16R == {"f16r": 6} and evaluator._DTYPES_F16R_RESIDENT == {"f16r_resident": 7}
    assert "CATTUS_T64F_NARROW" in evaluator.DIAG_SWITCHES
    header = (ROOT / "include" / "cattus_hip.h").read_text()
    assert re.search(r"^\s*CATTUS_DTYPE_F32_RESIDENT = 9,", header, re.M) and re.search(r"^\s*CATTUS_DTYPE_F16R_RESIDENT = 7,", header, re.M)
    assert not re.search(r"^\s*CATTUS_DTYPE_\w+ = 8,", header, re.M) and "8 is unassigned" in header
    src = (ROOT / "cattus_amd" / "evaluator.py").read_text()
    assert "{**_DTYPES_F16R_RESIDENT, **_DTYPES, **_DTYPES_WINO_F32, **_DTYPES_F16R}[dtype]" in src
    assert "_DTYPES_F32_RESIDENT[dtype] if dtype in _DTYPES_F32_RESIDENT else" in src
    # the self-player hands model.inference.dtype through as it is
    assert re.search(r"dtype=inf\.get\(\"dtype\", \"f16x2\"\)", (ROOT / "cattus_amd" / "selfplay.py").read_text())
    rust = (ROOT / "integration" / "rust" / "hip.rs").read_text()
    assert "F32Resident = 9" in rust and "F16rResident = 7" in rust and not re.search(r"= 8,", rust)


def regs(substring):
    out = subprocess.run([sys.executable, str(ROOT / "scripts" / "kernel_regs.py"), substring], capture_output=True, text=True, check=True).stdout
    return [line.split() for line in out.splitlines()[1:] if line.strip()], out


def test_the_build_holds_three_f32_instances_without_scratch_beside_the_old_ones():
    lib = build_hip()
    rows, out = regs("tower64_f32_kernel")
    print(out)
    assert len(rows) == 3, out
    for vgpr, agpr, _sgpr, scratch, spills, *_ in rows:
        assert int(scratch) == 0 and int(spills) == 0 and int(vgpr) + int(agpr) <= 256, out
    syms = lib.read_bytes()
    for shape in ("Li4ELb0E", "Li2ELb0E", "Li2ELb1E"):  # CH, BIG
        assert f"tower64_f32_kernelI{shape}".encode() in syms, shape
    assert len(regs("tower64_lds_kernel")[0]) == 8
    assert len(regs("tower64_stream_kernel")[0]) == 4
    assert len(regs("conv3x3_f16r")[0]) == 18
