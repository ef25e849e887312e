"""The one-launch LDS-resident form of the f16r tower (dtype f16r_resident) without a GPU: cattus_amd/csrc/t64r_rule.h, which
tower64_stream_kernel's epilogue and the evaluator's layer table are written with.

tests/t64r_rule_check.cpp is a stand-alone program around the header.  It is built with the host compiler twice -- plain, and with
-fsanitize=address,undefined -- and both are run as programs.  In the program: the ownership map (wave, lane, block, element) -> (row,
channel) as a bijection onto the workgroup's rows x 64 channels for both workgroup shapes and for 64- and 128-slot boards, the LDS
address it gives against the address a conv's fragment read takes that element from, the f32 row index of the last layer's store; the
two LDS buffers and the layer table through towers of 0 .. 6 blocks; the resident plan (stream in registers, two LDS buffers) beside
f16r_rule.h's per-layer plan, every tensor tagged with the layer that wrote it: the same operand, skip source and destination in every
layer, and the heads read the same stream.

Here also: the kernel and the evaluator call the header and f16r_finish is the only place the new epilogue finishes an element, the
header is part of the build, the dtype has one number everywhere and the older tables are what they were, the library holds exactly
four instances of the new kernel without scratch or spills, and the eight resident and eighteen f16r instances are still there."""

import re
import subprocess
import sys
from pathlib import Path

import pytest

from cattus_amd.build import CSRC, HIP_DEPS, build_hip

from test_weight_layout import host_compiler

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


@pytest.fixture(scope="module")
def rule_checks(tmp_path_factory):
    """The stand-alone program, plain and under AddressSanitizer + UBSan (run as programs: no preloading of anything)."""
    d = tmp_path_factory.mktemp("t64r_rule")
    exes = []
    for name, extra in (("t64r_rule_check", []), ("t64r_rule_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / name
        subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *extra, f"-I{CSRC}", str(HERE / "t64r_rule_check.cpp"), "-o", str(exe)])
        exes.append(exe)
    return exes


def test_ownership_buffers_and_dataflow_plain_and_under_sanitizers(rule_checks):
    for exe in rule_checks:
        run = subprocess.run([str(exe)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.rstrip().endswith("t64r rule ok"), run.stdout[-3000:] + run.stderr[-3000:]


def kernel_function(text, signature):
    """The body of the function whose definition starts with `signature`, by brace matching."""
    at = text.index(signature)
    i = text.index("{", at)
    depth, j = 1, i + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        j += 1
    return text[i:j]


def test_the_kernel_and_the_evaluator_are_written_with_the_rule():
    k = (CSRC / "kernels.hip").read_text()
    tower = kernel_function(k, "__device__ __forceinline__ void tower64_lds_tower(")
    # one copy of the tower: both __global__ functions are a call of it and nothing else
    for wrapper, call in (("tower64_lds_kernel(Tower64Args A)", "tower64_lds_tower<T, CH, BIG, LS, false>(A);"),
                          ("tower64_stream_kernel(Tower64Args A)", "tower64_lds_tower<_Float16, CH, BIG, LS, true>(A);")):
        assert kernel_function(k, wrapper).strip("{} \n") == call, wrapper
    # the new instances are listed once, in for_each_tower64, and opted in for their LDS like the others
    assert len(re.findall(r"&tower64_stream_kernel<", k)) == 1 and len(re.findall(r"&tower64_lds_kernel<", k)) == 1
    assert re.search(r"for_each_tower64<Tower64Stream>\(\[&\]\(auto kernel, int lds, auto\.\.\.\) \{ lds_opt_in\(err, kernel, lds\); \}\);", k)
    # the stream branch of the epilogue: f16r_finish is the only place it finishes an element, the map is the only source of its addresses
    start = tower.index("if (stream_layer) {")
    branch = tower[start:tower.index("} else {  // (not indented: the code as it was)", start)]
    assert len(re.findall(r"\bf16r_finish\(", branch)) == 1 and len(re.findall(r"\bf16r_finish\(", tower)) == 1
    assert not re.search(r"fmaf|65504|> 0\.0f|eoff|eaddr", branch), "the stream branch restates the epilogue or takes an address of its own"
    for name in ("t64r_own", "t64r_lds_offset", "t64r_out_index", "sreg"):
        assert re.search(rf"\b{name}\b", branch), name
    assert "smem" in branch and len(re.findall(r"\bsmem\b", branch)) == 1, "the stream branch touches LDS once: the copy's store"
    for name in ("t64r_reads", "t64r_layer", "t64r_blocks", "t64r_rows", "t64r_npb"):
        assert re.search(rf"\b{name}\b", tower), name
    # only the f16 epilogue branches on STREAM: the flag is named in the asserts, the stream registers' declaration and that epilogue
    epilogue = tower[tower.index("if constexpr (F16T) {\n            // the per-layer f16 epilogue"):tower.index("} else {  // bf16 (not indented")]
    outside = tower.replace(epilogue, "")
    assert len(re.findall(r"\bSTREAM\b", outside)) == 2 and "static_assert(!STREAM ||" in outside and "if constexpr (STREAM) {" in outside
    e = (CSRC / "evaluator.hip").read_text()
    for name in ("t64r_layer", "t64r_layers", "launch_tower64_stream", "Resident64Stream", "f16r_head_input", "CATTUS_DTYPE_F16R_RESIDENT"):
        assert re.search(rf"\b{name}\b", e), name
    assert e.count("fpad == 64 && !sw.starts(\"CATTUS_TOWER64\", '0')") == 1, "resolve_plan's resident predicate, one copy"
    assert '"tower64_stream_kernel"' in e
    assert CSRC / "t64r_rule.h" in HIP_DEPS and CSRC / "f16r_rule.h" in HIP_DEPS
    assert '#include "t64r_rule.h"' in (CSRC / "kernels.h").read_text()


def test_the_dtype_has_one_number_and_the_older_tables_are_what_they_were():
    from cattus_amd import evaluator

    assert evaluator.DTYPE_F16R_RESIDENT == 7
    assert evaluator._DTYPES_F16R_RESIDENT == {"f16r_resident": 7}
    assert evaluator._DTYPES == {"f32": 0, "bf16": 1, "f16x2": 2, "f16": 3, "f16w": 4}
    assert evaluator._DTYPES_WINO_F32 == {"f32w": 5} and evaluator._DTYPES_F16R == {"f16r": 6}
    header = (ROOT / "include" / "cattus_hip.h").read_text()
    assert re.search(r"^\s*CATTUS_DTYPE_F16R_RESIDENT = 7,", header, re.M) and re.search(r"^\s*CATTUS_DTYPE_F16R = 6,", header, re.M)
    src = (ROOT / "cattus_amd" / "evaluator.py").read_text()
    assert "{**_DTYPES_F16R_RESIDENT, **_DTYPES, **_DTYPES_WINO_F32, **_DTYPES_F16R}[dtype]" in src
    # the self-player hands model.inference.dtype through as it is
    assert re.search(r"dtype=inf\.get\(\"dtype\", \"f16x2\"\)", (ROOT / "cattus_amd" / "selfplay.py").read_text())
    assert "F16rResident = 7" in (ROOT / "integration" / "rust" / "hip.rs").read_text()


def regs(substring):
    out = subprocess.run([sys.executable, str(ROOT / "scripts" / "kernel_regs.py"), substring], capture_output=True, text=True, check=True).stdout
    return [line.split() for line in out.splitlines()[1:] if line.strip()], out


def test_the_build_holds_four_stream_instances_without_scratch_beside_the_old_ones():
    lib = build_hip()
    rows, out = regs("tower64_stream_kernel")
    print(out)
    assert len(rows) == 4, out
    for vgpr, agpr, _sgpr, scratch, spills, *_ in rows:
        assert int(scratch) == 0 and int(spills) == 0 and int(vgpr) + int(agpr) <= 256, out
    syms = lib.read_bytes()
    for shape in ("Li4ELb0ELb0E", "Li4ELb0ELb1E", "Li2ELb0ELb0E", "Li2ELb1ELb0E"):  # CH, BIG, LS
        assert f"tower64_stream_kernelI{shape}".encode() in syms, shape
    assert len(regs("tower64_lds_kernel")[0]) == 8
    assert len(regs("conv3x3_f16r")[0]) == 18
