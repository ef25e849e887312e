"""The f16 tower with an f32 residual stream (dtype f16r) without a GPU: cattus_amd/csrc/f16r_rule.h, which conv3x3_f16r_kernel's
epilogue and the evaluator's enqueue function are written with.

tests/f16r_rule_check.cpp is a stand-alone program around the header.  It is built with the host compiler twice -- plain, and with
-fsanitize=address,undefined -- and both are run as programs.  In the program: the epilogue of one output element against a
restatement on the bits (the fused multiply-add, the f32 skip, ReLU, the pixel mask, the clamp of the copy alone, the count) and
against dtype f16's epilogue -- without a skip the copy is that tower's value bit for bit, with one the two differ within the bound
tests/test_f16r_gpu.py holds the device to; the three lane buffers through towers of 0 .. 6 blocks (conv1 reads the copy of the
current stream, conv2 its block's middle and adds the stream in place, no layer reads a buffer it writes, the heads read the last
stream); every point's tap layout decoded, with and without shifts, out of a buffer of exactly the lane's size.

Here also: the kernel and the evaluator call the header, the header is part of the build, the dtype has one number everywhere, the
library builds and no instance of the new kernel uses scratch or spills."""

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
    d = tmp_path_factory.mktemp("f16r_rule")
    exes = []
    for name, extra in (("f16r_rule_check", []), ("f16r_rule_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / name
        subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *extra, f"-I{CSRC}", str(HERE / "f16r_rule_check.cpp"), "-o", str(exe)])
        exes.append(exe)
    return exes


def test_epilogue_buffer_plan_and_tap_layouts_plain_and_under_sanitizers(rule_checks):
    for exe in rule_checks:
        run = subprocess.run([str(exe)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.rstrip().endswith("f16r rule ok"), run.stdout[-3000:] + run.stderr[-3000:]


def test_the_kernel_and_the_evaluator_are_written_with_the_rule():
    k = (CSRC / "kernels.hip").read_text()
    for name in ("f16r_finish", "F16rOut", "conv3x3_f16r_kernel", "ConvF16R"):
        assert re.search(rf"\b{name}\b", k), name
    # the new instances are listed once, through the family's for_each_conv, and opted in for their LDS like every family
    assert len(re.findall(r"&conv3x3_f16r_kernel<", k)) == 1
    assert re.search(r"conv_opt_in<ConvF16R>", k) and re.search(r"launch_conv_family<ConvF16R>", k)
    e = (CSRC / "evaluator.hip").read_text()
    for name in ("f16r_layer", "f16r_layers", "f16r_stream_layer", "f16r_is_last", "f16r_head_input", "f16r_tap_source", "launch_conv3x3_f16r", "PerLayerStream"):
        assert re.search(rf"\b{name}\b", e), name
    assert CSRC / "f16r_rule.h" in HIP_DEPS


def test_the_dtype_has_one_number_in_the_header_and_in_the_binding():
    from cattus_amd import evaluator

    assert evaluator.DTYPE_F16R == 6
    assert evaluator._DTYPES_F16R == {"f16r": 6}
    assert sorted({**evaluator._DTYPES, **evaluator._DTYPES_WINO_F32, **evaluator._DTYPES_F16R}.values()) == [0, 1, 2, 3, 4, 5, 6]
    header = (ROOT / "include" / "cattus_hip.h").read_text()
    assert re.search(r"^\s*CATTUS_DTYPE_F16R = 6,", header, re.M)


def test_the_self_player_hands_the_dtype_through():
    """model.inference.dtype reaches HipEvaluator as it is, and HipEvaluator looks it up in the merged table."""
    sp = (ROOT / "cattus_amd" / "selfplay.py").read_text()
    assert re.search(r"dtype=inf\.get\(\"dtype\", \"f16x2\"\)", sp)
    ev = (ROOT / "cattus_amd" / "evaluator.py").read_text()
    assert "**_DTYPES_F16R}[dtype]" in ev


def test_the_library_builds_and_no_new_instance_uses_scratch():
    build_hip()
    out = subprocess.run([sys.executable, str(ROOT / "scripts" / "kernel_regs.py"), "conv3x3_f16r"], capture_output=True, text=True, check=True).stdout
    rows = [line.split() for line in out.splitlines()[1:] if line.strip()]
    # <R, BIG, STEM, CB, PBW> without R && STEM, PBW = 1 on CB = 1 only: the f16 family's 18
    assert len(rows) == 18 and all("conv3x3_f16r_kernel" in " ".join(r[6:]) for r in rows), out
    for vgpr, agpr, _sgpr, scratch, spills, *_ in rows:
        assert int(scratch) == 0 and int(spills) == 0 and int(vgpr) + int(agpr) <= 512, out
