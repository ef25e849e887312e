"""The short-chain form of the f32 FC pair (cattus_hip_head_chain) without a GPU: cattus_amd/csrc/head_chain_rule.h, which
head_fc_chain_kernel and the evaluator are written with.

tests/head_chain_rule_check.cpp is a stand-alone program around the header.  It is built with the host compiler twice -- plain, and
with -fsanitize=address,undefined -- and both are run as programs; nothing is loaded into Python.  In the program: the grid map
(workgroup, thread, slot) -> (leaf, output unit) as a bijection for every n in 1 .. 70 and the (J, K) of the heads the GPU tests run,
the walk order against the order derived from the MFMA lane pair, the operand offsets against tap_frag_index and inside the operands'
allocations, the dot product over the walk against a plain kperm loop bit for bit (random values, rows of zeros, a partial sum that
underflows to -0), and the epilogues against restatements.

Here also: the kernel is written with the header, the header and the new file are part of the build, no fast-math or contraction flag
reaches it, kernels.hip asserts the order, the ABI has the three calls, and the library holds the two instances without scratch."""

import re
import subprocess
import sys
from pathlib import Path

import pytest

from cattus_amd.build import CSRC, HIP_DEPS, HIP_SOURCES, HIPCC_FLAGS, build_hip

from test_weight_layout import host_compiler

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


@pytest.fixture(scope="module")
def rule_checks(tmp_path_factory):
    """The stand-alone program, plain and under AddressSanitizer + UBSan (run as programs: no preloading of anything)."""
    d = tmp_path_factory.mktemp("head_chain_rule")
    exes = []
    for name, extra in (("head_chain_rule_check", []), ("head_chain_rule_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / name
        subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *extra, f"-I{CSRC}", str(HERE / "head_chain_rule_check.cpp"), "-o", str(exe)])
        exes.append(exe)
    return exes


def test_grid_walk_offsets_dot_and_epilogues_plain_and_under_sanitizers(rule_checks):
    for exe in rule_checks:
        run = subprocess.run([str(exe)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.rstrip().endswith("head chain rule ok"), run.stdout[-3000:] + run.stderr[-3000:]


def test_the_kernel_and_the_evaluator_are_written_with_the_rule():
    k = (CSRC / "kernels_head_chain.hip").read_text()
    for name in ("hc_map", "hc_load_row", "hc_load_leaf", "hc_piece_index", "hc_steps", "hc_step", "hc_fc1_epilogue", "hc_policy_epilogue", "hc_fc2_sum",
                 "hc_leaves_per_lane", "hc_grid_x", "hc_grid_y", "hc_lds_bytes", "hc_lds_hidden_at", "hc_hv_policy_at", "HC_STEP_STRIDE", "HC_HALF_STRIDE", "tanh_exact"):
        assert re.search(rf"\b{name}\b", k), name
    code = "\n".join(line.split("//")[0] for line in k.splitlines())
    # the arithmetic is the header's: the kernel file itself holds no fmaf, no product, no scrub constant
    assert not re.search(r"fmaf|3\.40282347e\+38|> 0\.0f", code), "the kernel restates arithmetic that head_chain_rule.h owns"
    assert "__builtin_amdgcn_mfma" not in code and "Mfma<" not in code, "the chain form issues no MFMA"
    # no second upload, no new layout: the launcher takes the operands launch_heads_mfma takes
    assert "const HeadsMfma& hd" in k and "launch_heads_conv(act, tower, nb, F, hd, st)" in k
    assert "static_assert(hc_order_is_kperm()" in (CSRC / "kernels.hip").read_text()
    e = (CSRC / "evaluator.hip").read_text()
    assert e.count("launch_heads_chain(") == 1 and e.count("launch_heads_mfma(") == 1, "heads_mfma picks one of the two launchers, nothing else changes"
    assert "!obs && !tt && chain_leaves && n <= chain_leaves" in e
    assert '#include "head_chain_rule.h"' in (CSRC / "kernels.h").read_text()


def test_the_build_has_the_file_and_no_fast_math():
    assert CSRC / "kernels_head_chain.hip" in HIP_SOURCES and CSRC / "head_chain_rule.h" in HIP_DEPS
    assert "-ffp-contract=off" in HIPCC_FLAGS
    assert not [f for f in HIPCC_FLAGS if "fast" in f or f.startswith("-ffp-contract=") and f != "-ffp-contract=off" or "unsafe" in f or "reciprocal" in f]
    src = (CSRC / "kernels_head_chain.hip").read_text()
    assert "#pragma clang fp" not in src and "STDC FP_CONTRACT" not in src


def test_the_abi_has_the_three_calls_and_the_configuration_is_what_it_was():
    import ctypes

    from cattus_amd import evaluator

    header = (ROOT / "include" / "cattus_hip.h").read_text()
    for name in ("cattus_hip_head_chain", "cattus_hip_head_chain_leaves", "cattus_hip_head_chain_batches"):
        assert name in evaluator.ABI_SYMBOLS and re.search(rf"^int {name}\(", header, re.M), name
    assert ctypes.sizeof(evaluator.EvalConfig) == 32
    sp = (ROOT / "cattus_amd" / "selfplay.py").read_text()
    assert 'inf.get("head_chain_leaves", 0)' in sp and "head_chain_leaves=head_chain_leaves" in sp


def test_the_library_holds_both_instances_without_scratch():
    build_hip()
    out = subprocess.run([sys.executable, str(ROOT / "scripts" / "kernel_regs.py"), "head_fc_chain_kernel"], capture_output=True, text=True, check=True).stdout
    rows = [line.split() for line in out.splitlines()[1:] if line.strip()]
    assert len(rows) == 2, out
    for vgpr, agpr, _sgpr, scratch, spills, *_ in rows:
        assert int(scratch) == 0 and int(spills) == 0 and int(vgpr) + int(agpr) <= 256, out
