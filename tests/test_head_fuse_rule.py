"""The head convs in the tail of the resident f16 and f16r towers (cattus_hip_fused_heads) without a GPU: cattus_amd/csrc/head_fuse_rule.h,
which the HEADS instances of tower64_lds_tower, the loader waves' operand copy, the chain's epilogue and the evaluator's setter are
written with.

tests/head_fuse_rule_check.cpp is a stand-alone program around the header.  It is built with the host compiler twice -- plain, and with
-fsanitize=address,undefined -- and both are run as programs.  In the program, per instance: the head weights, the biases and the tower's
rows lie inside the instance's unchanged LDS size, pairwise disjoint, and outside every byte the last layer's last step still reads; the pitch
gives conflict-free 16-byte
reads down 32 rows; the ownership map is a bijection onto (row, channel < 32) and is the MFMA accumulator's; an element's k sequence is
head_conv_tile<float>'s walk over K = 64, restated there; the hv index and the rows / channels written are the stand-alone epilogue's for ttt,
hex7, hex9 and chess heads; the predicate names exactly the two f16 plans (the resident f32 tower keeps its head conv launch: its kernel's
body cannot be shared with a HEADS instance without moving the code of the instances that exist).

Here also: kernels and evaluator call the header, the header is part of the build, the ABI has the three functions, the self-player reads
the setting, the timing script starts, the library builds with eight HEADS instances, none with scratch, and the instances that were there
are the ones they were."""

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
    d = tmp_path_factory.mktemp("head_fuse_rule")
    exes = []
    for name, extra in (("head_fuse_rule_check", []), ("head_fuse_rule_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / name
        subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *extra, f"-I{CSRC}", str(HERE / "head_fuse_rule_check.cpp"), "-o", str(exe)])
        exes.append(exe)
    return exes


def test_lds_plan_ownership_chain_and_hv_index_plain_and_under_sanitizers(rule_checks):
    for exe in rule_checks:
        run = subprocess.run([str(exe)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.rstrip().endswith("head fuse rule ok"), run.stdout[-3000:] + run.stderr[-3000:]


def test_the_kernels_and_the_evaluator_are_written_with_the_rule():
    """What the build and the rule program cannot show: that the code under test CALLS the header the program checks."""
    k = (CSRC / "kernels.hip").read_text()
    common = (CSRC / "device_common.h").read_text()
    # the tower takes its plan from the header; the loaders' copy, the chain and its epilogue are device_common.h's
    for name in ("hf_lds_t64", "hf_stage_operands", "hf_head_convs"):
        assert re.search(rf"\b{name}\b", k), name
    for name in ("hf_piece_dst", "hf_tile_of_wave", "hf_own", "hf_w_frag", "hf_writes", "hf_hv_index"):
        assert re.search(rf"\b{name}\b", common), name
    # the chain's order and the hv index are tied to head_conv_tile's at compile time
    assert "static_assert(hf_rule_is_head_conv_tile()" in k
    e = (CSRC / "evaluator.hip").read_text()
    assert re.search(r"\bhf_takes\b", e), "the evaluator's predicate is the header's"
    assert CSRC / "head_fuse_rule.h" in HIP_DEPS
    assert '#include "head_fuse_rule.h"' in (CSRC / "kernels.h").read_text()


def test_the_abi_the_binding_and_the_self_player_have_the_setting():
    from cattus_amd import evaluator

    header = (ROOT / "include" / "cattus_hip.h").read_text()
    for name in ("cattus_hip_fused_heads", "cattus_hip_fused_heads_effective", "cattus_hip_fused_heads_batches"):
        assert name in evaluator.ABI_SYMBOLS and re.search(rf"^int {name}\(", header, re.M), name
    # no new field in the config struct: the setting is a call, as cattus_hip_head_chain is
    assert "fused_heads" not in header[header.index("typedef struct cattus_eval_config"):header.index("} cattus_eval_config;")]
    for method in ("fused_heads", "fused_heads_effective", "fused_heads_batches"):
        assert callable(getattr(evaluator.HipEvaluator, method))
    sp = (ROOT / "cattus_amd" / "selfplay.py").read_text()
    assert re.search(r"fused_heads = bool\(inf\.get\(\"fused_heads\", False\)\)", sp) and "fused_heads=fused_heads" in sp
    assert "cattus_hip_fused_heads" in (ROOT / "INTEGRATION.md").read_text()


def test_the_timing_script_starts_and_names_what_it_needs(tmp_path):
    """scripts/fused_heads_time.py without the parent commit's library: it compiles, parses its arguments and says which file is missing; its
    workers load an older build through CATTUS_HIP_LIB, which the binding lets lack exactly this setting's symbols."""
    from cattus_amd import evaluator

    script = ROOT / "scripts" / "fused_heads_time.py"
    compile(script.read_text(), str(script), "exec")
    missing = tmp_path / "libcattus_hip_parent.so"
    run = subprocess.run([sys.executable, str(script)], env={**__import__("os").environ, "CATTUS_HIP_PARENT_LIB": str(missing)}, capture_output=True, text=True)
    assert run.returncode != 0 and str(missing) in run.stderr and "is missing" in run.stderr, run.stderr[-2000:]
    run = subprocess.run([sys.executable, str(script), "--worker", "sideways"], capture_output=True, text=True)
    assert run.returncode != 0 and "--worker on" in run.stderr
    assert set(evaluator.ABI_NEWER_SYMBOLS) == {n for n in evaluator.ABI_SYMBOLS if "fused_heads" in n}


def regs(substring):
    out = subprocess.run([sys.executable, str(ROOT / "scripts" / "kernel_regs.py"), substring], capture_output=True, text=True, check=True).stdout
    return [line.split() for line in out.splitlines()[1:] if line.strip()], out


def test_the_build_holds_eight_heads_instances_without_scratch_beside_the_old_ones():
    build_hip()
    rows, out = regs("tower_heads_kernel")
    print(out)
    names = sorted(" ".join(r[6:]) for r in rows)
    # <f32 stream, CH, BIG, LS> for dtype f16 and f16r_resident: the shapes their twins have
    want = [f"Tower64Heads<{s}, {shape}>" for s in ("false", "true") for shape in ("2, false, false", "2, true, false", "4, false, false", "4, false, true")]
    assert len(rows) == 8 and all(any(w in n for n in names) for w in want), out
    for vgpr, agpr, _sgpr, scratch, spills, *_ in rows:
        assert int(scratch) == 0 and int(spills) == 0 and int(vgpr) + int(agpr) <= 256, out
    # the instances without the flag, by the names they always had
    assert len(regs("tower64_lds_kernel")[0]) == 8 and len(regs("tower64_stream_kernel")[0]) == 4 and len(regs("tower64_f32_kernel")[0]) == 3
