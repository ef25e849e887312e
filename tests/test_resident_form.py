"""tower_form RESIDENT without a GPU: the number in the header and in the bindings, the engine JSON's name for it, and the kernels the build
holds for it -- tower64_lds_kernel as a template over its element type, four workgroup shapes each for bf16 and for f16, none with scratch.
tests/test_resident_f16_gpu.py holds the f16 instantiations to the per-layer f16 tower, bit for bit, on the device."""

import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_the_form_has_one_number_in_the_header_and_in_the_binding():
    from cattus_amd import evaluator

    header = (ROOT / "include" / "cattus_hip.h").read_text()
    assert re.search(r"CATTUS_TOWER_RESIDENT = 5,", header)
    assert re.search(r"CATTUS_TOWER_DIRECT_SPLITK = 4,", header)
    assert evaluator.TOWER_FORMS_RESIDENT == {"resident": 5}
    assert evaluator.TOWER_FORMS == {"auto": 0, "direct": 1, "winograd": 2, "winograd_f4": 3, "direct_splitk": 4}  # the five old entries, exactly
    import ctypes

    assert ctypes.sizeof(evaluator.EvalConfig) == 32 and len(evaluator.EvalConfig._fields_) == 8  # no field was added for it
    assert "unknown tower_form" in (ROOT / "cattus_amd" / "csrc" / "evaluator.hip").read_text()
    assert re.search(r"tower_form > CATTUS_TOWER_RESIDENT\)", (ROOT / "cattus_amd" / "csrc" / "evaluator.hip").read_text())


def test_the_engine_json_names_the_form():
    from cattus_amd.selfplay import tower_form_from_inference

    assert tower_form_from_inference({"tower_form": "resident"}) == "resident"
    assert tower_form_from_inference({}) == "auto"
    assert tower_form_from_inference({"tower_form": "direct_splitk"}) == "direct_splitk"
    with pytest.raises(SystemExit) as ei:
        tower_form_from_inference({"tower_form": "residant"})
    assert "'resident'" in str(ei.value) and "'auto'" in str(ei.value) and "residant" in str(ei.value)


def test_the_build_holds_eight_resident_instantiations_without_scratch():
    """The library cross-compiles for gfx950 (build_hip: what `python -m cattus_amd.build` runs for it, skipped where the library is newer than
    every source) and scripts/kernel_regs.py finds tower64_lds_kernel<T, CH, BIG, LS> for T = __bf16, _Float16 over (4, no, no), (4, no, yes),
    (2, no, no), (2, yes, no): no scratch, no spilled register, at most the 256 VGPRs that two 512-thread workgroups per CU leave a thread."""
    from cattus_amd.build import build_hip

    lib = build_hip()
    assert lib.exists()
    p = subprocess.run([sys.executable, str(ROOT / "scripts" / "kernel_regs.py"), "tower64_lds_kernel"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    print(p.stdout)
    rows = [l.split() for l in p.stdout.splitlines()[1:] if l.strip()]
    assert len(rows) == 8, p.stdout
    for vgpr, agpr, sgpr, scratch, spills, *_ in rows:
        assert int(scratch) == 0 and int(spills) == 0 and int(vgpr) + int(agpr) <= 256, p.stdout
    # the element type is in the mangled name: DF16_ = _Float16, DF16b = __bf16; then CH, BIG, LS
    syms = lib.read_bytes()
    for t in ("DF16_", "DF16b"):
        for shape in ("Li4ELb0ELb0E", "Li4ELb0ELb1E", "Li2ELb0ELb0E", "Li2ELb1ELb0E"):
            assert f"tower64_lds_kernelI{t}{shape}".encode() in syms, (t, shape)
