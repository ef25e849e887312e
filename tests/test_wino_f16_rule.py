"""The single-term f16 Winograd kernel's geometry and transforms without a GPU: cattus_amd/csrc/wino_f16_rule.h, which
conv3x3_wino_f16_kernel (dtype f16w) is written with.

tests/wino_f16_rule_check.cpp is a stand-alone program around the header.  It is built with the host compiler twice -- plain, and with
-fsanitize=address,undefined -- and both are run as programs.  In the program: the grid map is a bijection onto (board pair, cout
group) for one and for two cout blocks per workgroup, 128 / 192 / 256 / 384 filters and 4 .. 256 padded boards (grids that are and are
not multiples of 8), and the rule that chooses between one and two blocks; the transform's threads cover every (tile, channel) of a
chunk once; V-image, chunk and exchange offsets stay inside their areas and on bytes of their own, the exchange over V image 0 alone;
the LDS total fits 160 KiB; the lane groups of every 16-byte read and write of the V images and of the exchange fall on 16 different
bank slots and the 4-byte V writes of a half wave on 32 banks; the U index is a bijection onto the buffer, agrees with the kernel's
stage offset and with the builder; the header's B^T / G / A^T orders reproduce the matrices, and together the 3x3 correlation,
against float64 on random data.

Here also: the kernel source calls the header's functions, and the dtype's number in the header and in the Python binding."""

import re
import subprocess
from pathlib import Path

import pytest

from cattus_amd.build import CSRC, HIP_DEPS, HIP_SOURCES

from test_weight_layout import host_compiler

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


@pytest.fixture(scope="module")
def rule_checks(tmp_path_factory):
    """The stand-alone program, plain and under AddressSanitizer + UBSan (run as programs: no preloading of anything)."""
    d = tmp_path_factory.mktemp("wino_f16_rule")
    exes = []
    for name, extra in (("wino_f16_rule_check", []), ("wino_f16_rule_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / name
        subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *extra, f"-I{CSRC}", str(HERE / "wino_f16_rule_check.cpp"), "-o", str(exe)])
        exes.append(exe)
    return exes


def test_grid_items_offsets_bank_slots_u_index_and_transforms_plain_and_under_sanitizers(rule_checks):
    for exe in rule_checks:
        run = subprocess.run([str(exe)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.rstrip().endswith("wino_f16 rule ok"), run.stdout[-3000:] + run.stderr[-3000:]


def test_the_kernel_is_written_with_the_rule():
    """Every LDS address, every index and both transforms of the kernel go through the header's functions."""
    k = (CSRC / "kernels_wino_f16.hip").read_text()
    for name in ("wf16_ncb", "wf16_grid", "wf16_logical", "wf16_pair", "wf16_cout_group", "wf16_u_stage", "wf16_item_tile", "wf16_item_chp", "wf16_v_image",
                 "wf16_v_write", "wf16_v_read", "wf16_chunk_buffer", "wf16_piece_row", "wf16_piece_dst", "wf16_patch_read", "wf16_z", "wf16_out_pixel",
                 "wf16_out_row", "wf16_out_tile", "wf16_bt", "wf16_at", "WF16_LDS_TOTAL", "WF16_VF", "WF16_VHALF", "WF16_DHALF", "WF16_UD"):
        assert re.search(rf"\b{name}\b", k), name
    # the builder writes U through the index the header's stage offset is checked against
    assert re.search(r"\bwino_f16_frag_index\b", (CSRC / "weight_layout.h").read_text())
    assert re.search(r"\bwino_u_f16\b", (CSRC / "evaluator.hip").read_text())


def test_the_kernel_and_its_rule_are_part_of_the_build():
    assert CSRC / "kernels_wino_f16.hip" in HIP_SOURCES
    assert CSRC / "wino_f16_rule.h" in HIP_DEPS


def test_the_dtype_has_one_number_in_the_header_and_in_the_binding():
    from cattus_amd.evaluator import _DTYPES

    assert _DTYPES["f16w"] == 4
    assert sorted(_DTYPES.values()) == [0, 1, 2, 3, 4]
    header = (ROOT / "include" / "cattus_hip.h").read_text()
    assert re.search(r"^\s*CATTUS_DTYPE_F16W = 4,", header, re.M)
