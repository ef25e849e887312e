"""The small-tile Winograd kernel's geometry without a GPU: cattus_amd/csrc/wino4s_rule.h, which conv3x3_wino4s_kernel is written with.

tests/wino4s_rule_check.cpp is a stand-alone program around the header.  It is built with the host compiler twice -- plain, and with
-fsanitize=address,undefined -- and both are run as programs.  In the program: the grid map is a bijection onto (board pair, cout
block) for 128 / 192 / 256 / 384 filters and 4 / 8 / 20 / 256 padded boards, and with the XCD map the cout blocks of a pair share
index % 8 wherever an XCD's share of the grid is whole pairs; the transform's threads cover every (tile, channel pair) once; V-image,
chunk and exchange offsets stay inside their areas and on bytes of their own; the LDS total fits 160 KiB; the lane groups of every
16-byte read and write of the V images and of the exchange fall on 16 different bank slots (tests/test_wino4_layout.py's enumeration).

Here also: the sizes cattus_eval_config has had, as the header states them and as the Python binding lays the structure out."""

import ctypes
import re
import subprocess
from pathlib import Path

import pytest

from cattus_amd.build import CSRC

from test_weight_layout import host_compiler

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


@pytest.fixture(scope="module")
def rule_checks(tmp_path_factory):
    """The stand-alone program, plain and under AddressSanitizer + UBSan (run as programs: no preloading of anything)."""
    d = tmp_path_factory.mktemp("wino4s_rule")
    exes = []
    for name, extra in (("wino4s_rule_check", []), ("wino4s_rule_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / name
        subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *extra, f"-I{CSRC}", str(HERE / "wino4s_rule_check.cpp"), "-o", str(exe)])
        exes.append(exe)
    return exes


def test_grid_items_offsets_and_bank_slots_plain_and_under_sanitizers(rule_checks):
    for exe in rule_checks:
        run = subprocess.run([str(exe)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.rstrip().endswith("wino4s rule ok"), run.stdout[-3000:] + run.stderr[-3000:]


def test_the_kernel_is_written_with_the_rule():
    """Every LDS address and every index of the kernel goes through the header's functions: no offset arithmetic of its own."""
    k = (CSRC / "kernels_wino4s.hip").read_text()
    for name in ("wino4s_grid", "wino4s_logical", "wino4s_pair", "wino4s_cout_block", "wino4s_item_tile", "wino4s_item_chp", "wino4s_v_image", "wino4s_v_write",
                 "wino4s_v_read", "wino4s_chunk_buffer", "wino4s_piece_row", "wino4s_piece_dst", "wino4s_patch_read", "wino4s_z", "wino4s_out_pixel",
                 "wino4s_out_row", "wino4s_out_tile", "W4S_LDS_TOTAL"):
        assert re.search(rf"\b{name}\b", k), name


def test_config_sizes_are_stated_in_the_header_and_match_the_binding():
    from cattus_amd.evaluator import EvalConfig

    header = (ROOT / "include" / "cattus_hip.h").read_text()
    struct = header[header.index("typedef struct cattus_eval_config {"):header.index("} cattus_eval_config;")]
    fields = re.findall(r"^\s*(u?int32_t) (\w+);", struct, re.M)
    assert [name for _, name in fields] == [name for name, _ in EvalConfig._fields_]
    assert fields[-1][1] == "tail_leaves" and fields[-2][1] == "tower_form"
    assert ctypes.sizeof(EvalConfig) == 4 * len(fields) == 32
    assert EvalConfig.tower_form.offset == 24 and EvalConfig.tail_leaves.offset == 28  # the two earlier lengths
    comment = struct[:struct.index("uint32_t struct_size;")]
    for size in (24, 28, 32):
        assert re.search(rf"\b{size}\b", comment), size
