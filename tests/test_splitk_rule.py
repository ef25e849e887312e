"""The split-K direct kernel's rule without a GPU: cattus_amd/csrc/splitk_rule.h, which conv3x3_splitk_kernel is written with.

tests/splitk_rule_check.cpp is a stand-alone program around the header.  It is built with the host compiler twice -- plain, and with
-fsanitize=address,undefined -- and both are run as programs.  In the program: for every chunk count from 4 to the header's bound (16:
512 filters) and every forced way count, the waves' ranges are contiguous, non-empty and partition [0, chunks), and nothing but the chunk
count enters them; the reduction walk reads every partial exactly once and spells the pairwise tree by wave index; the grid map is a
bijection onto (board, cout block) and keeps a board's cout blocks on one XCD where an XCD's share is whole boards; images, zero areas
and exchange tiles lie on bytes of their own and the total fits 160 KiB; the lane groups of every ds_read_b128 (pixel fragments on
boards of edge 1..8, the exchange's reads) and every ds_write_b128 (image fill, the exchange's writes) are enumerated as conflict-free;
reads off the board stay in the zero area.

Here also: the form's number in the binding and the header, and that cattus_eval_config's layout did not move."""

import ctypes
import re
import subprocess
from pathlib import Path

import pytest

from cattus_amd.build import CSRC, HIP_SOURCES

from test_weight_layout import host_compiler

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


@pytest.fixture(scope="module")
def rule_checks(tmp_path_factory):
    """The stand-alone program, plain and under AddressSanitizer + UBSan (run as programs: no preloading of anything)."""
    d = tmp_path_factory.mktemp("splitk_rule")
    exes = []
    for name, extra in (("splitk_rule_check", []), ("splitk_rule_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / name
        subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *extra, f"-I{CSRC}", str(HERE / "splitk_rule_check.cpp"), "-o", str(exe)])
        exes.append(exe)
    return exes


def test_split_tree_grid_offsets_and_bank_slots_plain_and_under_sanitizers(rule_checks):
    for exe in rule_checks:
        run = subprocess.run([str(exe)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.rstrip().endswith("splitk rule ok"), run.stdout[-3000:] + run.stderr[-3000:]


def test_the_kernel_is_written_with_the_rule():
    """Every LDS address, the ranges and the grid map of the kernel go through the header's functions, and the file is built."""
    assert CSRC / "kernels_splitk.hip" in HIP_SOURCES
    k = (CSRC / "kernels_splitk.hip").read_text()
    for name in ("splitk_ways", "splitk_bound", "splitk_grid", "splitk_logical", "splitk_board", "splitk_cout_block", "splitk_image", "splitk_lds_bytes",
                 "splitk_piece_row", "splitk_piece_dst", "splitk_tap_read", "splitk_frag_offset", "splitk_x", "splitk_item_pixel", "splitk_item_cg",
                 "SK_DZERO", "SK_ZAREA", "SK_MAX_FILTERS"):
        assert re.search(rf"\b{name}\b", k), name
    # workgroups are independent: LDS barriers only -- no atomics on the sums, no polling of memory another workgroup writes
    code = re.sub(r"//[^\n]*", "", k)
    assert "atomic" not in code and "__threadfence" not in code and "sleep" not in code
    assert set(re.findall(r'asm volatile\("([^"]*)"', code)) == {r"s_waitcnt lgkmcnt(0)\n\ts_barrier"}  # the only hand-written instructions


def test_the_form_number_and_the_unchanged_config_layout():
    from cattus_amd.evaluator import TOWER_FORMS, EvalConfig

    assert TOWER_FORMS["direct_splitk"] == 4
    assert TOWER_FORMS == {"auto": 0, "direct": 1, "winograd": 2, "winograd_f4": 3, "direct_splitk": 4}
    header = (ROOT / "include" / "cattus_hip.h").read_text()
    assert re.search(r"CATTUS_TOWER_DIRECT_SPLITK = 4,", header)
    struct = header[header.index("typedef struct cattus_eval_config {"):header.index("} cattus_eval_config;")]
    fields = re.findall(r"^\s*(u?int32_t) (\w+);", struct, re.M)
    assert [name for _, name in fields] == [name for name, _ in EvalConfig._fields_]
    assert [name for name, _ in EvalConfig._fields_] == ["struct_size", "device", "max_batch", "plane_words", "dtype", "flush_us", "tower_form", "tail_leaves"]
    assert ctypes.sizeof(EvalConfig) == 32 and EvalConfig.tower_form.offset == 24 and EvalConfig.tail_leaves.offset == 28
