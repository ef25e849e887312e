"""The f32-operand Winograd kernel's geometry, transforms and arithmetic order without a GPU: cattus_amd/csrc/wino_f32_rule.h, which
conv3x3_wino_f32_kernel (dtype f32w) is written with.

tests/wino_f32_rule_check.cpp is a stand-alone program around the header.  It is built with the host compiler twice -- plain, and with
-fsanitize=address,undefined -- and both are run as programs.  In the program: the grid map is a bijection onto (board pair, cout
group) for one and for two cout blocks per workgroup, 128 / 192 / 256 / 384 filters and 2 .. 256 padded boards (grids that are and are
not multiples of 8), and the rule that chooses between one and two blocks; the transform's threads cover every (tile, channel) of a
step once; V-image, chunk and exchange offsets stay inside their areas and on bytes of their own, the exchange over V image 0 alone;
the LDS total fits 160 KiB; the lane groups of every 16-byte V read and exchange access fall on 16 different bank slots, and the 8-byte
V writes and patch reads of a half wave on 32 different bank pairs; the U index is a bijection onto the buffer, agrees with the kernel's
stage offset and with the builder; the chain visits every channel once in Mfma<float>::mac's order; the header's B^T / G / A^T orders
reproduce the matrices, and together the 3x3 correlation, against float64 on random data.

tests/wino_f32_layer_ref.cpp restates one whole layer with std::fmaf in the header's order (the program tests/test_f32w_gpu.py holds the
kernel to bit for bit); here it is held to a float64 direct convolution on a random 128 -> 128 layer by a bound derived from the operand
sizes.

Here also: the kernel source calls the header's functions, the new files are part of the build, and the dtype's number in the header and
in the Python binding."""

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from cattus_amd.build import CSRC, HIP_DEPS, HIP_SOURCES

from test_weight_layout import host_compiler

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent


def build_layer_ref(directory, extra=()):
    """tests/wino_f32_layer_ref.cpp as a program (tests/test_f32w_gpu.py builds it too)."""
    exe = Path(directory) / "wino_f32_layer_ref"
    subprocess.check_call([host_compiler(), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *extra, f"-I{CSRC}", str(HERE / "wino_f32_layer_ref.cpp"), "-o", str(exe)])
    return exe


def run_layer_ref(exe, directory, rows, w, b, skip=None):
    """rows [boards * 64, cin], w [9, cout, cin], b [cout], skip [boards * 64, cout] or None -> the layer's output rows [boards * 64, cout]."""
    d = Path(directory)
    boards, cin, cout = rows.shape[0] // 64, rows.shape[1], w.shape[1]
    assert rows.shape == (boards * 64, cin) and w.shape == (9, cout, cin) and b.shape == (cout,)
    for name, a in (("in", rows), ("w", w), ("b", b), ("skip", skip)):
        if a is not None:
            np.ascontiguousarray(a, dtype=np.float32).tofile(d / f"{name}.f32")
    run = subprocess.run([str(exe), str(boards), str(cin), str(cout), str(d / "in.f32"), str(d / "w.f32"), str(d / "b.f32"), str(d / "skip.f32") if skip is not None else "-", str(d / "out.f32")],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    return np.fromfile(d / "out.f32", dtype=np.float32).reshape(boards * 64, cout)


@pytest.fixture(scope="module")
def rule_checks(tmp_path_factory):
    """The stand-alone program, plain and under AddressSanitizer + UBSan (run as programs: no preloading of anything)."""
    d = tmp_path_factory.mktemp("wino_f32_rule")
    exes = []
    for name, extra in (("wino_f32_rule_check", []), ("wino_f32_rule_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / name
        subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *extra, f"-I{CSRC}", str(HERE / "wino_f32_rule_check.cpp"), "-o", str(exe)])
        exes.append(exe)
    return exes


def test_grid_items_offsets_bank_slots_u_index_chain_and_transforms_plain_and_under_sanitizers(rule_checks):
    for exe in rule_checks:
        run = subprocess.run([str(exe)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.rstrip().endswith("wino_f32 rule ok"), run.stdout[-3000:] + run.stderr[-3000:]


def test_the_layer_restatement_is_the_convolution(tmp_path):
    """A random 128 -> 128 layer on two boards, with and without a skip, against the float64 direct convolution.

    The bound, from the operand sizes (eps = 2^-24, the unit roundoff of f32; D, W the largest |input| and |weight|; n = 128 channels):
    |U| <= 2.25 W (G's largest absolute row sum is 1.5, twice), rounded once: relative eps.  |V| <= 4 D (B^T's is 2, twice), made with one
    rounded add per pass: |dV| <= 8 eps D = 2 eps (4 D).  A chain of n fmaf errs by at most n eps times the sum of its |products|, <=
    n (2.25 W)(4 D); the operands' own errors add (1 + 2) eps times the same sum.  So |dM| <= (n + 3) eps n 9 W D.  Y is a signed sum of 9
    M's in 4 rounded adds of partial sums <= 9 |M|: |dY| <= 9 |dM| + 4 eps 9 n 9 W D = 81 n (n + 7) eps W D, and the bias add and the
    skip add round once more each, on values <= 81 n W D + |b| + |skip|: at most 2 eps of that, far below one more unit of n.  In all
    81 n (n + 8) eps W D = 0.084 W D for n = 128: every term is a worst case, a rounding error of this restatement is ~1e-5, and a
    wrong channel, tap or sign is an error of the outputs' own size, ~10."""
    rng = np.random.default_rng(17)
    boards, n = 2, 128
    rows = rng.uniform(-1, 1, (boards * 64, n)).astype(np.float32)
    w = rng.uniform(-1, 1, (9, n, n)).astype(np.float32)
    b = rng.uniform(-1, 1, n).astype(np.float32)
    skip = rng.uniform(-1, 1, (boards * 64, n)).astype(np.float32)
    x = np.zeros((boards, 10, 10, n))
    x[:, 1:9, 1:9] = rows.astype(np.float64).reshape(boards, 8, 8, n)
    conv = np.zeros((boards, 8, 8, n))
    for ky in range(3):
        for kx in range(3):
            conv += x[:, ky:ky + 8, kx:kx + 8] @ w[ky * 3 + kx].astype(np.float64).T
    conv = conv.reshape(boards * 64, n) + b.astype(np.float64)
    D, W = float(np.abs(rows).max()), float(np.abs(w).max())
    bound = 81 * n * (n + 8) * 2.0**-24 * W * D
    exe = build_layer_ref(tmp_path)
    for sk in (None, skip):
        got = run_layer_ref(exe, tmp_path, rows, w, b, sk)
        want = np.maximum(conv + (0 if sk is None else sk.astype(np.float64)), 0)
        err = float(np.abs(got - want).max())
        print("layer restatement vs float64, skip %s: max |d| %.3g (bound %.3g), outputs up to %.3g" % (sk is not None, err, bound, np.abs(want).max()))
        assert got.dtype == np.float32 and (got >= 0).all() and err <= bound
        assert np.abs(want).max() > 50 * bound  # the bound is far below the outputs' own size


def test_the_kernel_is_written_with_the_rule():
    """Every LDS address, every index, both transforms and the epilogue of the kernel go through the header's functions."""
    k = (CSRC / "kernels_wino_f32.hip").read_text()
    for name in ("wf32_ncb", "wf32_grid", "wf32_logical", "wf32_pair", "wf32_cout_group", "wf32_u_stage", "wf32_item_tile", "wf32_item_chp", "wf32_v_image",
                 "wf32_v_write", "wf32_v_read", "wf32_chunk_buffer", "wf32_piece_row", "wf32_piece_dst", "wf32_patch_read", "wf32_z", "wf32_out_pixel",
                 "wf32_out_row", "wf32_out_tile", "wf32_bt", "wf32_at", "wf32_finish", "WF32_LDS_TOTAL", "WF32_VF", "WF32_VGROUP", "WF32_DHALF", "WF32_UD", "WF32_STEP"):
        assert re.search(rf"\b{name}\b", k), name
    assert re.search(r"Mfma<float>::mac\(", k)  # the chain is the exact tower's
    # the builder writes U through the index the header's stage offset is checked against
    assert re.search(r"\bwino_f32_frag_index\b", (CSRC / "weight_layout.h").read_text())
    assert re.search(r"\bwino_u_f32\b", (CSRC / "evaluator.hip").read_text())


def test_the_kernel_and_its_rule_are_part_of_the_build():
    assert CSRC / "kernels_wino_f32.hip" in HIP_SOURCES
    assert CSRC / "wino_f32_rule.h" in HIP_DEPS


def test_the_dtype_has_one_number_in_the_header_and_in_the_binding():
    from cattus_amd import evaluator

    assert evaluator.DTYPE_F32W == 5 and evaluator._DTYPES_WINO_F32 == {"f32w": 5}
    assert evaluator._DTYPES == {"f32": 0, "bf16": 1, "f16x2": 2, "f16": 3, "f16w": 4}  # the five old entries, exactly
    header = (ROOT / "include" / "cattus_hip.h").read_text()
    assert re.search(r"^\s*CATTUS_DTYPE_F32W = 5,", header, re.M)
