"""The stem's input-channel padding (cattus_amd/csrc/weight_layout.h: stem_cin_pad, stem_is_fused) without a GPU.

Every dtype takes a network of up to 128 plane words per leaf.  Up to 32 planes the stem conv expands the bitboard planes itself; beyond
that (or under CATTUS_FUSED_STEM=0) pack_planes_nhwc_kernel writes them as tower rows first and the stem runs as an ordinary layer.  The
f16x2 kernels without STEM request two 32-channel chunks up front, so that stem's channels are then padded to a multiple of 64, not 32.
tests/stem_padding_check.cpp checks

  * the rule for every (dtype, planes in {1, 18, 32, 33, 64, 65, 119, 128}, packed separately or not): f16x2 gives 32 only when fused
    (at most 32 planes, no switch), else the next multiple of 64; f16 / bf16 the next multiple of 64; f32 the next multiple of 32;
  * the f16x2 stem layouts at cin = 40 and cin = 18 with cin_pad = 64, in fragment order (split_frag_index) and in row order: every real
    weight's (hi, lo) pair sits where the index functions say, every padded channel is zero in both halves, nothing else is set, and the
    per-output-channel scales (and the [biases | inverse scales] buffer) equal those of the same weights under another padding -- zeros
    do not move them, which is what lets the packed stem give the fused stem's bits (tests/test_many_planes_gpu.py).

The header uses _Float16, so the program is built with the clang++ that hipcc drives as its host compiler."""

import subprocess
from pathlib import Path

from cattus_amd.build import CSRC

from test_weight_layout import host_compiler

HERE = Path(__file__).resolve().parent


def test_stem_padding_rule_and_the_f16x2_stem_layouts_it_asks_for(tmp_path):
    exe = tmp_path / "stem_padding_check"
    # -ffp-contract=off: as the library itself is built (cattus_amd/build.py)
    subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", f"-I{CSRC}", str(HERE / "stem_padding_check.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "stem padding ok" in run.stdout, run.stdout[-4000:] + run.stderr[-2000:]
