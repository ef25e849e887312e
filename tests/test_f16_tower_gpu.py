"""The single-term f16 tower (dtype f16) against the float64 network, on every conv tile its launch code can pick.

dtype f16 runs every 3x3 conv of the tower on conv3x3_mfma_v2_kernel<_Float16, R, BIG, STEM, CB, PBW> (no resident tower, no
Winograd form), with the tile chosen PER LAUNCH from the call's own padded batch nb (launch_conv3x3_mfma, kernels.hip):

    full_grid = (nb * slots / 256) * (cout_pad / 64)
    CB  = 2 if full_grid > 128 else 1                        (CATTUS_CONV_CB forces it)
    PBW = 1 if CB == 1 and 2 * full_grid <= 128 else 2       (CATTUS_CONV_PBW forces it; CB = 2 always has PBW = 2)

and the template flags from the layer: STEM = the stem (planes expanded in the kernel, R = false), R = the second conv of a
residual block (skip input), neither = the first conv of a block; BIG = 128-slot boards (above 8x8).  Every network below with
at least one residual block runs all three layer kinds, so a shape and a tile cover three instances.  Which test runs which:

    BIG = false (64 slots)
      CB=1 PBW=1  chess 3x256 n=40, ttt 2x64 n=7, hex7 6x64 n=128 (default); every 64-slot shape under CB=1 PBW=1;
                  a single leaf of chess 3x256 / 20x256 (test_single_leaf_..., the full-size test's 37-leaf sub-batch)
      CB=1 PBW=2  chess 3x256 n=70, hex5 4x96 n=77 (default); every 64-slot shape under CB=1 PBW=2;
                  the full-size test's 100-leaf sub-batch
      CB=2 PBW=2  chess 3x256 n=256, chess 20x256 n=256, chess 40x384 n=512, the range test at 520 leaves (default);
                  every 64-slot shape under CB=2
    BIG = true (128 slots)
      CB=1 PBW=1  hex11 2x128 n=21 (default); hex9 2x128 under CB=1 PBW=1
      CB=1 PBW=2  hex9 2x128 n=100 (default); hex11 2x128 under CB=1 PBW=2
      CB=2 PBW=2  hex11 2x128 and hex9 2x128 under CB=2

Bars: all tiles of a shape give the same bits; that result is within F16_VS_F64 of the float64 network (tests/helpers.py
forward_f64, built from the raw tensors, not from the blob); the f16 error is at most a quarter of the bf16 tower's error on the
same leaves (the structural ceiling: 11 against 8 significant bits), and the bf16 outputs FAIL the f16 bound (the bound tells the
two apart): helpers.check_f16_against_f64.  The full-size networks (chess 20x256 at 256 leaves, 40x384 at 512) are held to the
same bars in test_hip_parity.py.
"""

import numpy as np
import pytest

from cattus_amd.evaluator import HipEvaluator
from cattus_amd.weights import CHESS, NetDesc, hex_game, pack_tensors, seeded_tensors

from helpers import check_f16_against_f64, forward_f64

pytestmark = pytest.mark.gpu

TTT = dict(planes=3, board=3, moves=9)

# max |dlogit|, max |dvalue| of the f16 tower against forward_f64, per shape: 2x the error measured on an MI355X (every leaf of
# the test; all tiles give the same bits).  Measured f16 | bf16 on the same leaves:
#   chess3x256   3.34e-4 7.72e-5 | 3.90e-3 9.63e-4  (n = 40, 70, 256: the largest of the three)
#   hex11_2x128  2.94e-4 7.25e-5 | 3.90e-3 7.61e-4
#   hex9_2x128   3.55e-4 7.32e-5 | 4.69e-3 8.13e-4
#   hex5_4x96    3.39e-4 1.33e-4 | 4.24e-3 1.20e-3
#   ttt2x64      1.96e-4 2.53e-5 | 1.83e-3 1.99e-4
#   hex7_6x64    5.86e-4 9.19e-5 | 5.09e-3 9.92e-4
F16_VS_F64 = {
    "chess3x256": (6.7e-4, 1.6e-4),
    "hex11_2x128": (5.9e-4, 1.5e-4),
    "hex9_2x128": (7.1e-4, 1.5e-4),
    "hex5_4x96": (6.8e-4, 2.7e-4),
    "ttt2x64": (4.0e-4, 5.1e-5),
    "hex7_6x64": (1.2e-3, 1.9e-4),
}
# the range test at stem BN scale 200 (logits in the tens): max |dlogit| over max |logit|, and max |dvalue|, against forward_f64;
# 2x the measured 4.11e-4 / 1.09e-2 (520 leaves, CB=2 by itself; 16 leaves with CB=2 forced: 3.7e-4 / 2.1e-3)
F16_RANGE_REL_POLICY, F16_RANGE_VALUE = 8.3e-4, 2.2e-2

SHAPES = [
    # id, game preset, blocks, filters, heads, plane words, n (default tile)
    ("chess3x256", CHESS, 3, 256, 8, 1, 40),        # 64 slots, 4 cout slabs: CB=1 PBW=1
    ("chess3x256", CHESS, 3, 256, 8, 1, 70),        # CB=1 PBW=2
    ("chess3x256", CHESS, 3, 256, 8, 1, 256),       # CB=2: the tile of the timed batch
    ("hex11_2x128", hex_game(11), 2, 128, 16, 2, 21),  # 128 slots, 2 cout slabs: CB=1 PBW=1
    ("hex9_2x128", hex_game(9), 2, 128, 4, 2, 100),    # 128 slots: CB=1 PBW=2
    ("hex5_4x96", hex_game(5), 4, 96, 8, 2, 77),       # 96 filters padded to 128 (two cout slabs, zero channels): CB=1 PBW=2
    ("ttt2x64", TTT, 2, 64, 8, 1, 7),                  # 3x3 board in 64 slots: CB=1 PBW=1
    ("hex7_6x64", hex_game(7), 6, 64, 16, 2, 128),     # BASELINE config 2's shape: CB=1 PBW=1
]
# every forced tile, and the default (CB=2 ignores PBW: both spellings must give the same bits)
TILE_SWITCHES = [{}, {"CATTUS_CONV_CB": "1", "CATTUS_CONV_PBW": "1"}, {"CATTUS_CONV_CB": "1", "CATTUS_CONV_PBW": "2"},
                 {"CATTUS_CONV_CB": "2", "CATTUS_CONV_PBW": "1"}, {"CATTUS_CONV_CB": "2", "CATTUS_CONV_PBW": "2"}]


def random_planes(d: NetDesc, words: int, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    hw = d.board * d.board
    planes = np.zeros((n, d.planes, words), dtype=np.uint64)
    bits = rng.integers(0, 2, size=(n, d.planes, hw), dtype=np.uint64)
    for i in range(hw):
        planes[:, :, i >> 6] |= bits[:, :, i] << np.uint64(i & 63)
    return planes


@pytest.mark.parametrize("name,game,blocks,filters,heads,words,n", SHAPES)
def test_every_tile_gives_the_same_bits_within_the_f64_bound(name, game, blocks, filters, heads, words, n):
    d = NetDesc(**game, blocks=blocks, filters=filters, vhc=heads, phc=heads)
    tensors = seeded_tensors(d, 31)
    blob = pack_tensors(d, tensors)
    planes = random_planes(d, words, n, 3)
    outs = []
    for sw in TILE_SWITCHES:
        with HipEvaluator(blob, batch_size=n, plane_words=words, dtype="f16", switches=sw) as ev:
            outs.append(ev.eval(planes))
            assert ev.stats()["saturated"] == 0
    for sw, (p, v) in zip(TILE_SWITCHES[1:], outs[1:]):
        assert (p == outs[0][0]).all() and (v == outs[0][1]).all(), sw
    with HipEvaluator(blob, batch_size=n, plane_words=words, dtype="bf16", switches={}) as ev:
        bf = ev.eval(planes)
    check_f16_against_f64(f"{name} n={n}", F16_VS_F64[name], outs[0], bf, forward_f64(d, tensors, planes))


def test_single_leaf_equals_the_same_leaf_in_a_full_batch():
    """A leaf alone runs the small-grid tile (CB=1 PBW=1), inside a 256-leaf batch the CB=2 tile: same bits, in any slot."""
    d = NetDesc(**CHESS, blocks=3, filters=256, vhc=8, phc=8)
    blob = pack_tensors(d, seeded_tensors(d, 37))
    planes = random_planes(d, 1, 256, 4)
    with HipEvaluator(blob, batch_size=256, plane_words=1, dtype="f16", switches={}) as ev:
        p_all, v_all = ev.eval(planes)
        for i in (0, 1, 99, 254, 255):
            p1, v1 = ev.eval(planes[i : i + 1])
            assert (p1[0] == p_all[i]).all() and v1[0] == v_all[i], i
        p_rev, v_rev = ev.eval(planes[::-1].copy())
        assert (p_rev[::-1] == p_all).all() and (v_rev[::-1] == v_all).all()


@pytest.mark.parametrize("switches,n", [({"CATTUS_CONV_CB": "2"}, 16), ({}, 520)])
def test_f16_range_on_the_large_tile(switches, n):
    """The saturation contract of test_f16x2_range_large_batchnorm_scales for the single-term f16 tower on the CB=2 tile, forced and
    picked by itself (520 leaves of a 64-filter net: a grid of 130 > 128 workgroups).  A stem BatchNorm scale of 200 puts the
    residual stream in the hundreds: nothing saturates and the result tracks the float64 network; one of 1e5 leaves the f16
    range: the epilogue clamps at 65504 and counts it (sticky over the evaluator's life), and every output stays finite."""
    d = NetDesc(**CHESS, blocks=2, filters=64, vhc=8, phc=8)
    planes = random_planes(d, 1, n, 6)
    for scale, saturates in ((200.0, False), (1e5, True)):
        t = seeded_tensors(d, 6)
        t["_conv1._bn.weight"] = t["_conv1._bn.weight"] * np.float32(scale)
        t["_residual_blocks.0._conv1.weight"] = t["_residual_blocks.0._conv1.weight"] * np.float32(1e-3)
        blob = pack_tensors(d, t)
        with HipEvaluator(blob, batch_size=n, plane_words=1, dtype="f16", switches=switches) as ev:
            assert ev.stats()["saturated"] == 0
            p, v = ev.eval(planes)
            sat = ev.stats()["saturated"]
            p2, v2 = ev.eval(planes)
            assert ev.stats()["saturated"] == 2 * sat  # sticky: it accumulates
            assert (p2 == p).all() and (v2 == v).all()
        assert (sat > 0) == saturates, (scale, sat)
        assert np.isfinite(p).all() and np.isfinite(v).all()
        if not saturates:
            p64, v64 = forward_f64(d, t, planes)
            assert np.abs(p64).max() > 20  # the scale did reach the logits
            rel_p = float(np.abs(p - p64).max() / np.abs(p64).max())
            dv = float(np.abs(v - v64).max())
            print("f16 range, scale %g, %d leaves %s: max |dlogit| / max |logit| %.3g, max |dvalue| %.3g" % (scale, n, switches, rel_p, dv))
            assert rel_p <= F16_RANGE_REL_POLICY and dv <= F16_RANGE_VALUE, (rel_p, dv)

