"""Which tower an evaluator runs, pinned for a matrix of small evaluators that reaches every plan kind of
cattus_amd/csrc/evaluator.hip (Simple, Generic, PerLayer, Resident64, Resident64Split, Wino16, Wino4 in one launch and per layer) and
every fallback between them: dtype x filters x board x blocks x max_batch under tower_form AUTO, the three forms for f16x2, the
diagnostic switches one at a time, wide heads and a SimpleTwoHeadedModel blob.  EXPECTED is what cattus_hip_tower_kernel() reported
for each case before the plan was resolved in one place ("refused -2": cattus_hip_create returned CATTUS_E_UNSUPPORTED); a case
that is missing from the table fails.  Every evaluator also runs one batch of four leaves."""

import functools

import numpy as np
import pytest

from cattus_amd.evaluator import CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, NetDesc, hex_game, seeded_blob, simple_desc

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "bf16", "f16", "f16x2")
FILTERS = (16, 64, 128, 192)
BOARDS = (8, 9)
BLOCKS = (1, 0)
BATCHES = (4, 128, 132)
RESIDENT = ("tower64_lds_kernel", "tower64_split_kernel")


def case_id(dtype, filters, board, blocks, batch, form="auto", switch=""):
    return f"{dtype}-f{filters}-s{board}-b{blocks}-n{batch}-{form}" + (f"-{switch}" if switch else "")


def _groups():
    g = {}
    for dt in DTYPES:
        g[f"auto-{dt}"] = [(dt, f, s, b, n, "auto", "") for f in FILTERS for s in BOARDS for b in BLOCKS for n in BATCHES]
    g["forms-f16x2"] = [("f16x2", f, s, b, n, form, "") for form in ("direct", "winograd") for f in FILTERS for s in BOARDS for b in BLOCKS for n in BATCHES]
    g["forms-others"] = [(dt, 128, 8, 1, 132, form, "") for dt in ("f32", "bf16", "f16") for form in ("direct", "winograd")]
    g["CATTUS_TOWER64"] = [(dt, f, s, 1, 4, "auto", "CATTUS_TOWER64=0") for dt in ("bf16", "f16x2") for f in (16, 64, 128) for s in BOARDS]
    g["CATTUS_SPLIT_W"] = [("f16x2", f, 8, 1, n, form, "CATTUS_SPLIT_W=0") for f in (16, 64, 128) for n in (4, 132) for form in ("auto", "winograd") if f == 128 or form == "auto"]
    for sw in ("CATTUS_WINO_KERNEL=k16", "CATTUS_WINO_KERNEL=k4"):
        g[sw] = [("f16x2", f, s, b, n, form, sw) for f in (64, 128, 192) for s in BOARDS for b in BLOCKS for n in (4, 132) for form in ("auto", "winograd")
                 if (s == 8 and b == 1) or (f == 128 and n == 132)]
    for sw in ("CATTUS_WINO_PERSIST=0", "CATTUS_WINO_INPLACE=0"):
        g[sw] = [("f16x2", f, 8, 1, n, form, sw) for f in (64, 128, 192) for n in (4, 132) for form in ("auto", "winograd") if f != 64 or form == "auto"]
    g["CATTUS_FORCE_GENERIC"] = [(dt, f, s, 1, 4, "auto", "CATTUS_FORCE_GENERIC=1") for dt in ("f32", "bf16", "f16x2") for f in (16, 128) for s in BOARDS]
    return g


GROUPS = _groups()


@functools.lru_cache(maxsize=None)
def blob_of(filters, board, blocks, vhc=8):
    game = CHESS if board == 8 else hex_game(board)
    return seeded_blob(NetDesc(**game, blocks=blocks, filters=filters, vhc=vhc, phc=vhc), 40 + filters + board + blocks)


def fixed_planes(n, planes, board, words, seed=5):
    """n leaves of random bits on the board's squares (not positions of any game: the tower does not care)."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 2**63, size=(n, planes, words), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, planes, words), dtype=np.uint64)
    hw = board * board
    for w in range(words):
        bits = min(64, max(0, hw - 64 * w))
        p[:, :, w] &= np.uint64((1 << bits) - 1)
    return p


def run_case(blob, words, dtype, batch, form, switch, leaves=(4,)):
    """(kernel name or 'refused <status>', launches per forward or None, [(policy, value) per entry of leaves])."""
    switches = dict([switch.split("=")]) if switch else {}
    try:
        ev = HipEvaluator(blob, batch_size=batch, plane_words=words, dtype=dtype, tower_form=form, switches=switches)
    except CattusHipError as err:
        return f"refused {err.status}", None, []
    with ev:
        d = ev.desc
        outs = [ev.eval(fixed_planes(n, d.planes, d.board, words)) for n in leaves if n <= batch]
        try:
            launches = ev.time_tower(min(4, batch), 1)[1]
        except CattusHipError as err:
            launches = f"refused {err.status}"
        return ev.tower_kernel(), launches, outs


def special_cases():
    """(id, blob, plane_words, dtype, max_batch): heads wider than one 32-row tile, and SimpleTwoHeadedModel blobs."""
    wide = seeded_blob(NetDesc(**hex_game(5), blocks=1, filters=32, vhc=24, phc=24), 4)
    simple = seeded_blob(simple_desc(**hex_game(5)), 3)
    return [("wide-f32", wide, 2, "f32", 4), ("wide-bf16", wide, 2, "bf16", 4), ("wide-f16x2", wide, 2, "f16x2", 132),
            ("simple-f32", simple, 2, "f32", 4), ("simple-f16x2", simple, 2, "f16x2", 132)]


EXPECTED = {
    "f32-f16-s8-b1-n4-auto-CATTUS_FORCE_GENERIC=1": "conv3x3_generic_kernel", "f32-f16-s9-b1-n4-auto-CATTUS_FORCE_GENERIC=1": "conv3x3_generic_kernel",
    "f32-f128-s8-b1-n4-auto-CATTUS_FORCE_GENERIC=1": "conv3x3_generic_kernel", "f32-f128-s9-b1-n4-auto-CATTUS_FORCE_GENERIC=1": "conv3x3_generic_kernel",
    "bf16-f16-s8-b1-n4-auto-CATTUS_FORCE_GENERIC=1": "refused -2", "bf16-f16-s9-b1-n4-auto-CATTUS_FORCE_GENERIC=1": "refused -2",
    "bf16-f128-s8-b1-n4-auto-CATTUS_FORCE_GENERIC=1": "refused -2", "bf16-f128-s9-b1-n4-auto-CATTUS_FORCE_GENERIC=1": "refused -2",
    "f16x2-f16-s8-b1-n4-auto-CATTUS_FORCE_GENERIC=1": "refused -2", "f16x2-f16-s9-b1-n4-auto-CATTUS_FORCE_GENERIC=1": "refused -2",
    "f16x2-f128-s8-b1-n4-auto-CATTUS_FORCE_GENERIC=1": "refused -2", "f16x2-f128-s9-b1-n4-auto-CATTUS_FORCE_GENERIC=1": "refused -2",
    "f16x2-f16-s8-b1-n4-auto-CATTUS_SPLIT_W=0": "conv3x3_split_kernel", "f16x2-f16-s8-b1-n132-auto-CATTUS_SPLIT_W=0": "conv3x3_split_kernel",
    "f16x2-f64-s8-b1-n4-auto-CATTUS_SPLIT_W=0": "conv3x3_split_kernel", "f16x2-f64-s8-b1-n132-auto-CATTUS_SPLIT_W=0": "conv3x3_split_kernel",
    "f16x2-f128-s8-b1-n4-auto-CATTUS_SPLIT_W=0": "conv3x3_split_kernel", "f16x2-f128-s8-b1-n4-winograd-CATTUS_SPLIT_W=0": "tower_wino4_kernel",
    "f16x2-f128-s8-b1-n132-auto-CATTUS_SPLIT_W=0": "tower_wino4_kernel", "f16x2-f128-s8-b1-n132-winograd-CATTUS_SPLIT_W=0": "tower_wino4_kernel",
    "bf16-f16-s8-b1-n4-auto-CATTUS_TOWER64=0": "conv3x3_mfma_v2_kernel", "bf16-f16-s9-b1-n4-auto-CATTUS_TOWER64=0": "conv3x3_mfma_v2_kernel",
    "bf16-f64-s8-b1-n4-auto-CATTUS_TOWER64=0": "conv3x3_mfma_v2_kernel", "bf16-f64-s9-b1-n4-auto-CATTUS_TOWER64=0": "conv3x3_mfma_v2_kernel",
    "bf16-f128-s8-b1-n4-auto-CATTUS_TOWER64=0": "conv3x3_mfma_v2_kernel", "bf16-f128-s9-b1-n4-auto-CATTUS_TOWER64=0": "conv3x3_mfma_v2_kernel",
    "f16x2-f16-s8-b1-n4-auto-CATTUS_TOWER64=0": "conv3x3_splitw_kernel", "f16x2-f16-s9-b1-n4-auto-CATTUS_TOWER64=0": "conv3x3_splitw_kernel",
    "f16x2-f64-s8-b1-n4-auto-CATTUS_TOWER64=0": "conv3x3_splitw_kernel", "f16x2-f64-s9-b1-n4-auto-CATTUS_TOWER64=0": "conv3x3_splitw_kernel",
    "f16x2-f128-s8-b1-n4-auto-CATTUS_TOWER64=0": "conv3x3_splitw_kernel", "f16x2-f128-s9-b1-n4-auto-CATTUS_TOWER64=0": "conv3x3_splitw_kernel",
    "f16x2-f64-s8-b1-n4-auto-CATTUS_WINO_INPLACE=0": "tower64_split_kernel", "f16x2-f64-s8-b1-n132-auto-CATTUS_WINO_INPLACE=0": "tower64_split_kernel",
    "f16x2-f128-s8-b1-n4-auto-CATTUS_WINO_INPLACE=0": "conv3x3_splitw_kernel",
    "f16x2-f128-s8-b1-n4-winograd-CATTUS_WINO_INPLACE=0": "conv3x3_wino4_kernel",
    "f16x2-f128-s8-b1-n132-auto-CATTUS_WINO_INPLACE=0": "conv3x3_wino4_kernel",
    "f16x2-f128-s8-b1-n132-winograd-CATTUS_WINO_INPLACE=0": "conv3x3_wino4_kernel",
    "f16x2-f192-s8-b1-n4-auto-CATTUS_WINO_INPLACE=0": "conv3x3_splitw_kernel",
    "f16x2-f192-s8-b1-n4-winograd-CATTUS_WINO_INPLACE=0": "conv3x3_wino4_kernel",
    "f16x2-f192-s8-b1-n132-auto-CATTUS_WINO_INPLACE=0": "conv3x3_wino4_kernel",
    "f16x2-f192-s8-b1-n132-winograd-CATTUS_WINO_INPLACE=0": "conv3x3_wino4_kernel",
    "f16x2-f64-s8-b1-n4-auto-CATTUS_WINO_KERNEL=k16": "tower64_split_kernel", "f16x2-f64-s8-b1-n4-winograd-CATTUS_WINO_KERNEL=k16": "refused -2",
    "f16x2-f64-s8-b1-n132-auto-CATTUS_WINO_KERNEL=k16": "tower64_split_kernel", "f16x2-f64-s8-b1-n132-winograd-CATTUS_WINO_KERNEL=k16": "refused -2",
    "f16x2-f128-s8-b1-n4-auto-CATTUS_WINO_KERNEL=k16": "conv3x3_splitw_kernel",
    "f16x2-f128-s8-b1-n4-winograd-CATTUS_WINO_KERNEL=k16": "conv3x3_wino_kernel",
    "f16x2-f128-s8-b1-n132-auto-CATTUS_WINO_KERNEL=k16": "conv3x3_wino_kernel",
    "f16x2-f128-s8-b1-n132-winograd-CATTUS_WINO_KERNEL=k16": "conv3x3_wino_kernel",
    "f16x2-f128-s8-b0-n132-auto-CATTUS_WINO_KERNEL=k16": "conv3x3_splitw_kernel", "f16x2-f128-s8-b0-n132-winograd-CATTUS_WINO_KERNEL=k16": "refused -2",
    "f16x2-f128-s9-b1-n132-auto-CATTUS_WINO_KERNEL=k16": "conv3x3_splitw_kernel", "f16x2-f128-s9-b1-n132-winograd-CATTUS_WINO_KERNEL=k16": "refused -2",
    "f16x2-f128-s9-b0-n132-auto-CATTUS_WINO_KERNEL=k16": "conv3x3_splitw_kernel", "f16x2-f128-s9-b0-n132-winograd-CATTUS_WINO_KERNEL=k16": "refused -2",
    "f16x2-f192-s8-b1-n4-auto-CATTUS_WINO_KERNEL=k16": "conv3x3_splitw_kernel", "f16x2-f192-s8-b1-n4-winograd-CATTUS_WINO_KERNEL=k16": "refused -2",
    "f16x2-f192-s8-b1-n132-auto-CATTUS_WINO_KERNEL=k16": "conv3x3_splitw_kernel", "f16x2-f192-s8-b1-n132-winograd-CATTUS_WINO_KERNEL=k16": "refused -2",
    "f16x2-f64-s8-b1-n4-auto-CATTUS_WINO_KERNEL=k4": "tower64_split_kernel", "f16x2-f64-s8-b1-n4-winograd-CATTUS_WINO_KERNEL=k4": "refused -2",
    "f16x2-f64-s8-b1-n132-auto-CATTUS_WINO_KERNEL=k4": "tower64_split_kernel", "f16x2-f64-s8-b1-n132-winograd-CATTUS_WINO_KERNEL=k4": "refused -2",
    "f16x2-f128-s8-b1-n4-auto-CATTUS_WINO_KERNEL=k4": "conv3x3_splitw_kernel",
    "f16x2-f128-s8-b1-n4-winograd-CATTUS_WINO_KERNEL=k4": "tower_wino4_kernel", "f16x2-f128-s8-b1-n132-auto-CATTUS_WINO_KERNEL=k4": "tower_wino4_kernel",
    "f16x2-f128-s8-b1-n132-winograd-CATTUS_WINO_KERNEL=k4": "tower_wino4_kernel",
    "f16x2-f128-s8-b0-n132-auto-CATTUS_WINO_KERNEL=k4": "conv3x3_splitw_kernel", "f16x2-f128-s8-b0-n132-winograd-CATTUS_WINO_KERNEL=k4": "refused -2",
    "f16x2-f128-s9-b1-n132-auto-CATTUS_WINO_KERNEL=k4": "conv3x3_splitw_kernel", "f16x2-f128-s9-b1-n132-winograd-CATTUS_WINO_KERNEL=k4": "refused -2",
    "f16x2-f128-s9-b0-n132-auto-CATTUS_WINO_KERNEL=k4": "conv3x3_splitw_kernel", "f16x2-f128-s9-b0-n132-winograd-CATTUS_WINO_KERNEL=k4": "refused -2",
    "f16x2-f192-s8-b1-n4-auto-CATTUS_WINO_KERNEL=k4": "conv3x3_splitw_kernel",
    "f16x2-f192-s8-b1-n4-winograd-CATTUS_WINO_KERNEL=k4": "tower_wino4_kernel", "f16x2-f192-s8-b1-n132-auto-CATTUS_WINO_KERNEL=k4": "tower_wino4_kernel",
    "f16x2-f192-s8-b1-n132-winograd-CATTUS_WINO_KERNEL=k4": "tower_wino4_kernel",
    "f16x2-f64-s8-b1-n4-auto-CATTUS_WINO_PERSIST=0": "tower64_split_kernel", "f16x2-f64-s8-b1-n132-auto-CATTUS_WINO_PERSIST=0": "tower64_split_kernel",
    "f16x2-f128-s8-b1-n4-auto-CATTUS_WINO_PERSIST=0": "conv3x3_splitw_kernel",
    "f16x2-f128-s8-b1-n4-winograd-CATTUS_WINO_PERSIST=0": "conv3x3_wino4_kernel",
    "f16x2-f128-s8-b1-n132-auto-CATTUS_WINO_PERSIST=0": "conv3x3_wino4_kernel",
    "f16x2-f128-s8-b1-n132-winograd-CATTUS_WINO_PERSIST=0": "conv3x3_wino4_kernel",
    "f16x2-f192-s8-b1-n4-auto-CATTUS_WINO_PERSIST=0": "conv3x3_splitw_kernel",
    "f16x2-f192-s8-b1-n4-winograd-CATTUS_WINO_PERSIST=0": "conv3x3_wino4_kernel",
    "f16x2-f192-s8-b1-n132-auto-CATTUS_WINO_PERSIST=0": "conv3x3_wino4_kernel",
    "f16x2-f192-s8-b1-n132-winograd-CATTUS_WINO_PERSIST=0": "conv3x3_wino4_kernel", "bf16-f16-s8-b1-n4-auto": "tower64_lds_kernel",
    "bf16-f16-s8-b1-n128-auto": "tower64_lds_kernel", "bf16-f16-s8-b1-n132-auto": "tower64_lds_kernel", "bf16-f16-s8-b0-n4-auto": "tower64_lds_kernel",
    "bf16-f16-s8-b0-n128-auto": "tower64_lds_kernel", "bf16-f16-s8-b0-n132-auto": "tower64_lds_kernel", "bf16-f16-s9-b1-n4-auto": "tower64_lds_kernel",
    "bf16-f16-s9-b1-n128-auto": "tower64_lds_kernel", "bf16-f16-s9-b1-n132-auto": "tower64_lds_kernel", "bf16-f16-s9-b0-n4-auto": "tower64_lds_kernel",
    "bf16-f16-s9-b0-n128-auto": "tower64_lds_kernel", "bf16-f16-s9-b0-n132-auto": "tower64_lds_kernel", "bf16-f64-s8-b1-n4-auto": "tower64_lds_kernel",
    "bf16-f64-s8-b1-n128-auto": "tower64_lds_kernel", "bf16-f64-s8-b1-n132-auto": "tower64_lds_kernel", "bf16-f64-s8-b0-n4-auto": "tower64_lds_kernel",
    "bf16-f64-s8-b0-n128-auto": "tower64_lds_kernel", "bf16-f64-s8-b0-n132-auto": "tower64_lds_kernel", "bf16-f64-s9-b1-n4-auto": "tower64_lds_kernel",
    "bf16-f64-s9-b1-n128-auto": "tower64_lds_kernel", "bf16-f64-s9-b1-n132-auto": "tower64_lds_kernel", "bf16-f64-s9-b0-n4-auto": "tower64_lds_kernel",
    "bf16-f64-s9-b0-n128-auto": "tower64_lds_kernel", "bf16-f64-s9-b0-n132-auto": "tower64_lds_kernel",
    "bf16-f128-s8-b1-n4-auto": "conv3x3_mfma_v2_kernel", "bf16-f128-s8-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "bf16-f128-s8-b1-n132-auto": "conv3x3_mfma_v2_kernel", "bf16-f128-s8-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "bf16-f128-s8-b0-n128-auto": "conv3x3_mfma_v2_kernel", "bf16-f128-s8-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "bf16-f128-s9-b1-n4-auto": "conv3x3_mfma_v2_kernel", "bf16-f128-s9-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "bf16-f128-s9-b1-n132-auto": "conv3x3_mfma_v2_kernel", "bf16-f128-s9-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "bf16-f128-s9-b0-n128-auto": "conv3x3_mfma_v2_kernel", "bf16-f128-s9-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "bf16-f192-s8-b1-n4-auto": "conv3x3_mfma_v2_kernel", "bf16-f192-s8-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "bf16-f192-s8-b1-n132-auto": "conv3x3_mfma_v2_kernel", "bf16-f192-s8-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "bf16-f192-s8-b0-n128-auto": "conv3x3_mfma_v2_kernel", "bf16-f192-s8-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "bf16-f192-s9-b1-n4-auto": "conv3x3_mfma_v2_kernel", "bf16-f192-s9-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "bf16-f192-s9-b1-n132-auto": "conv3x3_mfma_v2_kernel", "bf16-f192-s9-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "bf16-f192-s9-b0-n128-auto": "conv3x3_mfma_v2_kernel", "bf16-f192-s9-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f16-f16-s8-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f16-f16-s8-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f16-f16-s8-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f16-f16-s8-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f16-f16-s8-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f16-f16-s8-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f16-f16-s9-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f16-f16-s9-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f16-f16-s9-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f16-f16-s9-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f16-f16-s9-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f16-f16-s9-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f16-f64-s8-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f16-f64-s8-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f16-f64-s8-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f16-f64-s8-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f16-f64-s8-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f16-f64-s8-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f16-f64-s9-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f16-f64-s9-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f16-f64-s9-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f16-f64-s9-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f16-f64-s9-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f16-f64-s9-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f16-f128-s8-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f16-f128-s8-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f16-f128-s8-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f16-f128-s8-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f16-f128-s8-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f16-f128-s8-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f16-f128-s9-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f16-f128-s9-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f16-f128-s9-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f16-f128-s9-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f16-f128-s9-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f16-f128-s9-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f16-f192-s8-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f16-f192-s8-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f16-f192-s8-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f16-f192-s8-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f16-f192-s8-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f16-f192-s8-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f16-f192-s9-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f16-f192-s9-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f16-f192-s9-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f16-f192-s9-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f16-f192-s9-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f16-f192-s9-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f16x2-f16-s8-b1-n4-auto": "tower64_split_kernel", "f16x2-f16-s8-b1-n128-auto": "tower64_split_kernel",
    "f16x2-f16-s8-b1-n132-auto": "tower64_split_kernel", "f16x2-f16-s8-b0-n4-auto": "tower64_split_kernel",
    "f16x2-f16-s8-b0-n128-auto": "tower64_split_kernel", "f16x2-f16-s8-b0-n132-auto": "tower64_split_kernel",
    "f16x2-f16-s9-b1-n4-auto": "tower64_split_kernel", "f16x2-f16-s9-b1-n128-auto": "tower64_split_kernel",
    "f16x2-f16-s9-b1-n132-auto": "tower64_split_kernel", "f16x2-f16-s9-b0-n4-auto": "tower64_split_kernel",
    "f16x2-f16-s9-b0-n128-auto": "tower64_split_kernel", "f16x2-f16-s9-b0-n132-auto": "tower64_split_kernel",
    "f16x2-f64-s8-b1-n4-auto": "tower64_split_kernel", "f16x2-f64-s8-b1-n128-auto": "tower64_split_kernel",
    "f16x2-f64-s8-b1-n132-auto": "tower64_split_kernel", "f16x2-f64-s8-b0-n4-auto": "tower64_split_kernel",
    "f16x2-f64-s8-b0-n128-auto": "tower64_split_kernel", "f16x2-f64-s8-b0-n132-auto": "tower64_split_kernel",
    "f16x2-f64-s9-b1-n4-auto": "tower64_split_kernel", "f16x2-f64-s9-b1-n128-auto": "tower64_split_kernel",
    "f16x2-f64-s9-b1-n132-auto": "tower64_split_kernel", "f16x2-f64-s9-b0-n4-auto": "tower64_split_kernel",
    "f16x2-f64-s9-b0-n128-auto": "tower64_split_kernel", "f16x2-f64-s9-b0-n132-auto": "tower64_split_kernel",
    "f16x2-f128-s8-b1-n4-auto": "conv3x3_splitw_kernel", "f16x2-f128-s8-b1-n128-auto": "conv3x3_splitw_kernel",
    "f16x2-f128-s8-b1-n132-auto": "tower_wino4_kernel", "f16x2-f128-s8-b0-n4-auto": "conv3x3_splitw_kernel",
    "f16x2-f128-s8-b0-n128-auto": "conv3x3_splitw_kernel", "f16x2-f128-s8-b0-n132-auto": "conv3x3_splitw_kernel",
    "f16x2-f128-s9-b1-n4-auto": "conv3x3_splitw_kernel", "f16x2-f128-s9-b1-n128-auto": "conv3x3_splitw_kernel",
    "f16x2-f128-s9-b1-n132-auto": "conv3x3_splitw_kernel", "f16x2-f128-s9-b0-n4-auto": "conv3x3_splitw_kernel",
    "f16x2-f128-s9-b0-n128-auto": "conv3x3_splitw_kernel", "f16x2-f128-s9-b0-n132-auto": "conv3x3_splitw_kernel",
    "f16x2-f192-s8-b1-n4-auto": "conv3x3_splitw_kernel", "f16x2-f192-s8-b1-n128-auto": "conv3x3_splitw_kernel",
    "f16x2-f192-s8-b1-n132-auto": "tower_wino4_kernel", "f16x2-f192-s8-b0-n4-auto": "conv3x3_splitw_kernel",
    "f16x2-f192-s8-b0-n128-auto": "conv3x3_splitw_kernel", "f16x2-f192-s8-b0-n132-auto": "conv3x3_splitw_kernel",
    "f16x2-f192-s9-b1-n4-auto": "conv3x3_splitw_kernel", "f16x2-f192-s9-b1-n128-auto": "conv3x3_splitw_kernel",
    "f16x2-f192-s9-b1-n132-auto": "conv3x3_splitw_kernel", "f16x2-f192-s9-b0-n4-auto": "conv3x3_splitw_kernel",
    "f16x2-f192-s9-b0-n128-auto": "conv3x3_splitw_kernel", "f16x2-f192-s9-b0-n132-auto": "conv3x3_splitw_kernel",
    "f32-f16-s8-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f32-f16-s8-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f32-f16-s8-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f32-f16-s8-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f32-f16-s8-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f32-f16-s8-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f32-f16-s9-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f32-f16-s9-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f32-f16-s9-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f32-f16-s9-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f32-f16-s9-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f32-f16-s9-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f32-f64-s8-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f32-f64-s8-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f32-f64-s8-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f32-f64-s8-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f32-f64-s8-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f32-f64-s8-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f32-f64-s9-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f32-f64-s9-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f32-f64-s9-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f32-f64-s9-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f32-f64-s9-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f32-f64-s9-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f32-f128-s8-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f32-f128-s8-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f32-f128-s8-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f32-f128-s8-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f32-f128-s8-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f32-f128-s8-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f32-f128-s9-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f32-f128-s9-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f32-f128-s9-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f32-f128-s9-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f32-f128-s9-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f32-f128-s9-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f32-f192-s8-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f32-f192-s8-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f32-f192-s8-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f32-f192-s8-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f32-f192-s8-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f32-f192-s8-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f32-f192-s9-b1-n4-auto": "conv3x3_mfma_v2_kernel", "f32-f192-s9-b1-n128-auto": "conv3x3_mfma_v2_kernel",
    "f32-f192-s9-b1-n132-auto": "conv3x3_mfma_v2_kernel", "f32-f192-s9-b0-n4-auto": "conv3x3_mfma_v2_kernel",
    "f32-f192-s9-b0-n128-auto": "conv3x3_mfma_v2_kernel", "f32-f192-s9-b0-n132-auto": "conv3x3_mfma_v2_kernel",
    "f16x2-f16-s8-b1-n4-direct": "tower64_split_kernel", "f16x2-f16-s8-b1-n128-direct": "tower64_split_kernel",
    "f16x2-f16-s8-b1-n132-direct": "tower64_split_kernel", "f16x2-f16-s8-b0-n4-direct": "tower64_split_kernel",
    "f16x2-f16-s8-b0-n128-direct": "tower64_split_kernel", "f16x2-f16-s8-b0-n132-direct": "tower64_split_kernel",
    "f16x2-f16-s9-b1-n4-direct": "tower64_split_kernel", "f16x2-f16-s9-b1-n128-direct": "tower64_split_kernel",
    "f16x2-f16-s9-b1-n132-direct": "tower64_split_kernel", "f16x2-f16-s9-b0-n4-direct": "tower64_split_kernel",
    "f16x2-f16-s9-b0-n128-direct": "tower64_split_kernel", "f16x2-f16-s9-b0-n132-direct": "tower64_split_kernel",
    "f16x2-f64-s8-b1-n4-direct": "tower64_split_kernel", "f16x2-f64-s8-b1-n128-direct": "tower64_split_kernel",
    "f16x2-f64-s8-b1-n132-direct": "tower64_split_kernel", "f16x2-f64-s8-b0-n4-direct": "tower64_split_kernel",
    "f16x2-f64-s8-b0-n128-direct": "tower64_split_kernel", "f16x2-f64-s8-b0-n132-direct": "tower64_split_kernel",
    "f16x2-f64-s9-b1-n4-direct": "tower64_split_kernel", "f16x2-f64-s9-b1-n128-direct": "tower64_split_kernel",
    "f16x2-f64-s9-b1-n132-direct": "tower64_split_kernel", "f16x2-f64-s9-b0-n4-direct": "tower64_split_kernel",
    "f16x2-f64-s9-b0-n128-direct": "tower64_split_kernel", "f16x2-f64-s9-b0-n132-direct": "tower64_split_kernel",
    "f16x2-f128-s8-b1-n4-direct": "conv3x3_splitw_kernel", "f16x2-f128-s8-b1-n128-direct": "conv3x3_splitw_kernel",
    "f16x2-f128-s8-b1-n132-direct": "conv3x3_splitw_kernel", "f16x2-f128-s8-b0-n4-direct": "conv3x3_splitw_kernel",
    "f16x2-f128-s8-b0-n128-direct": "conv3x3_splitw_kernel", "f16x2-f128-s8-b0-n132-direct": "conv3x3_splitw_kernel",
    "f16x2-f128-s9-b1-n4-direct": "conv3x3_splitw_kernel", "f16x2-f128-s9-b1-n128-direct": "conv3x3_splitw_kernel",
    "f16x2-f128-s9-b1-n132-direct": "conv3x3_splitw_kernel", "f16x2-f128-s9-b0-n4-direct": "conv3x3_splitw_kernel",
    "f16x2-f128-s9-b0-n128-direct": "conv3x3_splitw_kernel", "f16x2-f128-s9-b0-n132-direct": "conv3x3_splitw_kernel",
    "f16x2-f192-s8-b1-n4-direct": "conv3x3_splitw_kernel", "f16x2-f192-s8-b1-n128-direct": "conv3x3_splitw_kernel",
    "f16x2-f192-s8-b1-n132-direct": "conv3x3_splitw_kernel", "f16x2-f192-s8-b0-n4-direct": "conv3x3_splitw_kernel",
    "f16x2-f192-s8-b0-n128-direct": "conv3x3_splitw_kernel", "f16x2-f192-s8-b0-n132-direct": "conv3x3_splitw_kernel",
    "f16x2-f192-s9-b1-n4-direct": "conv3x3_splitw_kernel", "f16x2-f192-s9-b1-n128-direct": "conv3x3_splitw_kernel",
    "f16x2-f192-s9-b1-n132-direct": "conv3x3_splitw_kernel", "f16x2-f192-s9-b0-n4-direct": "conv3x3_splitw_kernel",
    "f16x2-f192-s9-b0-n128-direct": "conv3x3_splitw_kernel", "f16x2-f192-s9-b0-n132-direct": "conv3x3_splitw_kernel",
    "f16x2-f16-s8-b1-n4-winograd": "refused -2", "f16x2-f16-s8-b1-n128-winograd": "refused -2", "f16x2-f16-s8-b1-n132-winograd": "refused -2",
    "f16x2-f16-s8-b0-n4-winograd": "refused -2", "f16x2-f16-s8-b0-n128-winograd": "refused -2", "f16x2-f16-s8-b0-n132-winograd": "refused -2",
    "f16x2-f16-s9-b1-n4-winograd": "refused -2", "f16x2-f16-s9-b1-n128-winograd": "refused -2", "f16x2-f16-s9-b1-n132-winograd": "refused -2",
    "f16x2-f16-s9-b0-n4-winograd": "refused -2", "f16x2-f16-s9-b0-n128-winograd": "refused -2", "f16x2-f16-s9-b0-n132-winograd": "refused -2",
    "f16x2-f64-s8-b1-n4-winograd": "refused -2", "f16x2-f64-s8-b1-n128-winograd": "refused -2", "f16x2-f64-s8-b1-n132-winograd": "refused -2",
    "f16x2-f64-s8-b0-n4-winograd": "refused -2", "f16x2-f64-s8-b0-n128-winograd": "refused -2", "f16x2-f64-s8-b0-n132-winograd": "refused -2",
    "f16x2-f64-s9-b1-n4-winograd": "refused -2", "f16x2-f64-s9-b1-n128-winograd": "refused -2", "f16x2-f64-s9-b1-n132-winograd": "refused -2",
    "f16x2-f64-s9-b0-n4-winograd": "refused -2", "f16x2-f64-s9-b0-n128-winograd": "refused -2", "f16x2-f64-s9-b0-n132-winograd": "refused -2",
    "f16x2-f128-s8-b1-n4-winograd": "tower_wino4_kernel", "f16x2-f128-s8-b1-n128-winograd": "tower_wino4_kernel",
    "f16x2-f128-s8-b1-n132-winograd": "tower_wino4_kernel", "f16x2-f128-s8-b0-n4-winograd": "refused -2", "f16x2-f128-s8-b0-n128-winograd": "refused -2",
    "f16x2-f128-s8-b0-n132-winograd": "refused -2", "f16x2-f128-s9-b1-n4-winograd": "refused -2", "f16x2-f128-s9-b1-n128-winograd": "refused -2",
    "f16x2-f128-s9-b1-n132-winograd": "refused -2", "f16x2-f128-s9-b0-n4-winograd": "refused -2", "f16x2-f128-s9-b0-n128-winograd": "refused -2",
    "f16x2-f128-s9-b0-n132-winograd": "refused -2", "f16x2-f192-s8-b1-n4-winograd": "tower_wino4_kernel",
    "f16x2-f192-s8-b1-n128-winograd": "tower_wino4_kernel", "f16x2-f192-s8-b1-n132-winograd": "tower_wino4_kernel",
    "f16x2-f192-s8-b0-n4-winograd": "refused -2", "f16x2-f192-s8-b0-n128-winograd": "refused -2", "f16x2-f192-s8-b0-n132-winograd": "refused -2",
    "f16x2-f192-s9-b1-n4-winograd": "refused -2", "f16x2-f192-s9-b1-n128-winograd": "refused -2", "f16x2-f192-s9-b1-n132-winograd": "refused -2",
    "f16x2-f192-s9-b0-n4-winograd": "refused -2", "f16x2-f192-s9-b0-n128-winograd": "refused -2", "f16x2-f192-s9-b0-n132-winograd": "refused -2",
    "f32-f128-s8-b1-n132-direct": "conv3x3_mfma_v2_kernel", "f32-f128-s8-b1-n132-winograd": "refused -2",
    "bf16-f128-s8-b1-n132-direct": "conv3x3_mfma_v2_kernel", "bf16-f128-s8-b1-n132-winograd": "refused -2",
    "f16-f128-s8-b1-n132-direct": "conv3x3_mfma_v2_kernel", "f16-f128-s8-b1-n132-winograd": "refused -2", "wide-f32": "conv3x3_generic_kernel",
    "wide-bf16": "refused -2", "wide-f16x2": "refused -2", "simple-f32": "policy_fc_kernel", "simple-f16x2": "policy_fc_kernel",
}


def check(cid, blocks, got):
    name, launches, outs = got
    assert cid in EXPECTED, f"{cid}: no expected kernel name recorded (got {name})"
    assert name == EXPECTED[cid], (cid, name, EXPECTED[cid])
    if name.startswith("refused"):
        return
    for policy, value in outs:
        assert np.isfinite(policy).all() and np.isfinite(value).all(), cid
    if name == "policy_fc_kernel":
        assert launches == "refused -2", (cid, launches)  # a SimpleTwoHeadedModel has no conv tower to time
    else:
        assert launches == (1 if name in RESIDENT else 1 + 2 * blocks), (cid, name, launches)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_tower_kernel_of_every_plan_kind_and_fallback(group):
    for dtype, filters, board, blocks, batch, form, switch in GROUPS[group]:
        got = run_case(blob_of(filters, board, blocks), 1 if board == 8 else 2, dtype, batch, form, switch)
        check(case_id(dtype, filters, board, blocks, batch, form, switch), blocks, got)


def test_tower_kernel_of_wide_heads_and_simple_models():
    for cid, blob, words, dtype, batch in special_cases():
        check(cid, 1, run_case(blob, words, dtype, batch, "auto", ""))


def test_every_plan_kind_is_reached():
    assert {v for v in EXPECTED.values() if not v.startswith("refused")} == {
        "policy_fc_kernel", "conv3x3_generic_kernel", "conv3x3_mfma_v2_kernel", "conv3x3_splitw_kernel", "conv3x3_split_kernel",
        "tower64_lds_kernel", "tower64_split_kernel", "conv3x3_wino_kernel", "conv3x3_wino4_kernel", "tower_wino4_kernel"}
