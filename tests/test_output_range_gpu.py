"""tanh_exact and exp_nonpos (cattus_amd/csrc/device_common.h, kernels.hip) over their whole range on the device, in every kernel they are
compiled into: the value sweep and the legal-move lists of test_output_range.py through the dial network (helpers.dial_tensors), whose
outputs the input planes set.  Every tower and head operand of the dial is 0, 1 or a power of two, so every dtype's tower hands the heads
the exact target and what is compared is the last operation alone.

Value paths, each named by tower_kernel() and its switches so that the test proves which code ran:

  f32, f32_chain            head_fc_pair_kernel<float> / head_fc_chain_kernel behind the per-layer f32 tower
  bf16                      head_fc_pair_kernel<__bf16> behind tower64_lds_kernel
  f16x2, f16                the f32 pair behind tower64_split_kernel / the per-layer f16 tower
  f32_resident, f16r_resident, f16_resident   head convs fused in the one-launch towers
  f32_generic, f32_wide     CATTUS_FORCE_GENERIC=1 and 40 head channels: value_fc2_tanh_kernel
  hex11_*                   128-slot boards, K padded in both FCs
  chess128_f16x2            the default plan above 128 leaves: the one-launch Winograd tower with an f32 stream in front of the same heads

Per path: bit-equal to oracle.OracleNet (the f32 paths by contract, the others because the dial is exact in their formats too); within
test_output_range.value_bound of forward_f64, exactly +-1 from
|target| = 10 on, |v| <= 1, v(-x) == -v(x) bitwise, non-decreasing over the sorted targets, and a leaf's bits the same alone, reversed and
in a ragged sub-batch.  Measured max |v - v64| per path is printed before anything is asserted.

The softmax runs through eval_legal (stride 1024), apply_legal_ragged, submit_legal / wait_legal and apply_legal on f32, and through
eval_legal and apply_legal_ragged on bf16."""

import functools

import numpy as np
import pytest

from cattus_amd.evaluator import HipEvaluator
from oracle import oracle

from helpers import dial_planes
from test_output_range import (FLT_MAX, check_softmax, dial, expected_logits, odd_bitwise, softmax_lists, value_bound, value_leaves, value_targets)

pytestmark = pytest.mark.gpu

MAX_BATCH = 512
F32 = np.float32

# id -> (net, dtype, HipEvaluator keywords, tower_kernel())
PATHS = {
    "f32": ("chess64", "f32", {}, "conv3x3_mfma_v2_kernel"),
    "f32_chain": ("chess64", "f32", {"head_chain_leaves": MAX_BATCH}, "conv3x3_mfma_v2_kernel"),
    "bf16": ("chess64", "bf16", {}, "tower64_lds_kernel"),
    "f16x2": ("chess64", "f16x2", {}, "tower64_split_kernel"),
    "f16": ("chess64", "f16", {}, "conv3x3_mfma_v2_kernel"),
    "f32_resident": ("chess64", "f32_resident", {}, "tower64_f32_kernel"),
    "f16r_resident": ("chess64", "f16r_resident", {}, "tower64_stream_kernel"),
    "f16_resident": ("chess64", "f16", {"tower_form": "resident"}, "tower64_lds_kernel"),
    "f32_generic": ("chess64", "f32", {"switches": {"CATTUS_FORCE_GENERIC": "1"}}, "conv3x3_generic_kernel"),
    "f32_wide": ("chess_wide", "f32", {}, "conv3x3_generic_kernel"),
    "hex11_f32": ("hex11", "f32", {}, "conv3x3_mfma_v2_kernel"),
    "hex11_f32_chain": ("hex11", "f32", {"head_chain_leaves": MAX_BATCH}, "conv3x3_mfma_v2_kernel"),
    "hex11_bf16": ("hex11", "bf16", {}, "tower64_lds_kernel"),
    "hex11_f16x2": ("hex11", "f16x2", {}, "tower64_split_kernel"),
    "hex11_f32_resident": ("hex11", "f32_resident", {}, "tower64_f32_kernel"),
    "chess128_f16x2": ("chess128", "f16x2", {}, "tower_wino4_kernel"),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b) -> bool:
    return all(x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def oracle_outputs(net):
    p, v = oracle.OracleNet(dial(net)[2]).forward(value_leaves(net)[0])
    p.setflags(write=False), v.setflags(write=False)
    return p, v


def picked(t):
    """Leaves run alone: both ends, both sides of both branch points, the smallest target and 0."""
    want = [-32.0, -10.0, -0.5, 0.0, 2.0**-20, 0.5 - 2.0**-25, 0.5, 10.0 - 2.0**-20, 10.0, 32.0]
    return [int(np.flatnonzero(t == F32(x))[0]) for x in want]


@pytest.mark.parametrize("path", list(PATHS))
def test_the_value_head_over_its_whole_range(path):
    net, dtype, kw, kernel = PATHS[path]
    kw = dict(kw)
    switches = kw.pop("switches", {})
    d, tensors, blob = dial(net)
    planes, t, shift, p64, v64 = value_leaves(net)
    n = len(t)
    with HipEvaluator(blob, batch_size=MAX_BATCH, plane_words=planes.shape[2], dtype=dtype, switches=switches, **kw) as ev:
        p, v = ev.eval(planes)
        assert ev.tower_kernel() == kernel, (path, ev.tower_kernel())
        chain = kw.get("head_chain_leaves", 0)
        assert ev.head_chain_leaves() == chain and ev.head_chain_batches() == (1 if chain else 0)
        rev = ev.eval(planes[::-1].copy())
        ragged = ev.eval(planes[37 : 37 + 45])
        alone = {i: ev.eval(planes[i : i + 1]) for i in picked(t)}
        assert ev.head_chain_batches() == ((3 + len(alone)) if chain else 0)
        saturated = ev.stats()["saturated"]
    err, bound = np.abs(v.astype(np.float64) - v64), value_bound(t, v64)
    op, ov = oracle_outputs(net)
    print("%s [%s, %s]: max |v - v64| %.3g, max err / bound %.3g (bound at that leaf %.3g); values differing from the oracle's bits: %d of %d; "
          "logits differing: %d" % (path, dtype, kernel, err.max(), (err / bound).max(), bound[np.argmax(err / bound)], int((bits(v) != bits(ov)).sum()), n,
                                    int((bits(p) != bits(op)).sum())))
    assert saturated == 0
    # the oracle's bits -- on every path, not only the f32 ones: the dial hands every dtype's heads the exact target, FC2's sum of ladder
    # terms is exact in any order, and tanh_exact is f32 code wherever it is compiled
    assert same((p, v), (op, ov)), path
    assert np.isfinite(v).all() and (err <= bound).all(), (path, t[np.argmax(err / bound)])
    assert (v[t >= 10] == 1).all() and (v[t <= -10] == -1).all() and (np.abs(v) <= 1).all()
    assert (np.abs(v[np.abs(t) < 10]) < 1).sum() > 400  # and the sweep below 10 is not all saturated
    assert odd_bitwise(v)
    assert (np.diff(v) >= 0).all(), t[np.flatnonzero(np.diff(v) < 0)]
    # a leaf's bits do not depend on its batch
    assert same(rev, (p[::-1], v[::-1])), (path, "reversed")
    assert same(ragged, (p[37 : 37 + 45], v[37 : 37 + 45])), (path, "ragged")
    for i, one in alone.items():
        assert same(one, (p[i : i + 1], v[i : i + 1])), (path, "alone", float(t[i]))
    # logits: the scrub where the table is not finite, finite everywhere else; every dial operand is exact in every dtype, the bias is f32
    table = tensors["_policy_head.2.bias"]
    assert (bits(p[:, ~np.isfinite(table)]) == bits(F32(-FLT_MAX))).all() and np.isfinite(p).all()


# ---------------------------------------------------------------------------------------- the legal-move softmax
@functools.lru_cache(maxsize=None)
def softmax_leaves():
    """(planes, lists, shift bits, padded idx [n, 1024], counts, concatenated idx, offsets) of softmax_lists(): one leaf per list."""
    d = dial("chess64")[0]
    lists = softmax_lists()
    shift = np.array([s for _, s, _ in lists])
    targets = value_targets()[:: len(value_targets()) // len(lists)][: len(lists)]
    planes = dial_planes(d, targets, shift, seed=9)
    idx = np.zeros((len(lists), 1024), dtype=np.uint16)
    for i, (_, _, l) in enumerate(lists):
        idx[i, : len(l)] = l
    cnt = np.array([len(l) for _, _, l in lists], dtype=np.uint16)
    off = np.zeros(len(lists) + 1, dtype=np.uint32)
    np.cumsum(cnt, out=off[1:])
    return planes, lists, shift, idx, cnt, np.concatenate([l for _, _, l in lists]), off, targets


def check_rows(label, lists, logits, rows):
    """Every list's probabilities: the restatement's bits on these logits, the float64 bars, and the values known without arithmetic."""
    worst_a = worst_r = 0.0
    by_name = {}
    for i, (name, _, l) in enumerate(lists):
        got = rows[i]
        assert got.shape == (len(l),)
        assert np.array_equal(bits(got), bits(oracle.softmax_legal_det(logits[i], l))), (label, name)
        ea, er = check_softmax((label, name), got, logits[i], l)
        worst_a, worst_r = max(worst_a, ea), max(worst_r, er)
        by_name[name] = got
    print("%s: softmax vs float64 over %d lists: max abs %.3g, max rel above 1e-30 %.3g" % (label, len(lists), worst_a, worst_r))
    assert (by_name["equal_1024"] == F32(2.0**-10)).all() and (by_name["equal_shifted_512"] == F32(2.0**-9)).all()
    assert by_name["max_first"][0] == 1 and not by_name["max_first"][1:].any()
    assert by_name["max_middle"][17] == 1 and np.count_nonzero(by_name["max_middle"]) == 1
    assert by_name["max_over_shifted"][300] == 1 and np.count_nonzero(by_name["max_over_shifted"]) == 1
    assert (by_name["scrubbed_only"] == F32(1.0) / F32(96.0)).all() and by_name["scrubbed_one"].tolist() == [1.0]
    c = by_name["cutoff"]
    assert c[0] == 1 and c[2] == 0 and 0 < c[1] < c[3] < 2e-35
    c = by_name["cutoff_under_50"]
    assert c[3] == 1 and (c[:3] > 0).all() and (c[:3] < 2e-35).all()


def test_the_legal_softmax_over_its_whole_domain_f32():
    planes, lists, shift, idx, cnt, flat, off, targets = softmax_leaves()
    n = len(lists)
    blob = dial("chess64")[2]
    with HipEvaluator(blob, batch_size=64, plane_words=1, dtype="f32", switches={}) as ev:
        logits, values = ev.eval(planes)
        strided, v1 = ev.eval_legal(planes, idx, cnt)
        ragged, v2 = ev.apply_legal_ragged(planes, flat, off)
        tickets = [ev.submit_legal(planes[i], lists[i][2]) for i in range(n)]
        ev.flush()
        served = [ev.wait_legal(tk) for tk in tickets]
        applied, v4 = ev.apply_legal(planes, [l for _, _, l in lists])
        assert ev.tower_kernel() == "conv3x3_mfma_v2_kernel"
    for i in range(n):
        assert np.array_equal(bits(logits[i]), bits(expected_logits(bool(shift[i])))), lists[i][0]
    assert np.array_equal(bits(values), bits(np.array([oracle.tanhf(float(x)) for x in targets], dtype=np.float32)))
    for i in range(n):
        assert not strided[i, cnt[i] :].any(), lists[i][0]  # zeros past the count
    check_rows("eval_legal f32", lists, logits, [strided[i, : cnt[i]] for i in range(n)])
    check_rows("apply_legal_ragged f32", lists, logits, [ragged[off[i] : off[i + 1]] for i in range(n)])
    check_rows("submit_legal / wait_legal f32", lists, logits, [s[0] for s in served])
    check_rows("apply_legal f32", lists, logits, applied)
    # the ragged and the strided kernel give the same bits, and every entry point the same value
    assert np.array_equal(bits(ragged), bits(np.concatenate([strided[i, : cnt[i]] for i in range(n)])))
    for other in (v1, v2, v4, np.array([s[1] for s in served], dtype=np.float32)):
        assert np.array_equal(bits(other), bits(values))


def test_the_legal_softmax_over_its_whole_domain_bf16():
    """The bf16 heads' policy bias path: the logits are the f32 table's (every operand is exact in bf16, the bias is added in f32), and
    both softmax kernels give the restatement's bits on them."""
    planes, lists, shift, idx, cnt, flat, off, targets = softmax_leaves()
    n = len(lists)
    blob = dial("chess64")[2]
    with HipEvaluator(blob, batch_size=64, plane_words=1, dtype="bf16", switches={}) as ev:
        logits, values = ev.eval(planes)
        strided, v1 = ev.eval_legal(planes, idx, cnt)
        ragged, v2 = ev.apply_legal_ragged(planes, flat, off)
        assert ev.tower_kernel() == "tower64_lds_kernel"
    print("bf16: logits differing from the f32 table's bits: %d" % sum(int((bits(logits[i]) != bits(expected_logits(bool(shift[i])))).sum()) for i in range(n)))
    for i in range(n):
        assert np.array_equal(bits(logits[i]), bits(expected_logits(bool(shift[i])))), lists[i][0]
        assert not strided[i, cnt[i] :].any(), lists[i][0]
    check_rows("eval_legal bf16", lists, logits, [strided[i, : cnt[i]] for i in range(n)])
    check_rows("apply_legal_ragged bf16", lists, logits, [ragged[off[i] : off[i + 1]] for i in range(n)])
    assert np.array_equal(bits(ragged), bits(np.concatenate([strided[i, : cnt[i]] for i in range(n)])))
    assert np.array_equal(bits(v1), bits(values)) and np.array_equal(bits(v2), bits(values))
