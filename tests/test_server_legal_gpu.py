"""The leaf server with the legal-move softmax on the device: cattus_hip_submit_legal / wait_legal / apply_legal and
legal_softmax_ragged_kernel behind them.

Everything here is deterministic and a leaf's result does not depend on the batch it came in, so every comparison is exact: a leaf's
probabilities through the server are the bits cattus_hip_eval_legal writes for the same leaf and list (stride 1024, one batch), under f32
also the bits of oracle.softmax_legal_det on the f32 logits, and its value is cattus_hip_eval's.  No bound on any difference is set.

The net is chess-shaped -- 18 planes, 8x8, M = 1880, 1 block x 16 filters, vhc = phc = 4, seeded: the smallest one whose M allows a list of
1024 distinct moves.  max_batch is 8.  flush_us is the binding's default wherever a batch may seal by deadline; the tests that need ONE
batch of a known composition (the mixed batch, the two verification records that must be equal) use five seconds, as
test_verify_priors_gpu.py does: their batches are full or flushed, so nothing waits for that deadline."""

import functools
import threading

import numpy as np
import pytest

from cattus_amd.evaluator import CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, TTT, NetDesc, seeded_blob, simple_desc
from oracle import oracle

from test_many_planes_gpu import random_planes

pytestmark = pytest.mark.gpu

CATTUS_E_INVALID = -1
NET = NetDesc(**CHESS, blocks=1, filters=16, vhc=4, phc=4)
LENGTHS = (0, 1, 63, 64, 65, 218, 1023, 1024)  # across the wave width, odd offsets, the empty list and the cap
ONE_BATCH_US = 5_000_000


@functools.lru_cache(maxsize=None)
def blob() -> bytes:
    return seeded_blob(NET, 41)


@functools.lru_cache(maxsize=None)
def leaves():
    """(planes [8], the 8 lists): lengths LENGTHS, each a seeded shuffle of distinct moves."""
    rng = np.random.default_rng(17)
    lists = tuple(rng.permutation(NET.moves)[:c].astype(np.uint16) for c in LENGTHS)
    return random_planes(NET, 1, len(LENGTHS), 19), lists


def padded(lists, stride):
    idx = np.zeros((len(lists), stride), dtype=np.uint16)
    for i, l in enumerate(lists):
        idx[i, : len(l)] = l
    return idx, np.array([len(l) for l in lists], dtype=np.uint16)


@functools.lru_cache(maxsize=None)
def reference(dtype):
    """What the caller-assembled entry points give for the 8 leaves: (probs per leaf of eval_legal at stride 1024, logits and values of eval).
    Computed once per dtype and shared."""
    planes, lists = leaves()
    idx, cnt = padded(lists, 1024)
    with HipEvaluator(blob(), batch_size=8, plane_words=1, dtype=dtype, switches={}) as ev:
        logits, values = ev.eval(planes)
        probs, values_legal = ev.eval_legal(planes, idx, cnt)
        kernel = ev.tower_kernel()
    assert values_legal.tobytes() == values.tobytes()
    for arr in (logits, values, probs):
        arr.setflags(write=False)
    return tuple(probs[i, : len(l)] for i, l in enumerate(lists)), logits, values, kernel


def same_bits(got, want) -> bool:
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def check_leaf(dtype, i, probs, value):
    want_probs, _, want_values, _ = reference(dtype)
    assert same_bits(probs, want_probs[i]), (dtype, i, LENGTHS[i])
    assert same_bits(value, want_values[i]), (dtype, i, float(value), float(want_values[i]))


# ---------------------------------------------------------------------------------------- 1. bits


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_server_probabilities_are_eval_legals_bits(dtype):
    planes, lists = leaves()
    with HipEvaluator(blob(), batch_size=8, plane_words=1, dtype=dtype, switches={}) as ev:
        tickets = [ev.submit_legal(planes[i], lists[i]) for i in range(8)]
        ev.flush()
        got = [ev.wait_legal(t) for t in tickets]
        st = ev.stats()
    for i, (probs, value) in enumerate(got):
        assert len(probs) == LENGTHS[i]
        check_leaf(dtype, i, probs, value)
    assert st["positions"] == 8 and 1 <= st["batches"] <= 8
    if dtype == "f32":
        want_probs, logits, _, _ = reference("f32")
        for i, l in enumerate(lists):
            if len(l):
                assert same_bits(want_probs[i], oracle.softmax_legal_det(logits[i], l)), i  # the host restatement of the contract
                assert same_bits(got[i][0], oracle.softmax_legal_det(logits[i], l)), i


def test_simple_model_through_the_server():
    d = simple_desc(**TTT)
    sblob = seeded_blob(d, 7)
    planes = random_planes(d, 1, 3, 23)
    rng = np.random.default_rng(29)
    lists = [rng.permutation(9)[:c].astype(np.uint16) for c in (0, 1, 9)]
    idx, cnt = padded(lists, 9)
    with HipEvaluator(sblob, batch_size=8, plane_words=1, dtype="f32", switches={}) as ev:
        logits, values = ev.eval(planes)
        want, _ = ev.eval_legal(planes, idx, cnt)
    with HipEvaluator(sblob, batch_size=8, plane_words=1, dtype="f32", switches={}) as ev:
        tickets = [ev.submit_legal(planes[i], lists[i]) for i in range(3)]
        ev.flush()
        got = [ev.wait_legal(t) for t in tickets]
        probs, vals = ev.apply_legal(planes, lists)
    for i, l in enumerate(lists):
        assert same_bits(got[i][0], want[i, : len(l)]) and same_bits(got[i][1], values[i]), i
        assert same_bits(probs[i], want[i, : len(l)]) and same_bits(vals[i], values[i]), i
        if len(l):
            assert same_bits(got[i][0], oracle.softmax_legal_det(logits[i], l)), i


# ---------------------------------------------------------------------------------------- 2. a mixed batch


def test_mixed_batch_and_the_wrong_wait():
    planes, lists = leaves()
    _, logits, values, _ = reference("f32")
    with HipEvaluator(blob(), batch_size=8, plane_words=1, dtype="f32", switches={}, flush_us=ONE_BATCH_US) as ev:
        # plain leaves in the even slots, legal ones in the odd slots: lists of 1, 64, 218 and 1024 behind empty spans
        tickets = [ev.submit_legal(planes[i], lists[i]) if i % 2 else ev.submit(planes[i]) for i in range(8)]
        assert len({t >> 32 for t in tickets}) == 1  # one batch: it filled before any deadline
        for i, t in enumerate(tickets):
            with pytest.raises(CattusHipError) as err:
                ev.wait(t) if i % 2 else ev.wait_legal(t)
            assert err.value.status == CATTUS_E_INVALID, (i, err.value)
        for i, t in enumerate(tickets):  # refused, and still claimable by the right call
            if i % 2:
                check_leaf("f32", i, *ev.wait_legal(t))
            else:
                policy, value = ev.wait(t)
                assert same_bits(policy, logits[i]) and same_bits(value, values[i]), i
        st = ev.stats()
    assert st["batches"] == 1 and st["positions"] == 8 and st["full_batches"] == 1


# ---------------------------------------------------------------------------------------- 3. sealing


def test_a_lone_leaf_returns_by_the_deadline():
    planes, lists = leaves()
    with HipEvaluator(blob(), batch_size=8, plane_words=1, dtype="f32", switches={}) as ev:
        check_leaf("f32", 5, *ev.wait_legal(ev.submit_legal(planes[5], lists[5])))  # no flush: flush_us seals the batch of one
        st = ev.stats()
    assert st["batches"] == 1 and st["positions"] == 1 and st["full_batches"] == 0


def test_eight_threads_one_leaf_each():
    planes, lists = leaves()
    got, errors = [None] * 8, []
    with HipEvaluator(blob(), batch_size=8, plane_words=1, dtype="bf16", switches={}) as ev:

        def work(i):
            try:
                probs, vals = ev.apply_legal(planes[i : i + 1], [lists[i]])
                got[i] = (probs[0], vals[0])
            except Exception as exc:  # noqa: BLE001 -- reported below, in the main thread
                errors.append((i, exc))

        threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        st = ev.stats()
    assert not errors, errors
    for i in range(8):
        check_leaf("bf16", i, *got[i])
    assert st["positions"] == 8 and 1 <= st["batches"] <= 8


def test_apply_legal_over_three_batches_with_a_ragged_tail():
    planes, lists = leaves()
    order = [(3 * k + 1) % 8 for k in range(19)]  # 19 leaves: two full batches and a tail of three
    with HipEvaluator(blob(), batch_size=8, plane_words=1, dtype="f32", switches={}) as ev:
        probs, vals = ev.apply_legal(planes[order], [lists[i] for i in order])
        st = ev.stats()
    assert len(probs) == 19 and vals.shape == (19,)
    for k, i in enumerate(order):
        check_leaf("f32", i, probs[k], vals[k])
    assert st["positions"] == 19 and st["batches"] >= 3


# ---------------------------------------------------------------------------------------- 4. refusals


def test_refusals_queue_nothing():
    planes, lists = leaves()
    rng = np.random.default_rng(31)
    with HipEvaluator(blob(), batch_size=8, plane_words=1, dtype="f32", switches={}) as ev:
        bad_index = lists[5].copy()
        bad_index[100] = NET.moves
        refused = [
            lambda: ev.submit_legal(planes[0], rng.integers(0, NET.moves, size=1025)),  # one above the cap
            lambda: ev.submit_legal(planes[0], bad_index),  # an index of 1880
            lambda: ev.apply_legal_ragged(planes[:2], lists[5][:6], [1, 3, 6]),  # offsets not starting at 0
            lambda: ev.apply_legal_ragged(planes[:3], lists[5][:9], [0, 5, 4, 9]),  # offsets descending
            lambda: ev.apply_legal(planes[:2], [lists[1], bad_index]),  # the second leaf's list is bad: the first is not queued either
        ]
        for k, call in enumerate(refused):
            with pytest.raises(CattusHipError) as err:
                call()
            assert err.value.status == CATTUS_E_INVALID, (k, err.value)
        ev.flush()
        st = ev.stats()
        assert st["batches"] == 0 and st["positions"] == 0, st
        check_leaf("f32", 2, *ev.wait_legal(ev.submit_legal(planes[2], lists[2])))  # and the evaluator goes on working
        assert ev.stats()["batches"] == 1


# ---------------------------------------------------------------------------------------- 5. verification


def test_verified_server_batches_feed_the_prior_statistics():
    planes, lists = leaves()
    idx, cnt = padded(lists, 1024)
    want_probs, _, want_values, _ = reference("bf16")
    with HipEvaluator(blob(), batch_size=8, plane_words=1, dtype="bf16", switches={}, verify_every=1) as ev:
        ev.eval_legal(planes, idx, cnt)
        a_stats, a_worst = ev.verify_prior_stats(), ev.verify_worst_prior()
    with HipEvaluator(blob(), batch_size=8, plane_words=1, dtype="bf16", switches={}, flush_us=ONE_BATCH_US, verify_every=1) as ev:
        tickets = [ev.submit_legal(planes[i], lists[i]) for i in range(8)]
        ev.flush()
        for i, t in enumerate(tickets):
            check_leaf("bf16", i, *ev.wait_legal(t))  # a verified batch returns what an unverified one returns
        b_stats, b_worst = ev.verify_prior_stats(), ev.verify_worst_prior()
        st, vs = ev.stats(), ev.verify_stats()
    print("eval_legal:", a_stats, "\nserver:    ", b_stats)
    assert a_stats == b_stats  # leaves, flips, the float64 sums, maxima and histogram
    assert a_stats["batches"] == 1 and a_stats["leaves"] == 8 and a_stats["empty"] == 1 and a_stats["value_leaves"] == 8
    assert a_stats["batches_without_legal"] == 0 and b_stats["batches_without_legal"] == 0
    assert a_worst.keys() == b_worst.keys() and a_worst["top"] == b_worst["top"] and a_worst["top_ref"] == b_worst["top_ref"]
    assert (a_worst["planes"] == b_worst["planes"]).all() and a_worst["legal_idx"].tobytes() == b_worst["legal_idx"].tobytes()
    assert any(a_worst["legal_idx"].tobytes() == l.tobytes() and (a_worst["planes"] == planes[i]).all() for i, l in enumerate(lists))
    assert st["batches"] == 1 and st["positions"] == 8 and vs["batches"] == 1 and vs["leaves"] == 8

    # a mixed batch: 4 plain + 4 legal leaves -- the legal ones are the leaves of the record, all 8 feed the value part
    with HipEvaluator(blob(), batch_size=8, plane_words=1, dtype="bf16", switches={}, flush_us=ONE_BATCH_US, verify_every=1) as ev:
        tickets = [ev.submit_legal(planes[i], lists[i]) if i % 2 else ev.submit(planes[i]) for i in range(8)]
        for i, t in enumerate(tickets):
            if i % 2:
                check_leaf("bf16", i, *ev.wait_legal(t))
            else:
                assert same_bits(ev.wait(t)[1], want_values[i])
        mixed = ev.verify_prior_stats()
        worst = ev.verify_worst_prior()
        # and an all-plain batch still is one without legal moves
        tickets = [ev.submit(planes[i]) for i in range(8)]
        for t in tickets:
            ev.wait(t)
        after = ev.verify_prior_stats()
    print("mixed:", mixed)
    assert mixed["batches"] == 1 and mixed["leaves"] == 4 and mixed["batches_without_legal"] == 0 and mixed["empty"] == 0
    assert mixed["value_leaves"] == 8 and mixed["dvalue_mean"] == mixed["sum_dvalue"] / 8
    assert any(worst["legal_idx"].tobytes() == lists[i].tobytes() and (worst["planes"] == planes[i]).all() for i in (1, 3, 5, 7))
    assert after["batches_without_legal"] == 1 and after["batches"] == 1 and after["leaves"] == 4 and after["value_leaves"] == 16


# ---------------------------------------------------------------------------------------- 6. nothing else moved


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_existing_entry_points_return_what_they_returned(dtype):
    planes, lists = leaves()
    idx, cnt = padded(lists, 1024)
    want_probs, want_logits, want_values, want_kernel = reference(dtype)
    with HipEvaluator(blob(), batch_size=8, plane_words=1, dtype=dtype, switches={}) as ev:
        before = (*ev.eval(planes), *ev.eval_legal(planes, idx, cnt), ev.tower_kernel())
        ev.apply_legal(planes, lists)
        t_legal, t_plain = ev.submit_legal(planes[6], lists[6]), ev.submit(planes[6])
        ev.flush()
        ev.wait_legal(t_legal), ev.wait(t_plain)
        after = (*ev.eval(planes), *ev.eval_legal(planes, idx, cnt), ev.tower_kernel())
    for b, a in zip(before[:4], after[:4]):
        assert same_bits(b, a)
    assert same_bits(before[0], want_logits) and same_bits(before[1], want_values) and before[4] == after[4] == want_kernel
    for i, l in enumerate(lists):
        assert same_bits(after[2][i, : len(l)], want_probs[i]) and not after[2][i, len(l):].any()
