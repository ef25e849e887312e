"""The f32 heads' FC pair as short fmaf chains (cattus_hip_head_chain, head_fc_chain_kernel).

The chain form gives a lane one output element and walks its dot product with v_fma_f32 in the order the MFMA pair's lanes produce; its
logits, values and priors equal, BIT FOR BIT, what the same evaluator returns with the setting 0 -- head_fc_pair_kernel<float>, the
reference side of every comparison here (uint32 views, no tolerance) -- and, for dtype f32, the CPU oracle's.  Nets of one block,
max_batch 40 (hv holds 64 leaves), the smallest at which the kernel can go wrong:

  ttt 3x3, 8 filters, vhc 4 / phc 8   K1 != K2; K = 36 -> 48 and 72 -> 80 (padded terms); M = 9
  hex7, 16 filters, vhc = phc = 16     K = 784 (two straight-line groups); M = 49: one partial strip
  chess, 16 filters, vhc = phc = 8     K = 512; M = 1880: 15 strips, 88 outputs in the last
  hex9, 16 filters, vhc = phc = 4      128-slot boards; K = 324 -> 336
  chess 1x128                          per-layer tower: hv written by head_conv_kernel, not by a resident tail

Leaves: 1, 16 and 17 (one output per lane up to HC_SINGLE_MAX = 16 leaves, two beyond), 31 and 33 (odd counts: a lane's second leaf
missing), 40, and 1 again behind 40."""

import ctypes as C
import functools

import numpy as np
import pytest

from cattus_amd import synth
from cattus_amd.evaluator import CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, TTT, NetDesc, hex_game, pack_tensors, seeded_blob, seeded_tensors, simple_desc

pytestmark = pytest.mark.gpu

MAX_BATCH = 40
LEAVES = (1, 16, 17, 31, 33, 40, 1)
NETS = {
    "ttt": (NetDesc(**TTT, blocks=1, filters=8, vhc=4, phc=8), 1),
    "hex7": (NetDesc(**hex_game(7), blocks=1, filters=16, vhc=16, phc=16), 2),
    "chess16": (NetDesc(**CHESS, blocks=1, filters=16, vhc=8, phc=8), 1),
    "hex9": (NetDesc(**hex_game(9), blocks=1, filters=16, vhc=4, phc=4), 2),
    "chess128": (NetDesc(**CHESS, blocks=1, filters=128, vhc=8, phc=8), 1),
}
DTYPES = ("f32", "f16x2", "f16", "f16r_resident")
FLT_MAX_BITS = 0xFF7FFFFF  # -FLT_MAX


@functools.lru_cache(maxsize=None)
def net(name):
    d, words = NETS[name]
    return seeded_blob(d, 77), words


@functools.lru_cache(maxsize=None)
def leaves(name):
    d, _ = NETS[name]
    if name == "ttt":
        return synth.random_ttt_planes(MAX_BATCH, 9)
    if name.startswith("hex"):
        return synth.random_hex_planes(MAX_BATCH, d.board, 9)
    return synth.random_chess_planes(MAX_BATCH, 9)


def evaluator(name, dtype, blob=None, **kw):
    b, words = net(name)
    return HipEvaluator(blob or b, batch_size=MAX_BATCH, plane_words=words, dtype=dtype, switches={}, **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def oracle_outputs(name):
    from oracle import oracle

    return oracle.OracleNet(net(name)[0]).forward(leaves(name))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(NETS))
def test_the_chain_form_has_the_mfma_pairs_bits(name, dtype):
    if dtype == "f16r_resident":  # where it is accepted: networks the one-launch tower covers (at most 64 filters, ...)
        try:
            evaluator(name, dtype).close()
        except CattusHipError as err:
            assert err.status == -2, err  # CATTUS_E_UNSUPPORTED: nothing runs under this dtype, so there is nothing to compare
            assert NETS[name][0].filters > 64, "refused on a network of at most 64 filters"
            return
    planes, d = leaves(name), NETS[name][0]
    rng = np.random.default_rng(3)
    L = min(d.moves, 24)
    legal_idx = np.stack([rng.choice(d.moves, size=L, replace=False) for _ in range(MAX_BATCH)]).astype(np.uint16)
    legal_count = rng.integers(1, L + 1, size=MAX_BATCH).astype(np.uint16)
    with evaluator(name, dtype) as ref, evaluator(name, dtype) as ev:
        ev.head_chain(MAX_BATCH)
        assert ev.head_chain_leaves() == MAX_BATCH and ref.head_chain_leaves() == 0
        for i, n in enumerate(LEAVES):
            want, got = ref.eval(planes[:n]), ev.eval(planes[:n])
            print(name, dtype, n, "logits differing:", int((bits(got[0]) != bits(want[0])).sum()), "values differing:", int((bits(got[1]) != bits(want[1])).sum()))
            assert same(got, want), (name, dtype, n)
            assert ev.head_chain_batches() == i + 1
            if dtype == "f32":
                op, ov = oracle_outputs(name)
                assert same(got, (op[:n], ov[:n])), (name, n, "against the CPU oracle")
        count = len(LEAVES)
        if name == "chess16":  # the priors a search receives
            for n in (17, 40):
                want, got = ref.eval_legal(planes[:n], legal_idx[:n], legal_count[:n]), ev.eval_legal(planes[:n], legal_idx[:n], legal_count[:n])
                assert same(got, want), (dtype, n, "eval_legal")
                count += 1
        # one leaf through the leaf server
        f32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
        out = []
        for e in (ref, ev):
            p, v = np.empty((1, d.moves), dtype=np.float32), np.empty((1,), dtype=np.float32)
            leaf = np.ascontiguousarray(planes[5:6])
            assert e._lib.cattus_hip_apply(e._h, leaf.ctypes.data_as(u64p), 1, p.ctypes.data_as(f32p), v.ctypes.data_as(f32p)) == 0
            out.append((p, v))
        assert same(out[1], out[0]), (name, dtype, "apply")
        assert ev.head_chain_batches() == count + 1 and ref.head_chain_batches() == 0
        assert ev.stats()["saturated"] == ref.stats()["saturated"]


def test_the_scrub():
    """+inf and NaN in the policy FC's bias: -FLT_MAX at those two moves in both forms, the same bits everywhere else."""
    d, _ = NETS["chess16"]
    t = seeded_tensors(d, 77)
    bias = t["_policy_head.2.bias"].copy()
    bias[3], bias[1879] = np.inf, np.nan
    t["_policy_head.2.bias"] = bias
    blob = pack_tensors(d, t)
    planes = leaves("chess16")
    with evaluator("chess16", "f32", blob) as ref, evaluator("chess16", "f32", blob, head_chain_leaves=MAX_BATCH) as ev:
        assert ev.head_chain_leaves() == MAX_BATCH
        for n in (5, 33):
            want, got = ref.eval(planes[:n]), ev.eval(planes[:n])
            for p in (want[0], got[0]):
                assert (bits(p)[:, 3] == FLT_MAX_BITS).all() and (bits(p)[:, 1879] == FLT_MAX_BITS).all(), n
                assert np.isfinite(np.delete(p, (3, 1879), axis=1)).all()
            assert same(got, want), n
        assert ev.head_chain_batches() == 2


def test_the_boundary_and_the_setting_zero_again():
    planes = leaves("hex7")
    with evaluator("hex7", "f16x2") as ref, evaluator("hex7", "f16x2") as ev:
        ev.head_chain(8)
        assert ev.head_chain_leaves() == 8
        assert same(ev.eval(planes[:8]), ref.eval(planes[:8])) and ev.head_chain_batches() == 1
        assert same(ev.eval(planes[:9]), ref.eval(planes[:9])) and ev.head_chain_batches() == 1
        ev.head_chain(0)
        assert ev.head_chain_leaves() == 0
        assert same(ev.eval(planes[:8]), ref.eval(planes[:8])) and ev.head_chain_batches() == 1
        ev.head_chain(MAX_BATCH)
        assert same(ev.eval(planes[:9]), ref.eval(planes[:9])) and ev.head_chain_batches() == 2


def test_refusals_and_ignores():
    planes = leaves("chess16")
    with evaluator("chess16", "f32") as ev:
        with pytest.raises(CattusHipError) as err:
            ev.head_chain(MAX_BATCH + 1)
        assert err.value.status == -1  # CATTUS_E_INVALID
        assert ev.head_chain_leaves() == 0
    with pytest.raises(CattusHipError) as err:
        evaluator("chess16", "f32", head_chain_leaves=MAX_BATCH + 1)
    assert err.value.status == -1
    wide = seeded_blob(NetDesc(**CHESS, blocks=1, filters=16, vhc=8, phc=32), 5)  # 40 head channels: the generic path
    simple = seeded_blob(simple_desc(**TTT), 5)
    cases = [("bf16", None, planes, 1), ("f32", wide, planes, 1), ("f32", simple, synth.random_ttt_planes(MAX_BATCH, 9), 1)]
    for dtype, blob, pl, words in cases:
        kw = dict(batch_size=MAX_BATCH, plane_words=words, dtype=dtype, switches={})
        b = blob or net("chess16")[0]
        with HipEvaluator(b, **kw) as ref, HipEvaluator(b, **kw) as ev:
            before = ev.eval(pl[:17])
            ev.head_chain(MAX_BATCH)
            assert ev.head_chain_leaves() == 0
            after = ev.eval(pl[:17])
            assert same(after, before) and same(after, ref.eval(pl[:17])), dtype
            assert ev.head_chain_batches() == 0


def test_observed_passes_keep_their_outputs():
    planes = leaves("hex7")[:17]
    with evaluator("hex7", "f16x2") as ref, evaluator("hex7", "f16x2", head_chain_leaves=MAX_BATCH) as ev:
        point = ev.points() - 1
        a, pa, va = ev.tap(planes, point, outputs=True)
        b, pb, vb = ref.tap(planes, point, outputs=True)
        assert same((a, pa, va), (b, pb, vb))
        assert same((pa, va), ev.eval(planes))
        ra, tpa, tva = ev.trace(planes)
        rb, tpb, tvb = ref.trace(planes)
        assert ra.tobytes() == rb.tobytes() and same((tpa, tva), (tpb, tvb))
        assert ev.head_chain_batches() == 1  # the one eval: an observed pass keeps the MFMA pair and is not a batch
