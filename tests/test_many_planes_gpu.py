"""Networks with more than 32 input planes on every dtype, and the separate plane pack as a second route through the f16 stems.

Until this file, dtype f16x2 (the product default) and f16 refused a network with more than 32 input planes: their stems expand the
bitboard planes inside the conv kernel (STEM variant, one 128-byte chunk) and no plane pack existed for their activation layouts.  Now
pack_planes_nhwc_kernel writes all four layouts (f16: _Float16 rows; f16x2: pairs, [hi of 32 channels | lo of the same 32] per 128
bytes, hi = f16(bit), lo = 0), the stem then runs as an ordinary layer of cpad0 input channels (f16x2: a multiple of 64, the chunk
counts hidden layers run), and CATTUS_FUSED_STEM=0 forces that path for networks of at most 32 planes too -- which is what the comment
above test_hip_parity.py::test_fused_stem_equals_separate_plane_pack says was missing: here the switch has something to compare.

Shapes: the smallest at which each code path can go wrong (vhc = phc = 4, moves = board^2 + 3, planes random bits in EVERY plane):

    id  board / words  planes  filters x blocks    n   what it reaches
    A   8 / 1            33    64 x 1              5   one real channel in the second chunk; <= 64 filters falls to PerLayer
    B   8 / 1            40    128 x 1             9   tower_form DIRECT and WINOGRAD (stem with CONV_WINO_IN, f32 rows out)
    C   11 / 2           40    24 x 1              3   128-slot boards (BIG), padded filters
    D   7 / 2            64    64 x 1            130   128 plane words (the limit), many workgroups, ragged batch
    E   8 / 1           119    64 x 2             70   four pair chunks / two f16 chunks (AlphaZero's chess input)
    F   8 / 1            40    256 x 1           256   the 64-cout tile (CB = 2)

Bars.  f16x2: helpers.outputs_equal_ref_tol -- the reference's own cross-runtime bar, the one every f16x2 shape test here uses -- against
helpers.forward_f64 (float64, from the raw tensors) cast to f32, and against the f32 tower.  The f32 oracle alone holds that bar against
forward_f64 with room to spare (measured on the CPU on 6-leaf batches of networks at A-E's planes / board / filters: max |dlogit| <=
3.1e-7, max |dvalue| <= 4.3e-8 at logits up to 0.7).  f16: no fixed bound; its errors against forward_f64 are at most
helpers.F16_OVER_BF16_MAX of the bf16 tower's on the same leaves (the bf16 many-plane path predates this file).  f32 on these shapes is
pinned to the oracle bit for bit, so the f16 family is held to a tested neighbour.
"""

import functools

import numpy as np
import pytest

from cattus_amd.evaluator import CattusHipError, HipEvaluator
from cattus_amd.weights import CHESS, NetDesc, hex_game, pack_tensors, seeded_blob, seeded_tensors
from oracle import oracle

from helpers import F16_OVER_BF16_MAX, forward_f64, outputs_equal_ref_tol

pytestmark = pytest.mark.gpu

CATTUS_E_UNSUPPORTED = -2

# id: (board, plane words, planes, filters, blocks, n)
SHAPES = {
    "A": (8, 1, 33, 64, 1, 5),
    "B": (8, 1, 40, 128, 1, 9),
    "C": (11, 2, 40, 24, 1, 3),
    "D": (7, 2, 64, 64, 1, 130),
    "E": (8, 1, 119, 64, 2, 70),
    "F": (8, 1, 40, 256, 1, 256),
}
# tower forms an f16x2 evaluator of the shape is run in: B in both by name; F direct (the CB = 2 tile on every layer) and as
# cattus_hip_create chooses for 256 leaves (the Winograd tower behind the direct stem)
FORMS = {"B": ("direct", "winograd"), "F": ("direct", "auto")}


def random_planes(d: NetDesc, words: int, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    hw = d.board * d.board
    planes = np.zeros((n, d.planes, words), dtype=np.uint64)
    bits = rng.integers(0, 2, size=(n, d.planes, hw), dtype=np.uint64)
    for i in range(hw):
        planes[:, :, i >> 6] |= bits[:, :, i] << np.uint64(i & 63)
    assert (planes.reshape(n, d.planes, -1).max(axis=2) > 0).all()  # every plane populated
    return planes


@functools.lru_cache(maxsize=None)
def case(sid: str):
    """A shape's network, leaves and float64 outputs: made once, shared, never written to."""
    board, words, nplanes, filters, blocks, n = SHAPES[sid]
    d = NetDesc(planes=nplanes, board=board, moves=board * board + 3, blocks=blocks, filters=filters, vhc=4, phc=4)
    tensors = seeded_tensors(d, 41)
    planes = random_planes(d, words, n, 9)
    p64, v64 = forward_f64(d, tensors, planes)
    for a in (planes, p64, v64):
        a.setflags(write=False)
    return d, pack_tensors(d, tensors), words, planes, p64, v64


def run(sid: str, dtype: str, switches=None, tower_form="auto", sub=None):
    """(policy, value) of the shape's leaves on one evaluator; with `sub`, also of that slice evaluated alone."""
    d, blob, words, planes, _, _ = case(sid)
    with HipEvaluator(blob, batch_size=len(planes), plane_words=words, dtype=dtype, tower_form=tower_form, switches=switches or {}) as ev:
        out = ev.eval(planes)
        if dtype in ("f16x2", "f16"):
            assert ev.stats()["saturated"] == 0
            channels, packed = ev.stem_input()
            assert channels == (d.planes + 63) // 64 * 64 and packed, (sid, dtype, channels, packed)
        return out if sub is None else (out, ev.eval(planes[sub]))


@functools.lru_cache(maxsize=None)
def f32_outputs(sid: str):
    p, v = run(sid, "f32")
    p.setflags(write=False), v.setflags(write=False)
    return p, v


def errors(out, sid):
    _, _, _, _, p64, v64 = case(sid)
    return float(np.abs(out[0] - p64).max()), float(np.abs(out[1] - v64).max())


# ---------------------------------------------------------------------------------------- 1. f16x2 against float64


@pytest.mark.parametrize("sid", sorted(SHAPES))
def test_f16x2_within_the_reference_bar_of_float64_on_both_weight_paths(sid):
    """Every leaf of A-F inside the reference's cross-runtime bar of the float64 network and of the f32 tower; the register-ring
    kernel (default) and the LDS-ring kernel (CATTUS_SPLIT_W=0) read the packed stem input alike: the same bits."""
    _, _, _, _, p64, v64 = case(sid)
    want_p, want_v = f32_outputs(sid)
    for form in FORMS.get(sid, ("auto",)):
        got_p, got_v = run(sid, "f16x2", tower_form=form)
        print("%s %s: f16x2 vs f64 max |dlogit| %.3g |dvalue| %.3g, max |logit| %.3g" % ((sid, form) + errors((got_p, got_v), sid) + (float(np.abs(p64).max()),)))
        assert np.isfinite(got_p).all() and np.isfinite(got_v).all()
        assert outputs_equal_ref_tol(got_p, got_v, p64.astype(np.float32), v64.astype(np.float32)), (sid, form, errors((got_p, got_v), sid))
        assert outputs_equal_ref_tol(got_p, got_v, want_p, want_v), (sid, form, np.abs(got_p - want_p).max(), np.abs(got_v - want_v).max())
        rows_p, rows_v = run(sid, "f16x2", switches={"CATTUS_SPLIT_W": "0"}, tower_form=form)
        assert (rows_p == got_p).all() and (rows_v == got_v).all(), (sid, form)


# ---------------------------------------------------------------------------------------- 2. f16 against float64


@pytest.mark.parametrize("sid", ["A", "C", "E"])
def test_f16_error_is_at_most_a_quarter_of_the_bf16_towers(sid):
    """Single-term f16 (11 significant bits) on packed stem input: finite, and against the float64 network at most
    F16_OVER_BF16_MAX of the bf16 tower's (8 bits) error on the same leaves, computed here -- no fixed bound."""
    f16 = run(sid, "f16")
    bf16 = run(sid, "bf16")
    (ep, ev), (bp, bv) = errors(f16, sid), errors(bf16, sid)
    print("%s: f16 vs f64 max |dlogit| %.3g |dvalue| %.3g; bf16 vs f64 %.3g %.3g" % (sid, ep, ev, bp, bv))
    assert np.isfinite(f16[0]).all() and np.isfinite(f16[1]).all()
    assert ep <= F16_OVER_BF16_MAX * bp and ev <= F16_OVER_BF16_MAX * bv, (sid, ep, ev, bp, bv)


# ---------------------------------------------------------------------------------------- 3. batch independence


@pytest.mark.parametrize("dtype", ["f16x2", "f16"])
@pytest.mark.parametrize("sid", ["D", "F"])
def test_a_leafs_bits_do_not_depend_on_its_batch(sid, dtype):
    """A sub-batch planes[k : 2k + 1] alone (other boards per workgroup, another grid, another tile) gives the bits it had in the full
    batch: the pack writes whole boards, zero rows behind the batch's end."""
    k = SHAPES[sid][5] // 3
    (p, v), (sub_p, sub_v) = run(sid, dtype, sub=slice(k, 2 * k + 1))
    assert (sub_p == p[k : 2 * k + 1]).all() and (sub_v == v[k : 2 * k + 1]).all()


# ---------------------------------------------------------------------------------------- 4. the new path against the fused stem


def small_net(which: str):
    if which == "chess2x128":
        return NetDesc(**CHESS, blocks=2, filters=128, vhc=8, phc=8), 1, 61
    return NetDesc(**hex_game(11), blocks=2, filters=8, vhc=4, phc=4), 2, 21


@pytest.mark.parametrize("which,dtype,form,batch", [
    ("chess2x128", "f16x2", "auto", None), ("chess2x128", "f16", "auto", None), ("chess2x128", "f16x2", "winograd", 64),
    ("hex11_2x8", "f16x2", "auto", None), ("hex11_2x8", "f16", "auto", None),  # f16x2: the resident tower against the per-layer kernels
])
def test_packed_stem_equals_the_fused_stem_bit_for_bit(which, dtype, form, batch):
    """Networks of at most 32 planes: under CATTUS_FUSED_STEM=0 the planes go through pack_planes_nhwc_kernel and the stem runs on
    the kernel without STEM -- for f16x2 with 64 input channels and weights laid out for them, the second chunk all zero weights
    on all zero activations.  Per accumulator the MFMA sequence is the same template's and the added products are +0: the same
    policy and value bits as the stem that expands the planes itself.  The switch must have been honoured (it used to be ignored
    for the f16 family): the plane pack runs as its own launch, and the f16x2 stem has 64 input channels against 32."""
    d, words, n = small_net(which)
    blob = seeded_blob(d, 29)
    planes = random_planes(d, words, n, 12)
    outs, stems = [], []
    for sw in ({}, {"CATTUS_FUSED_STEM": "0"}):
        with HipEvaluator(blob, batch_size=batch or n, plane_words=words, dtype=dtype, tower_form=form, switches=sw) as ev:
            outs.append(ev.eval(planes))
            stems.append(ev.stem_input())
            assert ev.stats()["saturated"] == 0
    assert stems[0] == ((32 if dtype == "f16x2" else 64), False), stems
    assert stems[1] == (64, True), stems
    assert (outs[1][0] == outs[0][0]).all() and (outs[1][1] == outs[0][1]).all()


# ---------------------------------------------------------------------------------------- 5. f32 / bf16 on the same shapes


@pytest.mark.parametrize("sid", ["A", "E"])
def test_f32_many_planes_equals_the_oracle_bit_for_bit(sid):
    _, blob, _, planes, _, _ = case(sid)
    want_p, want_v = oracle.OracleNet(blob).forward(planes)
    got_p, got_v = f32_outputs(sid)
    assert (got_p == want_p).all() and (got_v == want_v).all()


def test_bf16_many_planes_is_finite_and_merely_different_from_f32():
    p, v = run("A", "bf16")
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert not outputs_equal_ref_tol(p, v, *f32_outputs("A"))  # 8 significant bits: outside the bar the f16x2 tower holds


# ---------------------------------------------------------------------------------------- 6. limits


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16x2", "f16"])
def test_more_than_128_plane_words_is_still_refused(dtype):
    d = NetDesc(planes=129, board=3, moves=9, blocks=1, filters=8, vhc=4, phc=4)
    with pytest.raises(CattusHipError) as err:
        HipEvaluator(seeded_blob(d, 3), batch_size=4, plane_words=1, dtype=dtype, switches={})
    assert err.value.status == CATTUS_E_UNSUPPORTED and "128 plane words" in str(err.value)
