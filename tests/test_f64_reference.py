"""The float64 reference network of the tests (helpers.forward_f64) against the reference's own float64 outputs.

forward_f64 builds the network from the raw tensors (not from a weight blob), so the f16 tower's tests
(test_f16_tower_gpu.py) compare the HIP evaluator with something that shares none of its weight path.  Here it is pinned to
every golden fixture's policy_f64 / value_f64 (the reference network run in float64 on the fixture's weights and positions).

helpers.stream_twin (the same network with its residual stream x c) is pinned here too: in float64 every twin computes the base
network's function, and the CPU oracle's exact-f32 arithmetic holds an f32-grade bound on every twin, with no cliff at small c --
the yardstick that the f16x2 tower is held to by stream scale in test_split_range_gpu.py.

helpers.channel_twin (stream channel k x 2^e_k, its readers' weights / 2^e_k) is exact, so it is pinned with no tolerance at all:
float64 run and f32 oracle of every twin equal the base network's to the bit.  helpers.hostile_tensors (negative gammas, dead
stream channels, all-zero conv rows) is another network; the oracle holds the same f32-grade bound on it, on the leaves that
test_channel_scale_gpu.py holds the f16x2 tower to."""

import numpy as np
import pytest

from cattus_amd.weights import pack_tensors, seeded_tensors
from oracle import oracle

from helpers import CHANNEL_PATTERNS, channel_twin, forward_f64, golden_names, hostile_tensors, load_golden, planes_to_f64, stream_twin

# every power of two that stream_twin allows on a seeded network (var >= 0.5: c >= 2^-7) up to a stream in the hundreds
TWIN_SCALES = [2.0**k for k in range(-7, 9)]
TWIN_NETS = ["hex7_6x64", "chess_2x64", "ttt_5x8"]
# max |dlogit|, max |dvalue| of a twin's float64 run against the base network's: 2x the measured 1.31e-8 / 1.96e-9 (the twins'
# f32-rounded BatchNorm statistics; 0 at c = 1)
TWIN_VS_BASE = (2.7e-8, 4.0e-9)
# the CPU oracle (exact f32) against each twin's own float64 run: 2x the largest measured over TWIN_NETS and every c, 5.11e-7 /
# 8.67e-8 (3.17e-7 / 8.58e-8 for hex7_6x64 at c = 1)
ORACLE_VS_TWIN_F64 = (1.1e-6, 1.8e-7)


@pytest.mark.parametrize("name", golden_names())
def test_forward_f64_reproduces_the_reference_float64_run(name):
    d, seed, z = load_golden(name)
    assert (planes_to_f64(z["planes"], d.board) == z["input_tensor"]).all()
    p, v = forward_f64(d, seeded_tensors(d, seed), z["planes"])
    assert p.dtype == np.float64 and v.dtype == np.float64
    assert p.shape == z["policy_f64"].shape and v.shape == z["value_f64"].shape
    assert np.abs(p - z["policy_f64"]).max() <= 1e-12, np.abs(p - z["policy_f64"]).max()
    assert np.abs(v - z["value_f64"]).max() <= 1e-12, np.abs(v - z["value_f64"]).max()


def test_forward_f64_sees_a_perturbed_tensor():
    """The helper reads the tensors it is given: one BatchNorm statistic moved moves the outputs (no cached or blob-derived weights)."""
    d, seed, z = load_golden("hex7_6x64")
    t = seeded_tensors(d, seed)
    t["_residual_blocks.3._bn1.running_var"] = t["_residual_blocks.3._bn1.running_var"].copy()
    t["_residual_blocks.3._bn1.running_var"][5] *= 2
    p, v = forward_f64(d, t, z["planes"])
    assert np.abs(p - z["policy_f64"]).max() > 1e-6


@pytest.mark.parametrize("name", TWIN_NETS)
def test_stream_twins_compute_the_base_network_in_float64(name):
    d, seed, z = load_golden(name)
    t = seeded_tensors(d, seed)
    p0, v0 = forward_f64(d, t, z["planes"])
    for c in TWIN_SCALES:
        tw = stream_twin(d, t, c)
        assert tw["_conv1._bn.weight"][0] == np.float32(c) * t["_conv1._bn.weight"][0]  # the stream did move
        p, v = forward_f64(d, tw, z["planes"])
        dp, dv = float(np.abs(p - p0).max()), float(np.abs(v - v0).max())
        assert dp <= TWIN_VS_BASE[0] and dv <= TWIN_VS_BASE[1], (c, dp, dv)
        if c == 1.0:
            assert dp == 0 and dv == 0


def test_stream_twin_refuses_what_it_cannot_build():
    d, seed, _ = load_golden("hex7_6x64")
    t = seeded_tensors(d, seed)
    with pytest.raises(ValueError):
        stream_twin(d, t, 2.0**-8)  # c^2 (0.5 + eps) < eps: a negative variance
    with pytest.raises(ValueError):
        stream_twin(d, t, 0.75)


@pytest.mark.parametrize("name", TWIN_NETS)
def test_the_f32_oracle_holds_its_bound_on_every_stream_twin(name):
    """The exact-f32 contract has no cliff in the stream's scale: the oracle is within ORACLE_VS_TWIN_F64 of each twin's float64
    run at every c from 2^-7 to 2^8."""
    d, seed, z = load_golden(name)
    t = seeded_tensors(d, seed)
    for c in TWIN_SCALES:
        tw = stream_twin(d, t, c)
        p64, v64 = forward_f64(d, tw, z["planes"])
        p, v = oracle.OracleNet(pack_tensors(d, tw)).forward(z["planes"])
        dp, dv = float(np.abs(p - p64).max()), float(np.abs(v - v64).max())
        assert dp <= ORACLE_VS_TWIN_F64[0] and dv <= ORACLE_VS_TWIN_F64[1], (c, dp, dv)


@pytest.mark.parametrize("name", TWIN_NETS)
def test_channel_twins_are_the_base_network_to_the_bit(name):
    """Every product of channel_twin is by a power of two: forward_f64 of a twin differs from the base network's by 0, and the
    oracle's f32 outputs -- folding included -- are the same bits."""
    d, seed, z = load_golden(name)
    t = seeded_tensors(d, seed)
    p0, v0 = forward_f64(d, t, z["planes"])
    o0 = oracle.OracleNet(pack_tensors(d, t)).forward(z["planes"])
    for pattern in ("Q8", "W8", "M8", "S8"):
        e = CHANNEL_PATTERNS[pattern](d.filters)
        tw = channel_twin(d, t, e)
        k = int(np.argmin(e))
        c = np.float32(2.0 ** int(e[k]))
        assert -8 <= e[k] <= -7 and e.max() <= 8 and tw["_conv1._bn.weight"][k] == c * t["_conv1._bn.weight"][k]  # the channel did move
        assert (tw["_policy_head.0._conv.weight"][:, k] * c == t["_policy_head.0._conv.weight"][:, k]).all()
        p, v = forward_f64(d, tw, z["planes"])
        assert np.abs(p - p0).max() == 0 and np.abs(v - v0).max() == 0, pattern
        o = oracle.OracleNet(pack_tensors(d, tw)).forward(z["planes"])
        assert o[0].tobytes() == o0[0].tobytes() and o[1].tobytes() == o0[1].tobytes(), pattern


def test_channel_twin_refuses_what_it_cannot_build():
    d, seed, _ = load_golden("hex7_6x64")
    t = seeded_tensors(d, seed)
    with pytest.raises(ValueError):
        channel_twin(d, t, np.zeros(d.filters - 1, dtype=int))  # one exponent short
    with pytest.raises(ValueError):
        channel_twin(d, t, np.zeros(d.filters))  # not integers
    with pytest.raises(ValueError):
        channel_twin(d, t, np.full(d.filters, -130))  # gamma 2^-130: an f32 subnormal
    with pytest.raises(ValueError):
        channel_twin(d, t, np.full(d.filters, 130))  # gamma 2^130: past the f32 range
    same = channel_twin(d, t, np.zeros(d.filters, dtype=int))
    assert all((same[k] == t[k]).all() and same[k].dtype == np.float32 for k in t)


def test_hostile_tensors_are_what_they_say():
    d, seed, _ = load_golden("hex7_6x64")
    t = seeded_tensors(d, seed)
    h = hostile_tensors(d, t)
    for p in ["_conv1._bn."] + [f"_residual_blocks.{i}._bn2." for i in range(d.blocks)]:
        g, b, g0, b0 = h[p + "weight"], h[p + "bias"], t[p + "weight"], t[p + "bias"]
        k = np.arange(d.filters)
        flipped, dead = (k % 3 == 1) & (k % 16 != 5), k % 16 == 5
        assert flipped.sum() > d.filters // 4 and dead.sum() == d.filters // 16
        assert (g[flipped] == -g0[flipped]).all() and (g[flipped] < 0).all() and (g[dead] == 0).all() and (b[dead] == 0).all()
        assert (g[~flipped & ~dead] == g0[~flipped & ~dead]).all() and (b[~dead] == b0[~dead]).all()
    for i in range(d.blocks):
        w = h[f"_residual_blocks.{i}._conv1.weight"]
        assert (w[9::16] == 0).all() and (w[8::16] != 0).any()
    assert (t["_conv1._bn.weight"] > 0).all()  # the input is left alone


def hostile_cases():
    from test_split_range_gpu import CASES

    return sorted({(c[1], c[2]) for c in CASES})


@pytest.mark.parametrize("net,n", hostile_cases(), ids=[f"{a}_n{b}" for a, b in hostile_cases()])
def test_the_f32_oracle_holds_its_bound_on_the_hostile_networks(net, n):
    """What lets test_channel_scale_gpu.py hold f16x2 on the hostile networks to the bars it is held to elsewhere: exact f32
    is as close to float64 on them as on the seeded ones, on every leaf that test samples (measured: at most 9.1e-7 / 5.9e-8)."""
    from test_f16_tower_gpu import random_planes
    from test_split_range_gpu import SEED, desc_of, sample

    d, words = desc_of(net)
    h = hostile_tensors(d, seeded_tensors(d, SEED))
    planes = random_planes(d, words, n, 5)[sample(n)]
    p64, v64 = forward_f64(d, h, planes)
    p, v = oracle.OracleNet(pack_tensors(d, h)).forward(planes)
    dp, dv = float(np.abs(p - p64).max()), float(np.abs(v - v64).max())
    print("%s n=%d hostile: oracle vs f64 max |dlogit| %.3g |dvalue| %.3g" % (net, n, dp, dv))
    assert dp <= ORACLE_VS_TWIN_F64[0] and dv <= ORACLE_VS_TWIN_F64[1], (dp, dv)
