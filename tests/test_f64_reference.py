"""The float64 reference network of the tests (helpers.forward_f64) against the reference's own float64 outputs.

forward_f64 builds the network from the raw tensors (not from a weight blob), so the f16 tower's tests
(test_f16_tower_gpu.py) compare the HIP evaluator with something that shares none of its weight path.  Here it is pinned to
every golden fixture's policy_f64 / value_f64 (the reference network run in float64 on the fixture's weights and positions).

helpers.stream_twin (the same network with its residual stream x c) is pinned here too: in float64 every twin computes the base
network's function, and the CPU oracle's exact-f32 arithmetic holds an f32-grade bound on every twin, with no cliff at small c --
the yardstick that the f16x2 tower is held to by stream scale in test_split_range_gpu.py."""

import numpy as np
import pytest

from cattus_amd.weights import pack_tensors, seeded_tensors
from oracle import oracle

from helpers import forward_f64, golden_names, load_golden, planes_to_f64, stream_twin

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
