"""The float64 reference network of the tests (helpers.forward_f64) against the reference's own float64 outputs.

forward_f64 builds the network from the raw tensors (not from a weight blob), so the f16 tower's tests
(test_f16_tower_gpu.py) compare the HIP evaluator with something that shares none of its weight path.  Here it is pinned to
every golden fixture's policy_f64 / value_f64 (the reference network run in float64 on the fixture's weights and positions)."""

import numpy as np
import pytest

from cattus_amd.weights import seeded_tensors

from helpers import forward_f64, golden_names, load_golden, planes_to_f64


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
