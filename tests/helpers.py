"""Shared helpers for the parity tests."""

from __future__ import annotations

import math
from pathlib import Path

import numpy as np

from cattus_amd.weights import BN_EPS, NetDesc, seeded_blob

GOLDEN = Path(__file__).resolve().parent / "golden"

# The reference's own "same net, different runtime" tolerance
# (training/tests/test_net_output.py:28-33): value rel 1e-5 / abs 1e-6, policy rtol 1e-3 / atol 1e-6.
REF_POLICY_RTOL, REF_POLICY_ATOL = 1e-3, 1e-6
REF_VALUE_REL, REF_VALUE_ABS = 1e-5, 1e-6


def load_golden(name: str):
    z = np.load(GOLDEN / f"{name}.npz")
    d = NetDesc(*[int(x) for x in z["desc"]])
    return d, int(z["seed"]), z


def golden_names():
    return sorted(p.stem for p in GOLDEN.glob("*.npz"))


def outputs_equal_ref_tol(policy, value, policy_ref, value_ref) -> bool:
    """is_outputs_equals of training/tests/test_net_output.py:28-33, per position."""
    ok = True
    for b in range(len(value_ref)):
        ok &= math.isclose(float(value[b]), float(value_ref[b]), rel_tol=REF_VALUE_REL, abs_tol=REF_VALUE_ABS)
        ok &= bool(np.isclose(policy[b], policy_ref[b], rtol=REF_POLICY_RTOL, atol=REF_POLICY_ATOL).all())
    return ok


def blob_for(name: str):
    d, seed, z = load_golden(name)
    return d, seeded_blob(d, seed), z


def planes_to_f64(planes: np.ndarray, board: int) -> np.ndarray:
    """uint64 bitboards [n, C, W64] (bit h*S+w of a plane in bit i & 63 of word i >> 6) -> float64 [n, C, S, S] of 0 / 1."""
    planes = np.asarray(planes, dtype=np.uint64)
    hw = board * board
    i = np.arange(hw)
    bits = (planes[:, :, i >> 6] >> (i & 63).astype(np.uint64)) & np.uint64(1)
    return bits.astype(np.float64).reshape(len(planes), planes.shape[1], board, board)


def forward_f64(desc: NetDesc, tensors: dict, planes: np.ndarray):
    """The network in float64 on the CPU, built from the raw tensors (the seeded_tensors / pack_tensors input) and not from a
    blob, so that a packing or BatchNorm-folding error of the blob path cannot cancel out.  Returns (policy, value) as float64."""
    import torch

    from cattus_amd.torch_model import PolicyValueNet

    net = PolicyValueNet(desc).to(torch.float64)
    sd = net.state_dict()
    for k in sd:
        if k.endswith("num_batches_tracked"):
            continue
        sd[k] = torch.from_numpy(np.asarray(tensors[k], dtype=np.float64).reshape(tuple(sd[k].shape)))
    net.load_state_dict(sd, strict=True)
    net.eval()
    with torch.no_grad():
        p, v = net(torch.from_numpy(planes_to_f64(planes, desc.board)))
    return p.numpy(), v.numpy().reshape(-1)


# the single-term f16 tower (11 significant bits) against the bf16 one (8): its error on the same leaves is at most a quarter
F16_OVER_BF16_MAX = 0.25


def check_f16_against_f64(label, bound, f16_out, bf16_out, f64_out):
    """The f16 tower's bars on one set of leaves, each a (policy, value) pair: within ``bound`` (max |dlogit|, max |dvalue|) of
    the float64 network, at most F16_OVER_BF16_MAX of the bf16 tower's error on the same leaves, and the bf16 outputs fail
    ``bound`` (a bound that passes bf16 would not notice an f16 tower that lost its extra bits).  Prints the errors first."""
    ep, ev = float(np.abs(f16_out[0] - f64_out[0]).max()), float(np.abs(f16_out[1] - f64_out[1]).max())
    bp, bv = float(np.abs(bf16_out[0] - f64_out[0]).max()), float(np.abs(bf16_out[1] - f64_out[1]).max())
    print("%s: f16 vs f64 max |dlogit| %.3g |dvalue| %.3g; bf16 vs f64 %.3g %.3g" % (label, ep, ev, bp, bv))
    assert np.isfinite(f16_out[0]).all() and np.isfinite(f16_out[1]).all()
    assert ep <= bound[0] and ev <= bound[1], (label, ep, ev, bound)
    assert ep <= F16_OVER_BF16_MAX * bp and ev <= F16_OVER_BF16_MAX * bv, (label, ep, ev, bp, bv)
    assert bp > bound[0] and bv > bound[1], ("the f16 bound passes the bf16 tower", label, bp, bv, bound)


def stream_twin(desc: NetDesc, tensors: dict, c: float) -> dict:
    """The tensors of a network that computes the same function as ``tensors`` with its residual stream (the stem output and
    every block's output) multiplied by ``c``, a power of two: stem BatchNorm and every block's _bn2 gamma, beta x c; every
    block's _bn1 and the two head BatchNorms (no affine parameters: they read the stream) running_mean x c and running_var ->
    c^2 (var + eps) - eps.  Computed in float64, returned as float32 (the blob is f32), so the new statistics are rounded: each
    twin is its own network, to be compared with its own forward_f64.  A variance that comes out <= 0 raises (with the seeded
    var >= 0.5 this limits c to >= 2^-7)."""
    c = float(c)
    if not (c > 0 and math.frexp(c)[0] == 0.5):
        raise ValueError(f"stream_twin: c = {c} is not a power of two")
    out = dict(tensors)

    def f64(k):
        return np.asarray(tensors[k], dtype=np.float64)

    affine = ["_conv1._bn."] + [f"_residual_blocks.{i}._bn2." for i in range(desc.blocks)]
    for p in affine:
        out[p + "weight"] = (f64(p + "weight") * c).astype(np.float32)
        out[p + "bias"] = (f64(p + "bias") * c).astype(np.float32)
    readers = [f"_residual_blocks.{i}._bn1." for i in range(desc.blocks)] + ["_value_head.0._bn.", "_policy_head.0._bn."]
    for p in readers:
        var = c * c * (f64(p + "running_var") + BN_EPS) - BN_EPS
        if not (var > 0).all():
            raise ValueError(f"stream_twin: c = {c} gives {p}running_var <= 0")
        out[p + "running_mean"] = (f64(p + "running_mean") * c).astype(np.float32)
        out[p + "running_var"] = var.astype(np.float32)
    return out


F32_MIN_NORMAL, F32_MAX = 2.0**-126, float(np.finfo(np.float32).max)


def channel_twin(desc: NetDesc, tensors: dict, exponents) -> dict:
    """The tensors of a network that computes the same function as ``tensors`` with channel k of its residual stream multiplied
    by c_k = 2^exponents[k] (integers, one per filter): gamma, beta of the stem BatchNorm and of every block's _bn2 x c_k; the
    weights that read channel k -- input channel k of every block's _conv1 and of both head convs -- / c_k.  (ReLU commutes with
    c_k > 0, the skip adds channel k to channel k, and _bn1 and the head BatchNorms normalise what the convs write, which does not
    move.)  Every product is by a power of two and so exact: unlike stream_twin's, this twin's float64 run equals the base
    network's to the bit, and so do the f32 outputs of anything that folds and sums in the oracle's order.  Computed in float64,
    returned as float32; a wrong number of exponents, or a product that leaves the f32 normal range (and would round), raises."""
    e = np.asarray(exponents)
    if e.shape != (desc.filters,) or not np.issubdtype(e.dtype, np.integer):
        raise ValueError(f"channel_twin: want {desc.filters} integer exponents, got {e.dtype} {e.shape}")
    c = np.ldexp(1.0, e.astype(np.int64))
    out = dict(tensors)

    def scaled(k, factor):
        x = np.asarray(tensors[k], dtype=np.float64) * factor
        a = np.abs(x[x != 0])
        if a.size and not (a.min() >= F32_MIN_NORMAL and a.max() <= F32_MAX):
            raise ValueError(f"channel_twin: {k} leaves the f32 normal range")
        out[k] = x.astype(np.float32)

    for p in ["_conv1._bn."] + [f"_residual_blocks.{i}._bn2." for i in range(desc.blocks)]:
        scaled(p + "weight", c)
        scaled(p + "bias", c)
    readers = [f"_residual_blocks.{i}._conv1.weight" for i in range(desc.blocks)] + ["_value_head.0._conv.weight", "_policy_head.0._conv.weight"]
    for k in readers:
        scaled(k, (1.0 / c).reshape(1, -1, 1, 1))
    return out


def hostile_tensors(desc: NetDesc, tensors: dict) -> dict:
    """A *different* network, of statistics that seeded_tensors never draws, to be compared with its own forward_f64: on the stem
    BatchNorm and every block's _bn2, gamma's sign flipped where k % 3 == 1 and gamma = beta = 0 where k % 16 == 5 (dead stream
    channels, unless a later _bn2 revives them -- none does: all are zeroed alike); in every block's _conv1, the weights of output
    channels k % 16 == 9 zeroed (an all-zero folded row: the middle activation of that channel is relu of its bias alone)."""
    out = dict(tensors)
    k = np.arange(desc.filters)
    for p in ["_conv1._bn."] + [f"_residual_blocks.{i}._bn2." for i in range(desc.blocks)]:
        g, b = np.array(tensors[p + "weight"], dtype=np.float32), np.array(tensors[p + "bias"], dtype=np.float32)
        g[k % 3 == 1] *= -1
        g[k % 16 == 5] = 0
        b[k % 16 == 5] = 0
        out[p + "weight"], out[p + "bias"] = g, b
    for i in range(desc.blocks):
        w = np.array(tensors[f"_residual_blocks.{i}._conv1.weight"], dtype=np.float32)
        w[k % 16 == 9] = 0
        out[f"_residual_blocks.{i}._conv1.weight"] = w
    return out


# channel_twin exponents by filter count F: channels of a stream that differ in scale by 2^8 or more
CHANNEL_PATTERNS = {
    "Q8": lambda F: np.where(np.arange(F) % 4 == 1, -8, 0),  # every fourth channel small beside a unit median
    "W8": lambda F: np.random.default_rng(3).integers(-8, 9, F),  # every scale from 2^-8 to 2^8
    "M8": lambda F: np.where(np.arange(F) % 4 == 1, 0, -8),  # a small median, every fourth channel 2^8 above it
    "S8": lambda F: (7 * np.arange(F)) % 17 - 8,  # an even spread over 2^-8 .. 2^8
}
