#!/usr/bin/env python3
"""CPU gate for dtype f16r: the direct single-term f16 tower with an f32 residual stream, emulated operation for operation as
conv3x3_f16r_kernel computes it (cattus_amd/csrc/f16r_rule.h), beside the emulations of today's direct f16 tower and of f16w that
scripts/winograd_gate_f16w.py holds (imported, not restated).

  f16r     stem      the direct f16 conv: planes 0 / 1, weights f16(w 2^s), f32 accumulation, y = relu(fmaf(acc, 2^-s, bias));
                     the stream S = y in f32, not clamped; the operand copy A = f16(min(y, 65504))
           conv1     reads A, writes the middle activation M = f16(min(relu(fmaf(acc, 2^-s, bias)), 65504)): the direct tower's layer
           conv2     reads M, y = relu(fmaf(acc, 2^-s, bias) + S) in f32; S = y, A = f16(min(y, 65504))
           the last layer leaves S alone for the heads
  direct   every layer rounds its output, the stream included, to f16 (winograd_gate_f16w.tower_direct)
  f16w     winograd_gate_f16w.tower_f16w, where that form covers the shape (8x8 board, >= 128 filters, a block)
  heads    f32 in all three

All are compared with the network's float64 run: rms and max |dlogit|, rms and max |dvalue|.  Nets: the reference-made fixtures
chess_4x128, chess_20x256, hex7_6x64 and chess_7x16 (tests/golden), 24 leaves of the seed-2 chess 20x256 bench network, and chess 6x64,
2x256 and 1x128 of seed 7 on the 77 leaves of synth.random_chess_planes(77, 3).  The seeded networks' stream shifts are all 0, so none is
emulated.  The gate: on the reference-made fixtures the new tower's rms |dlogit| is below 1.0x the direct tower's.

    python scripts/gate_f16r.py > profiles/gate_f16r.json      # CPU only, a few minutes
"""
import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))

from cattus_amd import synth  # noqa: E402
from cattus_amd.torch_model import PolicyValueNet  # noqa: E402
from cattus_amd.weights import CHESS, NetDesc, seeded_blob  # noqa: E402
from winograd_gate_a import fold, heads, pow2_scale  # noqa: E402
from winograd_gate_f16w import F16_MAX, conv_direct_f16, f16, rms, tower_direct, tower_f16w  # noqa: E402


def conv_stream(x, w, bias, skip):
    """A stream layer of conv3x3_f16r_kernel: conv_direct_f16's sums, the skip and the result in f32 -> (S, A)."""
    sc = pow2_scale(w.double())
    wq = f16((w.double() * sc[:, None, None, None]).float())
    acc = F.conv2d(x, wq, padding=1)
    y = acc * (1.0 / sc).float()[None, :, None, None] + bias[None, :, None, None]  # the scale is a power of two: one rounding, as the fmaf
    if skip is not None:
        y = y + skip
    y = torch.relu(y)
    return y, f16(y.clamp_max(F16_MAX))


def tower_f16r(net, x):
    w, b = fold(net._conv1._conv.weight, net._conv1._bn)
    s, a = conv_stream(x, w, b, None)
    for blk in net._residual_blocks:
        w1, b1 = fold(blk._conv1.weight, blk._bn1)
        w2, b2 = fold(blk._conv2.weight, blk._bn2)
        m = conv_direct_f16(a, w1, b1, None, "f16")
        s, a = conv_stream(m, w2, b2, s)
    return s


def run(name, blob, planes):
    net = PolicyValueNet.from_blob(blob)
    d = net.desc
    bits = np.unpackbits(planes.view(np.uint8).reshape(len(planes), d.planes, -1), axis=-1, bitorder="little")
    x = torch.from_numpy(bits[..., : d.hw].reshape(len(planes), d.planes, d.board, d.board).astype(np.float32))
    out = {"net": name, "leaves": len(planes)}
    towers = [("f16_direct", tower_direct), ("f16r", tower_f16r)]
    if d.board == 8 and d.blocks > 0 and d.filters >= 128 and d.filters % 64 == 0:
        towers.append(("f16w", tower_f16w))
    with torch.no_grad():
        p64, v64 = net.double()(x.double())
        p64, v64 = p64.numpy(), v64.flatten().numpy()
        net = net.float()
        for form, tower in towers:
            p, v = heads(net, tower(net, x))
            p, v = p.numpy(), v.numpy().reshape(-1)
            out[form] = dict(rms_dp_vs_f64=rms(p - p64), max_dp_vs_f64=float(np.abs(p - p64).max()), rms_dv_vs_f64=rms(v - v64),
                             max_dv_vs_f64=float(np.abs(v - v64).max()))
    for form, _ in towers[1:]:
        out[form + "_over_direct"] = {k: out[form][k] / out["f16_direct"][k] for k in out[form]}
    return out


def main():
    torch.manual_seed(0)
    from helpers import blob_for

    results = []

    def add(name, blob, planes):
        results.append(run(name, blob, planes))
        print(json.dumps(results[-1]), file=sys.stderr, flush=True)

    for name in ("chess_4x128", "chess_20x256", "hex7_6x64", "chess_7x16"):
        d, blob, z = blob_for(name)
        add(name, blob, z["planes"])
    add("chess20x256 bench weights (seed 2)", seeded_blob(NetDesc(**CHESS, blocks=20, filters=256, vhc=8, phc=8), 2), synth.random_chess_planes(24, 2))
    for blocks, filters in ((6, 64), (2, 256), (1, 128)):
        ds = NetDesc(**CHESS, blocks=blocks, filters=filters, vhc=8, phc=8)
        add("chess %dx%d (seed 7)" % (blocks, filters), seeded_blob(ds, 7), synth.random_chess_planes(77, 3))
    made = [r for r in results if r["net"] in ("chess_4x128", "chess_20x256", "hex7_6x64", "chess_7x16")]
    gate = all(r["f16r_over_direct"]["rms_dp_vs_f64"] < 1.0 for r in made)
    print(json.dumps({"what": "f16r (direct single-term f16, f32 residual stream), the direct f16 tower and f16w, emulated on the CPU, against float64",
                      "gate": "rms |dlogit| of f16r below 1.0x the direct f16 tower's on every reference-made fixture",
                      "gate_passed": gate, "results": results}, indent=1))
    return 0 if gate else 1


if __name__ == "__main__":
    sys.exit(main())
