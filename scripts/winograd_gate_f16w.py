#!/usr/bin/env python3
"""CPU gate for dtype f16w: the single-term f16 tower in Winograd F(2x2, 3x3) form with an f32 stream, emulated operation for
operation as conv3x3_wino_f16_kernel computes it, beside the same emulation of today's direct f16 tower.

  f16w     stem      the direct f16 conv: planes 0 / 1, weights f16(w 2^s) (s per output channel: largest |w 2^s| in [2^10, 2^11)), f32
                     accumulation, fmaf(acc, 2^-s, bias), ReLU, capped at 16376, written as PLAIN F32
           weights   U = G g G^T in float64 on the host, one 2^s per output channel over its 16 frequencies, rounded to f32 and then ONCE to f16
           input     V = B^T d B in f32 on the f32 rows -- down the patch's columns, then along its rows, each pass as d0 - d2, d1 + d2,
                     d2 - d1, d1 - d3 (wino_f16_rule.h: wf16_bt) -- rounded ONCE to f16
           products  M[f] = sum over cin of U V: f16 x f16 products are exact in f32, the sums are f32 (torch's f32 matmul stands in for
                     the MFMA's f32 accumulation)
           output    Z = M A along a frequency row, Y = A^T Z, each as m0 + m1 + m2 and m1 - m2 - m3 left to right (wf16_at), in f32;
                     fmaf(Y, 2^-s, bias), + skip (f32), ReLU, capped at 16376, written as plain f32
  direct   every layer the direct f16 conv above, + skip (an f16 value), ReLU, clamped at 65504 and ROUNDED TO F16 -- the residual stream
           is rounded at every layer; the last layer writes f32 for the heads
  heads    f32 in both

Both are compared with the network's float64 run: max and rms |dlogit|, max |dvalue|.  Nets: the two reference-made fixtures
(tests/golden/chess_4x128.npz, chess_20x256.npz), 24 leaves of the seed-2 chess 20x256 bench network, and the three small shapes
tests/test_f16w_gpu.py runs (seed 7, 77 leaves of synth.random_chess_planes(77, 3)).  The seeded networks' stream shifts are all 0, so
none is emulated.

    python scripts/winograd_gate_f16w.py [--leaves20 24] > profiles/winograd_gate_f16w.json      # CPU only, a few minutes
"""
import argparse
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
from winograd_gate_a import G, fold, heads, pow2_scale  # noqa: E402

F16_MAX, WINO_ACT_MAX = 65504.0, 16376.0


def f16(x: torch.Tensor) -> torch.Tensor:
    """One rounding to f16, as an f32 tensor."""
    return x.to(torch.float16).to(torch.float32)


def conv_direct_f16(x, w, bias, skip, out):
    """The direct f16 kernel: x holds f16 values (0 / 1 planes at the stem).  out: "f16" (a layer of the direct tower), "f32" (its last
    layer) or "wino" (the f16w stem: f32, capped at WINO_ACT_MAX)."""
    sc = pow2_scale(w.double())
    wq = f16((w.double() * sc[:, None, None, None]).float())
    acc = F.conv2d(x, wq, padding=1)
    y = acc * (1.0 / sc).float()[None, :, None, None] + bias[None, :, None, None]  # the scale is a power of two: one rounding, as the fmaf
    if skip is not None:
        y = y + skip
    y = torch.relu(y)
    if out == "f16":
        return f16(y.clamp_max(F16_MAX))
    return y.clamp_max(WINO_ACT_MAX) if out == "wino" else y


def bt4(d0, d1, d2, d3):
    return d0 - d2, d1 + d2, d2 - d1, d1 - d3


def at2(m0, m1, m2, m3):
    return m0 + m1 + m2, m1 - m2 - m3


def conv_wino_f16(x, w, bias, skip):
    """One layer of conv3x3_wino_f16_kernel on plain f32 rows x (capped where they were written)."""
    B, C, S, _ = x.shape
    T = S // 2
    U = torch.einsum("ij,ocjk,lk->ocil", G, w.double(), G)  # [cout, cin, 4, 4], float64 on the host (wino_transform)
    sc = pow2_scale(U)
    Uq = f16((U * sc[:, None, None, None]).float())  # wino_u_f16: f16(f32(U 2^s))
    tiles = F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)  # [B, C, T, T, 4 rows, 4 columns]
    rows = bt4(*[tiles[..., i, :] for i in range(4)])  # down the columns: row i of B^T d, each [B, C, T, T, 4]
    V = torch.stack([torch.stack(bt4(*[r[..., j] for j in range(4)]), dim=-1) for r in rows], dim=-2)  # along the rows: [.., i, l]
    Vq = f16(V)  # |V| <= 4 * 16376 = 65504: no clamp
    M = torch.einsum("ocil,bctuil->botuil", Uq, Vq)  # f32 accumulation over cin
    Z = torch.stack(at2(*[M[..., l] for l in range(4)]), dim=-1)  # [B, O, T, T, i, c']
    Y = torch.stack(at2(*[Z[..., i, :] for i in range(4)]), dim=-2)  # [B, O, T, T, r', c']
    Y = Y.permute(0, 1, 2, 4, 3, 5).reshape(B, -1, S, S)
    y = Y * (1.0 / sc).float()[None, :, None, None] + bias[None, :, None, None]
    if skip is not None:
        y = y + skip
    return torch.relu(y).clamp_max(WINO_ACT_MAX)


def tower_direct(net, x):
    nb = len(net._residual_blocks)
    w, b = fold(net._conv1._conv.weight, net._conv1._bn)
    a = conv_direct_f16(x, w, b, None, "f16" if nb else "f32")
    for i, blk in enumerate(net._residual_blocks):
        w1, b1 = fold(blk._conv1.weight, blk._bn1)
        w2, b2 = fold(blk._conv2.weight, blk._bn2)
        t = conv_direct_f16(a, w1, b1, None, "f16")
        a = conv_direct_f16(t, w2, b2, a, "f32" if i == nb - 1 else "f16")
    return a


def tower_f16w(net, x):
    w, b = fold(net._conv1._conv.weight, net._conv1._bn)
    a = conv_direct_f16(x, w, b, None, "wino")
    for blk in net._residual_blocks:
        w1, b1 = fold(blk._conv1.weight, blk._bn1)
        w2, b2 = fold(blk._conv2.weight, blk._bn2)
        t = conv_wino_f16(a, w1, b1, None)
        a = conv_wino_f16(t, w2, b2, a)
    return a


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, dtype=np.float64)))))


def run(name, blob, planes):
    net = PolicyValueNet.from_blob(blob)
    d = net.desc
    bits = np.unpackbits(planes.view(np.uint8).reshape(len(planes), d.planes, -1), axis=-1, bitorder="little")
    x = torch.from_numpy(bits[..., : d.hw].reshape(len(planes), d.planes, d.board, d.board).astype(np.float32))
    out = {"net": name, "leaves": len(planes)}
    with torch.no_grad():
        p64, v64 = net.double()(x.double())
        p64, v64 = p64.numpy(), v64.flatten().numpy()
        net = net.float()
        for form, tower in (("f16_direct", tower_direct), ("f16w", tower_f16w)):
            p, v = heads(net, tower(net, x))
            p, v = p.numpy(), v.numpy()
            out[form] = dict(max_dp_vs_f64=float(np.abs(p - p64).max()), rms_dp_vs_f64=rms(p - p64), max_dv_vs_f64=float(np.abs(v - v64).max()))
    out["f16w_over_direct"] = {k: out["f16w"][k] / out["f16_direct"][k] for k in out["f16w"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves20", type=int, default=24, help="leaves of the seeded chess 20x256 batch (the bench weights): 24 .. 48")
    args = ap.parse_args()
    torch.manual_seed(0)
    from helpers import blob_for

    results = []
    for name in ("chess_4x128", "chess_20x256"):
        d, blob, z = blob_for(name)
        results.append(run(name, blob, z["planes"]))
        print(json.dumps(results[-1]), file=sys.stderr, flush=True)
    d20 = NetDesc(**CHESS, blocks=20, filters=256, vhc=8, phc=8)
    results.append(run("chess20x256 bench weights (seed 2)", seeded_blob(d20, 2), synth.random_chess_planes(args.leaves20, 2)))
    print(json.dumps(results[-1]), file=sys.stderr, flush=True)
    for blocks, filters in ((1, 128), (2, 192), (2, 256)):
        ds = NetDesc(**CHESS, blocks=blocks, filters=filters, vhc=8, phc=8)
        results.append(run("chess %dx%d (seed 7)" % (blocks, filters), seeded_blob(ds, 7), synth.random_chess_planes(77, 3)))
        print(json.dumps(results[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"what": "f16w (single-term f16 Winograd F(2x2,3x3), f32 stream) and the direct f16 tower, emulated on the CPU, against float64",
                      "results": results}, indent=1))


if __name__ == "__main__":
    main()
