#!/usr/bin/env python3
"""CPU gate for dtype f32w: the f32-operand tower in Winograd F(2x2, 3x3) form, emulated in f32 in the order of wino_f32_rule.h, beside
the same emulation of the direct f32 tower (dtype f32).

  f32w     stem      the direct f32 conv on the 0 / 1 planes: f32 sums, + bias, ReLU, plain f32 rows
           weights   U = G g G^T in float64 on the host (wino_transform), rounded ONCE to f32; no per-channel scale
           input     V = B^T d B in f32 on the f32 rows -- down the patch's columns, then along its rows, each pass as d0 - d2, d1 + d2,
                     d2 - d1, d1 - d3 (wf32_bt)
           products  M[f] = sum over cin of U V in f32 (torch's f32 matmul stands in for the MFMA's in-order fmaf chain: numpy and torch
                     have no fmaf, so the emulation does not claim the device's bits -- tests/wino_f32_layer_ref.cpp does)
           output    Z = M A along a frequency row, Y = A^T Z, each as m0 + m1 + m2 and m1 - m2 - m3 left to right (wf32_at), in f32;
                     Y + bias, + skip, ReLU, plain f32 rows
  direct   every layer the direct f32 conv above, + skip, ReLU
  heads    f32 in both

Both are compared with the float64 outputs the reference-made fixtures store (tests/golden/chess_4x128.npz, chess_20x256.npz: max and
rms |dlogit|, max and rms |dvalue|) and held to the reference's cross-runtime bar against the fixtures' reference outputs (policy rtol
1e-3 / atol 1e-6, value rel 1e-5 / abs 1e-6).  PASS: on both fixtures the emulated f32w tower is inside that bar and its rms |dlogit|
against float64 is at most 2x the emulated direct f32 tower's -- the margin tests/test_splitk_gpu.py grants another f32 summation order
of the same operands.

    python scripts/winograd_gate_f32w.py > profiles/winograd_gate_f32w.json      # CPU only, about a minute
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

from cattus_amd.torch_model import PolicyValueNet  # noqa: E402
from winograd_gate_a import G, fold, heads, ref_tol_ok  # noqa: E402
from winograd_gate_f16w import at2, bt4, rms  # noqa: E402

MARGIN = 2.0


def conv_direct_f32(x, w, bias, skip):
    y = F.conv2d(x, w, padding=1) + bias[None, :, None, None]
    if skip is not None:
        y = y + skip
    return torch.relu(y)


def conv_wino_f32(x, w, bias, skip):
    """One layer of conv3x3_wino_f32_kernel on plain f32 rows x."""
    B, C, S, _ = x.shape
    U = torch.einsum("ij,ocjk,lk->ocil", G, w.double(), G).float()  # wino_u_f32: f32(G g G^T), [cout, cin, 4, 4]
    tiles = F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)  # [B, C, T, T, 4 rows, 4 columns]
    rows = bt4(*[tiles[..., i, :] for i in range(4)])  # down the columns: row i of B^T d, each [B, C, T, T, 4]
    V = torch.stack([torch.stack(bt4(*[r[..., j] for j in range(4)]), dim=-1) for r in rows], dim=-2)  # along the rows: [.., i, l]
    M = torch.einsum("ocil,bctuil->botuil", U, V)  # f32 accumulation over cin
    Z = torch.stack(at2(*[M[..., l] for l in range(4)]), dim=-1)  # [B, O, T, T, i, c']
    Y = torch.stack(at2(*[Z[..., i, :] for i in range(4)]), dim=-2)  # [B, O, T, T, r', c']
    y = Y.permute(0, 1, 2, 4, 3, 5).reshape(B, -1, S, S) + bias[None, :, None, None]
    if skip is not None:
        y = y + skip
    return torch.relu(y)


def tower(net, x, layer):
    w, b = fold(net._conv1._conv.weight, net._conv1._bn)
    a = conv_direct_f32(x, w, b, None)
    for blk in net._residual_blocks:
        w1, b1 = fold(blk._conv1.weight, blk._bn1)
        w2, b2 = fold(blk._conv2.weight, blk._bn2)
        a = layer(layer(a, w1, b1, None), w2, b2, a)
    return a


def run(name, blob, z):
    net = PolicyValueNet.from_blob(blob).float()
    d = net.desc
    planes = z["planes"]
    bits = np.unpackbits(planes.view(np.uint8).reshape(len(planes), d.planes, -1), axis=-1, bitorder="little")
    x = torch.from_numpy(bits[..., : d.hw].reshape(len(planes), d.planes, d.board, d.board).astype(np.float32))
    p64, v64 = z["policy_f64"], z["value_f64"].reshape(-1)
    out = {"net": name, "leaves": len(planes)}
    with torch.no_grad():
        for form, layer in (("f32_direct", conv_direct_f32), ("f32w", conv_wino_f32)):
            p, v = heads(net, tower(net, x, layer))
            p, v = p.numpy(), v.numpy()
            out[form] = dict(max_dp_vs_f64=float(np.abs(p - p64).max()), rms_dp_vs_f64=rms(p - p64), max_dv_vs_f64=float(np.abs(v - v64).max()),
                             rms_dv_vs_f64=rms(v - v64), inside_reference_bar=ref_tol_ok(p, v, z["policy"], z["value"].reshape(-1)))
    out["f32w_over_direct"] = {k: out["f32w"][k] / out["f32_direct"][k] for k in out["f32w"] if k != "inside_reference_bar"}
    out["pass"] = bool(out["f32w"]["inside_reference_bar"] and out["f32w"]["rms_dp_vs_f64"] <= MARGIN * out["f32_direct"]["rms_dp_vs_f64"])
    return out


def main():
    torch.manual_seed(0)
    from helpers import blob_for

    results = []
    for name in ("chess_4x128", "chess_20x256"):
        d, blob, z = blob_for(name)
        results.append(run(name, blob, z))
        print(json.dumps(results[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"what": "f32w (f32 operands, Winograd F(2x2,3x3), U = f32(G g G^T)) and the direct f32 tower, emulated on the CPU, against the fixtures' float64 outputs",
                      "criteria": "f32w inside the reference's cross-runtime bar against the fixtures' reference outputs, and rms |dlogit| vs float64 <= %g x the direct f32 tower's" % MARGIN,
                      "results": results, "pass": all(r["pass"] for r in results)}, indent=1))
    return 0 if all(r["pass"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
