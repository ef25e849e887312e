#!/usr/bin/env python3
"""The numerics gate of a Winograd F(4x4, 3x3) form of the split-precision tower: on the CPU, before (and beside) the kernel.

F(4x4, 3x3) needs 36 multiplies per 4x4 outputs and input channel where F(2x2, 3x3) needs 64 and the direct form 144; its
transforms have larger constants (B^T rows sum to 10 in absolute value, A^T rows to 21, G holds 1/24), so it loses more bits.
How many is emulated here operation for operation in the arithmetic of conv3x3_winof4_kernel (cattus_amd/csrc/winof4_rule.h):

  weights      U = G g G^T from the BatchNorm-folded f32 weights in float64 (Lavin's matrices, points 0, +-1, +-2, inf), ONE
               power-of-two scale per output channel over all 36 frequencies (largest |U 2^s| in [2^10, 2^11)), split (hi, lo)
  activations  plain f32 between the layers, capped at 655 where they are written (the stem included) -- the cap is modelled and
               the values that reached it are counted; zero is expected
  input        V = B^T d B in f32 on 6x6 patches at stride 4, in the header's operation order, split (hi, lo)
  products     M[f] = sum over cin of U_lo V_hi + U_hi V_lo + U_hi V_hi, f32 accumulation
  output       Y = A^T M A in f32 (the header's order), fma(Y, 2^-s, bias), + skip, ReLU, cap

next to the direct and F(2x2) emulations of scripts/winograd_gate_a.py, against the network's float64 run and against the
reference's cross-runtime tolerance (training/tests/test_net_output.py:28-33; the bar that decides).  Nets: the two
reference-made fixtures, 48 leaves of the seed-2 bench network, 6 leaves of chess 40x384.

    python scripts/winograd_gate_f4.py > profiles/winograd_gate_f4.json        # CPU only, a few minutes
    python scripts/winograd_gate_f4.py --only chess_4x128
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

import winograd_gate_a as gate_a  # noqa: E402
from winograd_gate_a import conv_direct_split, conv_winograd_split, fold, heads, pow2_scale, split  # noqa: E402
from cattus_amd import synth  # noqa: E402
from cattus_amd.torch_model import PolicyValueNet  # noqa: E402
from cattus_amd.weights import CHESS, NetDesc, seeded_blob  # noqa: E402

G6 = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
                  dtype=torch.float64)
ACT_MAX = 655.0  # WINOF4_ACT_MAX: 10 x 10 x 655 <= 65504

stats = {"capped": 0, "v_max": 0.0}


def bt_1d(d):
    """winof4_bt_1d: six f32 tensors -> B^T d, every operation an f32 operation in the header's order."""
    a02, a42, s12, s34, a12, a43 = d[0] - d[2], d[4] - d[2], d[1] + d[2], d[3] + d[4], d[1] - d[2], d[4] - d[3]
    a31, a13, a53 = d[3] - d[1], d[1] - d[3], d[5] - d[3]
    return [4.0 * a02 + a42, s34 - 4.0 * s12, 4.0 * a12 + a43, 2.0 * a31 + a42, a42 - 2.0 * a31, 4.0 * a13 + a53]


def at_1d(m):
    s12, s34, a12, a34 = m[1] + m[2], m[3] + m[4], m[1] - m[2], m[3] - m[4]
    return [(s12 + s34) + m[0], a12 + 2.0 * a34, s12 + 4.0 * s34, (a12 + 8.0 * a34) + m[5]]


def cap(y):
    """Activations as the F(4x4) tower writes them: f32, capped, the capped ones counted."""
    stats["capped"] += int((y >= ACT_MAX).sum())
    return y.clamp_max(ACT_MAX)


def conv_winograd_f4(x, w, bias, skip):
    B, C, S, _ = x.shape
    assert S == 8
    U = torch.einsum("ij,ocjk,lk->ocil", G6, w.double(), G6)  # [cout, cin, 6, 6], float64 on the host
    sc = pow2_scale(U)
    Uh, Ul = split((U * sc[:, None, None, None]).float())
    tiles = F.pad(x, (1, 1, 1, 1)).unfold(2, 6, 4).unfold(3, 6, 4)  # [B, C, 2, 2, 6, 6]
    t = torch.stack(bt_1d([tiles[..., a, :] for a in range(6)]), dim=-2)  # columns first: t[..., i, b]
    V = torch.stack(bt_1d([t[..., b] for b in range(6)]), dim=-1)  # then rows: V[..., i, l]
    stats["v_max"] = max(stats["v_max"], float(V.abs().max()))
    Vh, Vl = split(V)

    def mm(Ux, Vx):
        return torch.einsum("ocil,bctuil->botuil", Ux, Vx)

    M = mm(Ul, Vh) + mm(Uh, Vl) + mm(Uh, Vh)
    z = torch.stack(at_1d([M[..., i, :] for i in range(6)]), dim=-2)  # z[..., p, l]
    Y = torch.stack(at_1d([z[..., l] for l in range(6)]), dim=-1)  # [B, O, 2, 2, 4, 4]
    Y = Y.permute(0, 1, 2, 4, 3, 5).reshape(B, -1, S, S)
    y = Y * (1.0 / sc).float()[None, :, None, None] + bias[None, :, None, None]  # the scale is a power of two: one rounding, as the kernel's fma
    if skip is not None:
        y = y + skip
    return cap(torch.relu(y))


def tower_f4(net, x):
    w, b = fold(net._conv1._conv.weight, net._conv1._bn)
    a = cap(conv_direct_split(x, w, b, None))  # the stem stays direct and writes capped f32 rows (CONV_OUT_F32 | CONV_WINOF4_IN)
    for blk in net._residual_blocks:
        w1, b1 = fold(blk._conv1.weight, blk._bn1)
        w2, b2 = fold(blk._conv2.weight, blk._bn2)
        t = conv_winograd_f4(a, w1, b1, None)
        a = conv_winograd_f4(t, w2, b2, a)
    return a


def shares(p, v, pr, vr):
    """Worst share of the reference's bands: policy |d| / (1e-6 + 1e-3 |ref|) (numpy.isclose), value |d| / max(1e-5 max(|a|, |b|), 1e-6)."""
    ps = float((np.abs(p - pr) / (1e-6 + 1e-3 * np.abs(pr))).max())
    vs = float((np.abs(v - vr) / np.maximum(1e-5 * np.maximum(np.abs(v), np.abs(vr)), 1e-6)).max())
    return ps, vs


def run(name, blob, planes, p_ref32=None, v_ref32=None):
    net = PolicyValueNet.from_blob(blob)
    d = net.desc
    bits = np.unpackbits(planes.view(np.uint8).reshape(len(planes), d.planes, -1), axis=-1, bitorder="little")
    x = torch.from_numpy(bits[..., : d.hw].reshape(len(planes), d.planes, d.board, d.board).astype(np.float32))
    stats["capped"], stats["v_max"] = 0, 0.0
    with torch.no_grad():
        p64, v64 = net.double()(x.double())
        p64, v64 = p64.numpy(), v64.flatten().numpy()
        net = net.float()
        p32, v32 = net(x)
        p32, v32 = p32.numpy(), v32.flatten().numpy()
        out = {"net": name, "blocks": d.blocks, "filters": d.filters, "leaves": len(planes),
               "reference": "reference-made f32 outputs" if p_ref32 is not None else "torch f32 run",
               "torch_f32_vs_f64": dict(dp=float(np.abs(p32 - p64).max()), dv=float(np.abs(v32 - v64).max()))}
        if p_ref32 is None:
            p_ref32, v_ref32 = p32, v32
        forms = (("direct_split", lambda: gate_a.tower(net, x, conv_direct_split)), ("winograd_split", lambda: gate_a.tower(net, x, conv_winograd_split)),
                 ("winograd_f4_split", lambda: tower_f4(net, x)))
        for form, tower in forms:
            p, v = heads(net, tower())
            p, v = p.numpy(), v.numpy()
            ps, vs = shares(p, v, p_ref32, np.asarray(v_ref32).reshape(-1))
            out[form] = dict(dp_vs_f64=float(np.abs(p - p64).max()), dv_vs_f64=float(np.abs(v - v64).max()), policy_band_share=ps, value_band_share=vs,
                             within_reference_tolerance=gate_a.ref_tol_ok(p, v, p_ref32, np.asarray(v_ref32).reshape(-1)))
    out["winograd_f4_split"]["activations_capped"] = stats["capped"]
    out["winograd_f4_split"]["v_abs_max"] = stats["v_max"]
    out["f4_over_direct"] = dict(dp=out["winograd_f4_split"]["dp_vs_f64"] / out["direct_split"]["dp_vs_f64"],
                                 dv=out["winograd_f4_split"]["dv_vs_f64"] / out["direct_split"]["dv_vs_f64"])
    return out


def run_fixture(name):
    from helpers import blob_for

    d, blob, z = blob_for(name)
    return run(name, blob, z["planes"], z["policy"], z["value"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", help="one reference-made fixture (chess_4x128, chess_20x256)")
    ap.add_argument("--leaves20", type=int, default=48, help="leaves of the seeded chess 20x256 batch (the bench weights)")
    ap.add_argument("--leaves40", type=int, default=6, help="leaves of the seeded chess 40x384 batch")
    args = ap.parse_args()
    torch.manual_seed(0)
    if args.only:
        print(json.dumps(run_fixture(args.only), indent=1))
        return
    results = [run_fixture("chess_20x256"), run_fixture("chess_4x128")]
    d20 = NetDesc(**CHESS, blocks=20, filters=256, vhc=8, phc=8)
    results.append(run("chess20x256 bench weights (seed 2)", seeded_blob(d20, 2), synth.random_chess_planes(args.leaves20, 2)))
    d40 = NetDesc(**CHESS, blocks=40, filters=384, vhc=8, phc=8)
    results.append(run("chess40x384 (seed 3)", seeded_blob(d40, 3), synth.random_chess_planes(args.leaves40, 3)))
    print(json.dumps({"gate": "winograd F(4x4, 3x3), f16x2 operands, one scale per output channel",
                      "headline_inside_reference_tolerance": all(r["winograd_f4_split"]["within_reference_tolerance"] for r in results[:3]),
                      "results": results}, indent=1))


if __name__ == "__main__":
    main()
