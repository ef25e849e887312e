"""The numerics gate of the Winograd F(4x4, 3x3) form (scripts/winograd_gate_f4.py) on the small reference-made fixture, on the CPU:
the emulation of conv3x3_winof4_kernel's arithmetic stays inside the reference's cross-runtime tolerance on chess_4x128, reaches the
activation cap nowhere, and is what profiles/winograd_gate_f4.json records for that fixture."""

import importlib.util
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _gate():
    spec = importlib.util.spec_from_file_location("winograd_gate_f4", ROOT / "scripts" / "winograd_gate_f4.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules["winograd_gate_f4"] = mod
    spec.loader.exec_module(mod)
    return mod


def test_the_emulated_form_is_inside_the_reference_tolerance_on_chess_4x128():
    out = _gate().run_fixture("chess_4x128")
    f4 = out["winograd_f4_split"]
    print(json.dumps(out))
    assert out["leaves"] == 64 and f4["within_reference_tolerance"]
    assert f4["policy_band_share"] < 1.0 and f4["value_band_share"] < 1.0
    assert f4["activations_capped"] == 0 and 0 < f4["v_abs_max"] <= 65500.0
    assert out["direct_split"]["within_reference_tolerance"] and out["winograd_split"]["within_reference_tolerance"]
    # the committed record is this run (torch's f32 matmul may order a sum differently from build to build: a factor of two either way)
    rec = {r["net"]: r for r in json.loads((ROOT / "profiles" / "winograd_gate_f4.json").read_text())["results"]}["chess_4x128"]["winograd_f4_split"]
    assert rec["within_reference_tolerance"] and rec["activations_capped"] == 0
    assert 0.5 * rec["dp_vs_f64"] <= f4["dp_vs_f64"] <= 2 * rec["dp_vs_f64"] and 0.5 * rec["dv_vs_f64"] <= f4["dv_vs_f64"] <= 2 * rec["dv_vs_f64"]
