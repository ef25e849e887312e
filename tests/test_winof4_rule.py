"""The Winograd F(4x4, 3x3) form without a GPU: cattus_amd/csrc/winof4_rule.h and its entries in weight_layout.h against numpy.

tests/winof4_rule_check.cpp is a stand-alone program around the headers.  It is built with the host compiler twice -- plain, and with
-fsanitize=address,undefined -- and both are run as programs on a file of cases this test writes.  The headers are what
conv3x3_winof4_kernel, the evaluator's upload and cattus_hip_create_calibrated share; test_winof4_gpu.py holds the kernel to them.

In the program itself: tile geometry (every board pixel the output of exactly one (tile, y, x); off-board patch pixels exactly those
outside 0..7), the frequency -> wave map, the U index as a bijection onto the payload, winof4_u decoding to the float64 U, the cap's
derivation.  Against numpy here: the algebra in float64, the f32 transforms bit for bit, calibrated_stream_shifts' default, and stream_shifts' ceiling (the guard the F(4x4) tower puts on the
estimate: a channel far above the median is held back, weight_layout.h WINOF4_STREAM_CEILING) -- dead, infinite and NaN channels, a
global shift of 16, a channel exactly at the ceiling, a random sweep; guarded_shifts is the restatement test_winof4_range_gpu.py
holds the evaluator to."""

import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from cattus_amd.build import CSRC

from test_weight_layout import host_compiler

HERE = Path(__file__).resolve().parent

# Lavin's matrices for the points 0, +-1, +-2, infinity -- restated, not read from the header
BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=np.float64)
G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)


@pytest.fixture(scope="module")
def rule_checks(tmp_path_factory):
    """The stand-alone program, plain and under AddressSanitizer + UBSan (run as programs: no preloading of anything)."""
    d = tmp_path_factory.mktemp("winof4_rule")
    exes = []
    for name, extra in (("winof4_rule_check", []), ("winof4_rule_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / name
        # -ffp-contract=off: as the library's host code is built (cattus_amd/build.py)
        subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *extra, f"-I{CSRC}", str(HERE / "winof4_rule_check.cpp"), "-o", str(exe)])
        exes.append(exe)
    return exes


def _run(exe, path):
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("winof4 rule ok"), run.stdout[-3000:] + run.stderr[-3000:]
    return run.stdout.splitlines()[:-1]


# ---------------------------------------------------------------------------------------- the restatement (float32, the header's order)

F = np.float32


def bt_1d(d):
    """d: six float32 arrays -> B^T d, every operation a float32 operation in winof4_bt_1d's order."""
    a02, a42, s12, s34, a12, a43 = d[0] - d[2], d[4] - d[2], d[1] + d[2], d[3] + d[4], d[1] - d[2], d[4] - d[3]
    a31, a13, a53 = d[3] - d[1], d[1] - d[3], d[5] - d[3]
    return [F(4) * a02 + a42, s34 - F(4) * s12, F(4) * a12 + a43, F(2) * a31 + a42, a42 - F(2) * a31, F(4) * a13 + a53]


def at_1d(m):
    s12, s34, a12, a34 = m[1] + m[2], m[3] + m[4], m[1] - m[2], m[3] - m[4]
    return [(s12 + s34) + m[0], a12 + F(2) * a34, s12 + F(4) * s34, (a12 + F(8) * a34) + m[5]]


def input_2d(d):
    """d [n, 6, 6] float32 -> V [n, 6, 6]: columns first (T = B^T d), then rows (V = T B)."""
    t = np.stack(bt_1d([d[:, a, :] for a in range(6)]), axis=1)  # t[:, i, b]
    return np.stack(bt_1d([t[:, :, b] for b in range(6)]), axis=2)  # v[:, i, l]


def output_2d(m):
    z = np.stack(at_1d([m[:, i, :] for i in range(6)]), axis=1)  # z[:, p, l]
    return np.stack(at_1d([z[:, :, l] for l in range(6)]), axis=2)  # y[:, p, q]


def shifts(s2, abs_max, headroom):
    """weight_layout.h: stream_shifts on the measured mean squares, then the headroom guard."""
    n = len(s2)
    srt = sorted(s2)
    S = math.sqrt(srt[n // 2] if n % 2 else 0.5 * (srt[n // 2 - 1] + srt[n // 2]))
    t = 0 if not (S > 0.0) or not math.isfinite(S) or S >= 0.5 else min(16, -math.frexp(S)[1] + 1)
    out = []
    for k in range(n):
        s = math.sqrt(s2[k])
        tk = t if not (s > 0.0) or not math.isfinite(s) or math.ldexp(s, t) >= 0.5 else min(16, -math.frexp(s)[1] + 1)
        while tk > 0 and math.ldexp(abs_max[k], tk) > headroom:
            tk -= 1
        out.append(tk)
    return out


CEILING = 2.0  # WINOF4_STREAM_CEILING (the program checks the header's constant against this figure)


def guarded_shifts(s2, ceiling):
    """weight_layout.h: stream_shifts with a ceiling -- (global shift, the unguarded t_k, the guarded t_k).  The unguarded rule, then:
    while t_k > 0 and s_k 2^t_k >= ceiling, t_k drops by one; a dead channel and one whose s_k is not finite keep the global shift."""
    plain = shifts(list(s2), [0.0] * len(s2), math.inf)  # abs_max 0: the headroom guard of `shifts` never acts
    srt = sorted(s2)
    n = len(s2)
    S = math.sqrt(srt[n // 2] if n % 2 else 0.5 * (srt[n // 2 - 1] + srt[n // 2]))
    t = 0 if not (S > 0.0) or not math.isfinite(S) or S >= 0.5 else min(16, -math.frexp(S)[1] + 1)
    held = []
    for s2k, tk in zip(s2, plain):
        s = math.sqrt(s2k)
        while tk > 0 and math.isfinite(s) and math.ldexp(s, tk) >= ceiling:
            tk -= 1
        held.append(tk)
    return t, plain, held


# ---------------------------------------------------------------------------------------- the tests


def _hex32(a):
    return " ".join("%08x" % v for v in np.asarray(a, dtype=np.float32).reshape(-1).view(np.uint32))


def _hex64(a):
    return " ".join("%016x" % v for v in np.asarray(a, dtype=np.float64).reshape(-1).view(np.uint64))


def test_algebra_transforms_geometry_index_and_cap_plain_and_under_sanitizers(rule_checks, tmp_path):
    rng = np.random.default_rng(11)
    # f32 patches: unit normals, values at the cap, 2^-20 .. 2^9 spreads, exact zeros, and the sign pattern that reaches the bound
    d32 = np.concatenate([rng.standard_normal((40, 6, 6)), 655.0 * rng.choice([-1.0, 1.0, 0.0], size=(20, 6, 6)),
                          rng.standard_normal((40, 6, 6)) * np.exp2(rng.integers(-20, 10, size=(40, 6, 6)))]).astype(np.float32)
    m32 = (rng.standard_normal((60, 6, 6)) * np.exp2(rng.integers(-8, 20, size=(60, 6, 6)))).astype(np.float32)
    g64, d64 = rng.standard_normal((50, 3, 3)), rng.standard_normal((50, 6, 6))
    cal = []
    for n in (1, 6, 256):
        s2 = np.exp2(rng.uniform(-24, 6, size=n))
        s2[rng.random(n) < 0.1] = 0.0
        cal.append((s2, np.sqrt(s2) * np.exp2(rng.uniform(0, 9, size=n))))
    text = "".join("I %s\n" % _hex32(d) for d in d32) + "".join("O %s\n" % _hex32(m) for m in m32)
    text += "".join("D %s %s\n" % (_hex64(g), _hex64(d)) for g, d in zip(g64, d64))
    text += "".join("S %s %d %s %s\n" % (_hex64([163.75]), len(s2), _hex64(s2), _hex64(mx)) for s2, mx in cal)
    (tmp_path / "cases.txt").write_text(text)

    # the restatement against the matrices (float64 products of small integers and float32 data are close, not equal)
    v_want, y_want = input_2d(d32), output_2d(m32)
    assert v_want.dtype == np.float32 and y_want.dtype == np.float32
    np.testing.assert_allclose(v_want, BT @ d32.astype(np.float64) @ BT.T, rtol=0, atol=1e-4 * np.abs(d32).max())
    np.testing.assert_allclose(y_want, AT @ m32.astype(np.float64) @ AT.T, rtol=0, atol=5e-4 * np.abs(m32).max())
    assert np.abs(BT).sum(axis=1).max() == 10 and 10 * 10 * 655.0 <= 65504 < 10 * 10 * 656.0  # the cap's derivation
    # float64: the sixteen direct correlations
    direct = np.zeros((50, 4, 4))
    for y in range(4):
        for x in range(4):
            direct[:, y, x] = (g64 * d64[:, y:y + 3, x:x + 3]).sum(axis=(1, 2))

    want = [_hex32(v) for v in v_want] + [_hex32(y) for y in y_want]
    for exe in rule_checks:
        rows = _run(exe, tmp_path / "cases.txt")
        assert len(rows) == len(want) + 50 + len(cal)
        for k, (row, w) in enumerate(zip(rows, want)):
            assert row.strip() == w, (k, row, w)  # the f32 transforms, bit for bit
        got = np.array([[int(h, 16) for h in row.split()] for row in rows[len(want):len(want) + 50]], dtype=np.uint64).view(np.float64).reshape(50, 4, 4)
        assert np.abs(got - direct).max() <= 1e-12, np.abs(got - direct).max()
        for (s2, mx), row in zip(cal, rows[len(want) + 50:]):
            dflt, tight = (list(map(int, part.split())) for part in row.split("|"))
            assert dflt == shifts(list(s2), list(mx), 4096.0)  # the default headroom is today's
            assert tight == shifts(list(s2), list(mx), 163.75) and all(a <= b for a, b in zip(tight, dflt))
    assert any(a < b for (s2, mx) in cal[2:] for a, b in zip(shifts(list(s2), list(mx), 163.75), shifts(list(s2), list(mx), 4096.0)))  # the tighter guard bites somewhere


def _sq(v):
    return [x * x for x in v]


SMALL = 1.5 * 2.0**-8
# (what, s2, global shift, the unguarded t_k, t_k under the ceiling 2): the named cases, with what the rule must give written out
GUARD_NAMED = [
    ("M8's shape: a median at 2^-8 beside a unit channel and one in [0.75, 1)", _sq([SMALL, SMALL, SMALL, 1.0, 0.75]), 8, [8] * 5, [8, 8, 8, 0, 1]),
    ("exactly at the ceiling drops, just under it stays", _sq([SMALL] * 5 + [2.0**-7, float(np.nextafter(2.0**-7, 0.0))]), 8, [8] * 7, [8] * 5 + [7, 8]),
    ("a dead channel and an infinite one keep the global shift", _sq([SMALL] * 5) + [math.inf, 0.0, 1.0], 8, [8] * 8, [8] * 7 + [0]),
    ("nothing to go by", [math.nan], 0, [0], [0]),
    ("t = 16", _sq([2.0**-30] * 5 + [1.0, 2.0**-16, 2.0**-15]), 16, [16] * 8, [16] * 5 + [0, 16, 15]),
    ("t = 0: the guard cannot act", _sq([1.0, 4.0, 100.0, 0.75]), 0, [0] * 4, [0] * 4),
    ("a lifted channel sits in [1, 2), under the ceiling", _sq([1.0, 1.0, 1.0, 0.99 * 2.0**-8, 1.99 * 2.0**-8]), 0, [0, 0, 0, 9, 8], [0, 0, 0, 9, 8]),
    ("the guard stops at 0", _sq([SMALL] * 3 + [1e30]), 8, [8] * 4, [8, 8, 8, 0]),
]


def test_the_estimates_ceiling_agrees_with_its_restatement_plain_and_under_sanitizers(rule_checks, tmp_path):
    rng = np.random.default_rng(12)
    cases = [(s2, CEILING) for _, s2, _, _, _ in GUARD_NAMED]
    for _ in range(300):
        n = int(rng.integers(1, 12))
        s = np.exp2(rng.uniform(-20, 4, n)) * (rng.random(n) > 0.1)  # one channel in ten dead
        cases.append((list(s * s), CEILING if rng.random() < 0.7 else float(np.exp2(rng.integers(-2, 9)))))
    text = "".join("C %s %d %s\n" % (_hex64([c]), len(s2), _hex64(s2)) for s2, c in cases)
    (tmp_path / "cases.txt").write_text(text)
    for what, s2, t, plain, held in GUARD_NAMED:
        assert guarded_shifts(s2, CEILING) == (t, plain, held), what  # the restatement gives what is written out
    for exe in rule_checks:
        rows = _run(exe, tmp_path / "cases.txt")
        assert len(rows) == len(cases)
        acted = 0
        for (s2, c), row in zip(cases, rows):
            t, plain, held = ([int(x) for x in part.split()] for part in row.split("|"))
            assert (t[0], plain, held) == guarded_shifts(s2, c), (s2, c, row)
            acted += sum(a < b for a, b in zip(held, plain))
        assert acted > 100  # the sweep does meet the guard
