"""The comparison rule of cattus_hip_verify without a GPU: cattus_amd/csrc/verify_rule.h against a float64 numpy restatement.

tests/verify_rule_check.cpp is a stand-alone program around the header.  It is built with the host compiler twice -- plain, and with
-fsanitize=address,undefined -- and both are run as programs on a file of cases this test writes (floats travel as the hex of their 32
bits, so NaNs and signed zeros arrive as written).  The restatement below says the rule again in numpy float64; both programs must print
what it gives, pair by pair and leaf by leaf.  test_verify_gpu.py holds the kernel and the evaluator's sticky record to the same functions.

The rule (the issue's wording; b is the f32 shadow):
    dlogit(a, b) = float32(|float64(a) - float64(b)|)
    a logit is inside when |a - b| <= 1e-6 + 1e-3 |b| in float64, a value when |a - b| <= max(1e-5 max(|a|, |b|), 1e-6); a non-finite
    operand is outside; a leaf is outside when its value or any logit is; two scrubbed logits (f32::MIN both) differ by 0: inside.
A leaf's record: the largest dlogit over its moves with the lowest index that holds it (NaN differences take no part; 0 at move 0 where
none is positive), float32 |dvalue| (NaN as 0x7fc00000), flags bit 0 leaf outside, bit 1 value outside.

The boundary.  t = 1e-6 + 1e-3 |b| is a float64 with a full significand, and b + t is not an f32 for any b tried, so "the exact boundary"
is taken where f32 pairs can reach it: for each b the float64 number b + t, the f32 on either side of it, and one more ulp out on both
sides -- four values of a whose side of the bar is decided here in exact rational arithmetic on the float64 constants, not by the code
under test.
"""

import math
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from cattus_amd.build import CSRC

from helpers import REF_POLICY_ATOL, REF_POLICY_RTOL, REF_VALUE_ABS, REF_VALUE_REL, outputs_equal_ref_tol
from test_weight_layout import host_compiler

HERE = Path(__file__).resolve().parent
F32_MIN = np.float32(np.finfo(np.float32).min)  # f32::MIN, what a scrubbed logit holds
RECORD = np.dtype([("max_dlogit", "<f4"), ("move", "<u4"), ("dvalue", "<f4"), ("flags", "<u4")])
QNAN = np.uint32(0x7FC00000)


# ---------------------------------------------------------------------------------------- the restatement


def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def dlogit_restated(a, b) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.abs(_f64(a) - _f64(b)).astype(np.float32)


def logit_inside_restated(a, b) -> np.ndarray:
    a, b = _f64(a), _f64(b)
    with np.errstate(all="ignore"):
        return np.isfinite(a) & np.isfinite(b) & (np.abs(a - b) <= REF_POLICY_ATOL + REF_POLICY_RTOL * np.abs(b))


def value_inside_restated(a, b) -> np.ndarray:
    a, b = _f64(a), _f64(b)
    with np.errstate(all="ignore"):
        bound = np.maximum(REF_VALUE_REL * np.maximum(np.abs(a), np.abs(b)), REF_VALUE_ABS)
        return np.isfinite(a) & np.isfinite(b) & (np.abs(a - b) <= bound)


def dvalue_restated(a, b) -> np.ndarray:
    d = np.atleast_1d(dlogit_restated(a, b)).copy()
    d.view(np.uint32)[np.isnan(d)] = QNAN
    return d


def records_restated(policy_a, policy_b, value_a, value_b) -> np.ndarray:
    """[n] records of dtype RECORD for logits [n, M] and values [n] of two runtimes, b the reference side."""
    policy_a, policy_b = np.asarray(policy_a, dtype=np.float32), np.asarray(policy_b, dtype=np.float32)
    d = dlogit_restated(policy_a, policy_b)
    d = np.where(np.isnan(d), np.float32(-1), d)
    out = np.zeros(len(d), dtype=RECORD)
    positive = d.max(axis=1) > 0
    out["max_dlogit"] = np.where(positive, d.max(axis=1), np.float32(0))
    out["move"] = np.where(positive, d.argmax(axis=1), 0)  # argmax: the first index that holds the maximum
    out["dvalue"] = dvalue_restated(value_a, value_b)
    v_out = ~value_inside_restated(value_a, value_b)
    leaf_out = v_out | ~logit_inside_restated(policy_a, policy_b).all(axis=1)
    out["flags"] = leaf_out.astype(np.uint32) | (v_out.astype(np.uint32) << 1)
    return out


def fold_restated(records, policy_a, policy_b, value_a, value_b, into=None) -> dict:
    """The evaluator's sticky record after one more verified batch, leaves in index order: the first verified leaf seeds the worst-logit
    entry, after that only a strictly larger difference replaces an entry (`leaf`: index into this batch, None if an earlier batch's stays)."""
    s = dict(into) if into else dict(batches=0, leaves=0, leaves_outside=0, max_dlogit=0.0, logit=0.0, logit_ref=0.0, move=0, max_dvalue=0.0,
                                    value=0.0, value_ref=0.0, seeded=False)
    s["batches"] += 1
    s["leaf"] = None
    for i, r in enumerate(records):
        s["leaves"] += 1
        s["leaves_outside"] += int(r["flags"]) & 1
        if not s["seeded"] or float(r["max_dlogit"]) > s["max_dlogit"]:
            m = int(r["move"])
            s.update(seeded=True, leaf=i, max_dlogit=float(r["max_dlogit"]), move=m, logit=float(policy_a[i][m]), logit_ref=float(policy_b[i][m]))
        if float(r["dvalue"]) > s["max_dvalue"]:
            s.update(max_dvalue=float(r["dvalue"]), value=float(value_a[i]), value_ref=float(value_b[i]))
    return s


# ---------------------------------------------------------------------------------------- the cases


def _bits(x) -> str:
    return "%08x" % int(np.asarray(x, dtype=np.float32).reshape(1).view(np.uint32)[0])


def boundary_pairs():
    """[(a, b, inside)] around |a - b| == atol + rtol |b| for logits: per b the f32 below and above the float64 boundary and one ulp
    further out, on both sides of b; `inside` decided in exact arithmetic on the float64 numbers the rule names."""
    out = []
    for b in [0.0, -0.0, 1.0, -1.0, 1e-4, 0.3, -7.25, 50.0, 1e-30, 1000.0]:
        b = np.float32(b)
        t = REF_POLICY_ATOL + REF_POLICY_RTOL * abs(float(b))  # float64, as the rule computes it
        for sign in (1.0, -1.0):
            edge = float(b) + sign * t
            near = np.float32(edge)
            for a in {near, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf)),
                      np.nextafter(np.nextafter(near, np.float32(np.inf)), np.float32(np.inf)),
                      np.nextafter(np.nextafter(near, np.float32(-np.inf)), np.float32(-np.inf))}:
                out.append((a, b, abs(Fraction(float(a)) - Fraction(float(b))) <= Fraction(t)))
    assert {x[2] for x in out} == {True, False}
    return out


def value_boundary_pairs():
    out = []
    for b in [0.0, 1.0, -1.0, 0.5, -0.05, 0.1, 1e-3, 2e-7]:
        b = np.float32(b)
        for sign in (1.0, -1.0):
            near = np.float32(float(b) + sign * max(REF_VALUE_REL * abs(float(b)), REF_VALUE_ABS))
            for a in {near, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf))}:
                fa, fb = abs(Fraction(float(a))), abs(Fraction(float(b)))
                rel = REF_VALUE_REL * max(abs(float(a)), abs(float(b)))  # one float64 product, as the rule and math.isclose make it
                out.append((a, b, abs(Fraction(float(a)) - Fraction(float(b))) <= max(Fraction(rel), Fraction(REF_VALUE_ABS))))
                assert out[-1][2] == math.isclose(float(a), float(b), rel_tol=REF_VALUE_REL, abs_tol=REF_VALUE_ABS), (a, b, fa, fb)
    assert {x[2] for x in out} == {True, False}
    return out


SPECIAL = [np.float32(x) for x in (0.0, -0.0, 1.0, -1.0, 0.5, np.inf, -np.inf, np.nan, F32_MIN, np.finfo(np.float32).max, 1e-45, 3.25)]


def random_pairs(count=10000, seed=5):
    """f32 pairs at logit scales 1e-4 .. 50: b, and a = b (1 + e) + e' with e, e' log-uniform around the bar's rtol and atol, either sign."""
    rng = np.random.default_rng(seed)
    b = (10.0 ** rng.uniform(-4, math.log10(50.0), count) * rng.choice([-1.0, 1.0], count)).astype(np.float32)
    rel = 10.0 ** rng.uniform(-5, -1.5, count) * rng.choice([-1.0, 1.0], count)
    ab = 10.0 ** rng.uniform(-8, -4.5, count) * rng.choice([-1.0, 1.0], count)
    a = (b.astype(np.float64) * (1.0 + rel) + ab).astype(np.float32)
    return a, b


@pytest.fixture(scope="module")
def rule_checks(tmp_path_factory):
    """The stand-alone program, plain and under AddressSanitizer + UBSan (run as programs: no preloading of anything)."""
    d = tmp_path_factory.mktemp("verify_rule")
    exes = []
    for name, extra in (("verify_rule_check", []), ("verify_rule_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / name
        # -ffp-contract=off: as the library itself is built (cattus_amd/build.py)
        subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *extra, f"-I{CSRC}",
                               str(HERE / "verify_rule_check.cpp"), "-o", str(exe)])
        exes.append(exe)
    return exes


def _run(exe, path):
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("verify rule ok"), run.stdout[-3000:] + run.stderr[-3000:]
    return run.stdout.splitlines()[:-1]


def test_pairs_agree_with_the_restatement_plain_and_under_sanitizers(rule_checks, tmp_path):
    logit_edges, value_edges = boundary_pairs(), value_boundary_pairs()
    ra, rb = random_pairs()
    pairs = [(a, b) for a, b, _ in logit_edges] + [(a, b) for a, b, _ in value_edges] + [(a, b) for a in SPECIAL for b in SPECIAL] + list(zip(ra, rb))
    a = np.array([p[0] for p in pairs], dtype=np.float32)
    b = np.array([p[1] for p in pairs], dtype=np.float32)
    (tmp_path / "pairs.txt").write_text("".join("P %s %s\n" % (_bits(x), _bits(y)) for x, y in zip(a, b)))
    want_d, want_l, want_v, want_dv = dlogit_restated(a, b), logit_inside_restated(a, b), value_inside_restated(a, b), dvalue_restated(a, b)
    # the restatement itself: the edges' exact verdicts, and the named cases
    n_l, n_v = len(logit_edges), len(value_edges)
    assert list(want_l[:n_l]) == [e[2] for e in logit_edges]
    assert list(want_v[n_l:n_l + n_v]) == [e[2] for e in value_edges]
    one = lambda f, x, y: bool(f(np.float32(x), np.float32(y)))
    assert one(logit_inside_restated, F32_MIN, F32_MIN) and float(dlogit_restated(F32_MIN, F32_MIN)) == 0.0
    assert not one(logit_inside_restated, F32_MIN, 1.0) and not one(logit_inside_restated, 1.0, F32_MIN)
    assert one(logit_inside_restated, 0.0, -0.0) and one(value_inside_restated, -0.0, 0.0)
    assert one(value_inside_restated, 1.0, 1.0) and one(value_inside_restated, -1.0, -1.0) and not one(value_inside_restated, 1.0, -1.0)
    for bad in (np.inf, -np.inf, np.nan):
        for other in (0.0, bad):
            assert not one(logit_inside_restated, bad, other) and not one(logit_inside_restated, other, bad)
            assert not one(value_inside_restated, bad, other) and not one(value_inside_restated, other, bad)
    for exe in rule_checks:
        rows = [line.split() for line in _run(exe, tmp_path / "pairs.txt")]
        assert len(rows) == len(pairs)
        got_d = np.array([int(r[0], 16) for r in rows], dtype=np.uint32)
        got_dv = np.array([int(r[3], 16) for r in rows], dtype=np.uint32)
        nan = np.isnan(want_d)
        assert (np.isnan(got_d.view(np.float32)) == nan).all() and (got_d[~nan] == want_d.view(np.uint32)[~nan]).all()
        assert (got_dv == want_dv.view(np.uint32)).all()
        assert [int(r[1]) for r in rows] == list(want_l.astype(int)) and [int(r[2]) for r in rows] == list(want_v.astype(int))


def leaf_cases():
    """(policy_a, policy_b, value_a, value_b) per leaf, of several widths: random rows near the bar, planted ties, NaN / inf / f32::MIN."""
    rng = np.random.default_rng(17)
    cases = []
    for M in (1, 3, 9, 67, 130):
        for k in range(6):
            ra, rb = random_pairs(M, seed=100 * M + k)
            ra, rb = ra.copy(), rb.copy()
            if k == 1:
                ra[:] = rb  # nothing differs
            if k == 2 and M >= 3:
                ra[:] = rb
                ra[[M - 1, M // 2]], rb[[M - 1, M // 2]] = 0.5, 0.0  # one maximum at two indices: the lower one is reported
            if k == 3:
                ra[rng.integers(M)] = np.nan
                rb[rng.integers(M)] = np.inf
            if k == 4:
                ra[0] = rb[0] = F32_MIN
                if M > 1:
                    ra[M - 1] = F32_MIN
            va = np.float32(rng.uniform(-1, 1))
            vb = va if k % 2 else np.float32(float(va) * (1 + 10.0 ** rng.uniform(-7, -3)))
            if k == 5:
                va = np.float32(np.nan)
            cases.append((ra, rb, va, vb))
    return cases


def test_leaves_agree_with_the_restatement_plain_and_under_sanitizers(rule_checks, tmp_path):
    cases = leaf_cases()
    text = ""
    for ra, rb, va, vb in cases:
        text += "L %d %s %s %s\n" % (len(ra), _bits(va), _bits(vb), " ".join("%s %s" % (_bits(x), _bits(y)) for x, y in zip(ra, rb)))
    (tmp_path / "leaves.txt").write_text(text)
    want = [records_restated(ra[None], rb[None], [va], [vb])[0] for ra, rb, va, vb in cases]
    assert any(w["flags"] == 0 for w in want) and any(w["flags"] == 1 for w in want) and any(w["flags"] == 3 for w in want)
    assert any(w["max_dlogit"] == 0 for w in want) and any(np.isinf(w["max_dlogit"]) for w in want)
    for (ra, _, _, _), w in list(zip(cases, want))[2::6]:  # the planted ties
        if len(ra) >= 3:
            assert w["max_dlogit"] == 0.5 and w["move"] == len(ra) // 2, (len(ra), w)
    for exe in rule_checks:
        rows = _run(exe, tmp_path / "leaves.txt")
        assert len(rows) == len(cases)
        for row, w, c in zip(rows, want, cases):
            got = np.array([int(x, 16) for x in row.split()], dtype=np.uint32).view(RECORD)[0]
            assert got.tobytes() == w.tobytes(), (got, w, len(c[0]))


def test_the_leaf_verdict_is_the_bar_the_gpu_tests_use():
    """Away from the boundary (no pair within 1e-9 relative of it) the restatement's leaf verdict is helpers.outputs_equal_ref_tol, the
    function every f16x2 test of this suite holds the tower to -- for logits as the value, and for values."""
    ra, rb = random_pairs()
    a64, b64 = ra.astype(np.float64), rb.astype(np.float64)
    t = REF_POLICY_ATOL + REF_POLICY_RTOL * np.abs(b64)
    clear = np.abs(np.abs(a64 - b64) - t) > 1e-9 * t
    assert clear.sum() > 9900
    rows_a, rows_b = ra[clear][:9900].reshape(-1, 3), rb[clear][:9900].reshape(-1, 3)
    va = np.clip(rows_a[:, 0], -1, 1)
    vb = np.clip(rows_b[:, 0], -1, 1)
    tv = np.maximum(REF_VALUE_REL * np.maximum(np.abs(va), np.abs(vb)).astype(np.float64), REF_VALUE_ABS)
    vclear = np.abs(np.abs(va.astype(np.float64) - vb.astype(np.float64)) - tv) > 1e-9 * tv
    rec = records_restated(rows_a, rows_b, va, vb)
    verdicts = set()
    for i in np.flatnonzero(vclear):
        inside = outputs_equal_ref_tol(rows_a[i:i + 1], va[i:i + 1], rows_b[i:i + 1], vb[i:i + 1])
        assert inside == (rec["flags"][i] & 1 == 0), (i, rows_a[i], rows_b[i], va[i], vb[i])
        verdicts.add(inside)
    # logits alone (equal values), where both verdicts do occur
    rec = records_restated(rows_a, rows_b, vb, vb)
    for i in range(len(rows_a)):
        inside = outputs_equal_ref_tol(rows_a[i:i + 1], vb[i:i + 1], rows_b[i:i + 1], vb[i:i + 1])
        assert inside == (rec["flags"][i] == 0), i
        verdicts.add(inside)
    pair_inside = logit_inside_restated(ra[clear], rb[clear])
    assert (pair_inside == np.isclose(ra[clear], rb[clear], rtol=REF_POLICY_RTOL, atol=REF_POLICY_ATOL)).all() and 0.2 < pair_inside.mean() < 0.8
    assert verdicts == {True, False}
