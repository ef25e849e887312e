"""The prior rule of cattus_hip_verify without a GPU: cattus_amd/csrc/prior_rule.h against a numpy restatement.

tests/prior_rule_check.cpp is a stand-alone program around the header.  It is built with the host compiler twice -- plain, and with
-fsanitize=address,undefined -- and both are run as programs on a file of cases this test writes (floats travel as the hex of their 32
bits).  The restatement below says the rule again in numpy; both programs must print its bytes, leaf by leaf, and its fold of the sticky
record.  test_verify_priors_gpu.py holds the kernel and the evaluator's record to the same functions.

The rule (the issue's wording; pb is the f32 shadow's row, c = min(legal_count, L)):
    tv      float32(0.5 * sum_k |float64(pa[k]) - float64(pb[k])|) over k < c, summed as a wave sums it: lane l of 64 adds k = l, l + 64, ...
            ascending in float64, the 64 partials are combined by the xor butterfly 32, 16, .., 1 (new[l] = old[l] + old[l ^ off]), lane 0
    top_a, top_b   index of the largest pa / pb, the lowest on ties; regret = pb[top_b] - pb[top_a]
    max_dp, k_max  the largest float32(|pa[k] - pb[k]|) and the lowest k that holds it (NaN differences take no part)
    count c; flags bit 0 a non-finite probability on either side, bit 1 c == 0, bit 2 legal_count > L (bit 3: a non-finite value)
A leaf with bit 0 or bit 1 set is counted in nonfinite / empty and enters no sum, maximum or histogram; its tv and regret are 0x7fc00000
(bit 0) or 0 (bit 1).  Histogram: upper edges 1e-7 .. 1e-1, +inf, a leaf goes to the first bucket whose edge exceeds its tv."""

import subprocess
from pathlib import Path

import numpy as np
import pytest

from cattus_amd.build import CSRC

from test_verify_rule import QNAN, _bits, dlogit_restated, dvalue_restated
from test_weight_layout import host_compiler

HERE = Path(__file__).resolve().parent
RECORD = np.dtype([("tv", "<f4"), ("top_a", "<u4"), ("top_b", "<u4"), ("regret", "<f4"), ("max_dp", "<f4"), ("k_max", "<u4"), ("count", "<u2"),
                   ("flags", "<u2"), ("dvalue", "<f4")])
assert RECORD.itemsize == 32
EDGES = [1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1]
COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 218, 1024)


# ---------------------------------------------------------------------------------------- the restatement


def tv_restated(pa, pb, c) -> np.float32:
    """The wave's sum: 64 lane-strided float64 partials, ascending k, then the xor butterfly, lane 0."""
    with np.errstate(all="ignore"):
        d = np.abs(pa[:c].astype(np.float64) - pb[:c].astype(np.float64))
        rows = np.zeros(((c + 63) // 64) * 64, dtype=np.float64)  # + 0.0 leaves a non-negative partial as it is
        rows[:c] = d
        part = np.zeros(64, dtype=np.float64)
        for row in rows.reshape(-1, 64):
            part = part + row
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            part = part + part[lanes ^ off]
        return np.float32(0.5 * part[0])


def _favourite(p) -> int:
    """The lowest index of the largest entry; a NaN takes no part; 0 where nothing is comparable."""
    idx = np.flatnonzero(~np.isnan(p))
    return int(idx[np.argmax(p[idx])]) if len(idx) else 0


def record_restated(pa, pb, legal_count, va, vb) -> np.ndarray:
    pa, pb = np.asarray(pa, dtype=np.float32), np.asarray(pb, dtype=np.float32)
    L = len(pa)
    c = min(int(legal_count), L)
    r = np.zeros((), dtype=RECORD)
    nonfinite = not (np.isfinite(pa[:c]).all() and np.isfinite(pb[:c]).all())
    r["top_a"], r["top_b"] = _favourite(pa[:c]), _favourite(pb[:c])
    d = dlogit_restated(pa[:c], pb[:c])
    d = np.where(np.isnan(d), np.float32(-1), d)
    if c and d.max() > 0:
        r["max_dp"], r["k_max"] = d.max(), d.argmax()
    r["count"] = c
    value_nonfinite = not (np.isfinite(np.float32(va)) and np.isfinite(np.float32(vb)))
    r["flags"] = (1 if nonfinite else 0) | (2 if c == 0 else 0) | (4 if int(legal_count) > L else 0) | (8 if value_nonfinite else 0)
    if nonfinite:
        r["tv"] = r["regret"] = QNAN.view(np.float32)
    elif c:
        r["tv"] = tv_restated(pa, pb, c)
        r["regret"] = pb[int(r["top_b"])] - pb[int(r["top_a"])]  # a float32 difference
    r["dvalue"] = dvalue_restated(va, vb)[0]
    return r


def records_restated(pa, pb, legal_count, va, vb) -> np.ndarray:
    return np.array([record_restated(pa[i], pb[i], legal_count[i], va[i], vb[i]) for i in range(len(pa))], dtype=RECORD)


def bucket_restated(tv) -> int:
    tv = float(np.float32(tv))
    return next((i for i, e in enumerate(EDGES) if tv < e), 7)


def fold_restated(records, into=None) -> dict:
    """The sticky record after these leaves, in order (`holder`: index into `records` of the leaf that now holds max_tv, None if an
    earlier call's stays).  Sums are float64, added leaf by leaf."""
    s = dict(into) if into else dict(leaves=0, top1_flips=0, nonfinite=0, empty=0, sum_tv=0.0, sum_regret=0.0, max_tv=np.float32(0),
                                    max_regret=np.float32(0), tv_hist=[0] * 8, seeded=False)
    s["tv_hist"], s["holder"] = list(s["tv_hist"]), None
    for i, r in enumerate(records):
        s["leaves"] += 1
        if int(r["flags"]) & 1:
            s["nonfinite"] += 1
            continue
        if int(r["flags"]) & 2:
            s["empty"] += 1
            continue
        s["top1_flips"] += int(r["top_a"] != r["top_b"])
        s["sum_tv"] += float(r["tv"])
        s["sum_regret"] += float(r["regret"])
        s["tv_hist"][bucket_restated(r["tv"])] += 1
        if r["regret"] > s["max_regret"]:
            s["max_regret"] = np.float32(r["regret"])
        if not s["seeded"] or r["tv"] > s["max_tv"]:
            s["max_tv"], s["seeded"], s["holder"] = np.float32(r["tv"]), True, i
    return s


def fold_values_restated(va, vb, into=(0, 0.0)):
    """(value_leaves, sum_dvalue) after these pairs: finite pairs only, float64 sum of the float32 |differences|, pair by pair."""
    leaves, total = into
    for a, b in zip(np.asarray(va, dtype=np.float32), np.asarray(vb, dtype=np.float32)):
        if np.isfinite(a) and np.isfinite(b):
            leaves, total = leaves + 1, total + float(dvalue_restated(a, b)[0])
    return leaves, total


# ---------------------------------------------------------------------------------------- the cases


def softmax_rows(rng, n, L, scale=3.0):
    """Two nearby probability rows per leaf: a softmax of random logits and of the same logits perturbed at a bf16-like 2^-8 relative."""
    z = rng.normal(size=(n, L)) * scale
    zb = z * (1 + rng.normal(size=(n, L)) * 2.0 ** -8)
    ea, eb = np.exp(z - z.max(axis=1, keepdims=True)), np.exp(zb - zb.max(axis=1, keepdims=True))
    return (ea / ea.sum(axis=1, keepdims=True)).astype(np.float32), (eb / eb.sum(axis=1, keepdims=True)).astype(np.float32)


def edge_rows(L, seed=0):
    """[(name, pa, pb, legal_count, va, vb)] for stride L: the issue's edge cases at every c of COUNTS that fits."""
    rng = np.random.default_rng(1000 * L + seed)
    out = []
    for c in [c for c in COUNTS if c <= L]:
        pa, pb = softmax_rows(rng, 1, L)
        pa, pb = pa[0], pb[0]
        pa[c:], pb[c:] = 0.0, 0.0
        v = np.float32(np.tanh(rng.normal()))
        out.append((f"random c={c}", pa, pb, c, v, np.float32(v * (1 + 2.0 ** -9))))
    pa, pb = softmax_rows(rng, 1, L)
    pa, pb = pa[0], pb[0]
    out.append(("identical", pb.copy(), pb.copy(), L, np.float32(0.25), np.float32(0.25)))
    out.append(("legal_count > L", pa.copy(), pb.copy(), L + 7, np.float32(-1.0), np.float32(1.0)))
    if L >= 3:
        hi, lo = max(1, L // 2), L - 1  # ties at the maximum on both sides, at different places: the lowest index wins on either
        ta, tb = pa * np.float32(0.5), pb * np.float32(0.5)  # everything else at most 0.5
        ta[[hi, lo]] = 0.75
        tb[[0, hi]] = 0.875
        out.append(("ties", ta, tb, L, np.float32(0.5), np.float32(0.5)))
        sa, sb = np.full(L, 0.0, dtype=np.float32), np.full(L, 0.0, dtype=np.float32)  # two entries swapped, the rest zero
        sa[[0, L - 1]], sb[[0, L - 1]] = (0.75, 0.25), (0.25, 0.75)
        out.append(("swapped", sa, sb, L, np.float32(0.0), np.float32(-0.0)))
        for side in (0, 1):
            for bad in (np.nan, np.inf):
                na, nb = pa.copy(), pb.copy()
                (na, nb)[side][L // 3] = bad
                out.append((f"{bad} on side {side}", na, nb, L, np.float32(np.nan) if side else np.float32(0.1), np.float32(0.1)))
            na, nb = pa.copy(), pb.copy()
            (na, nb)[side][L - 1] = np.nan  # behind the legal moves: never read
            out.append((f"nan behind c on side {side}", na, nb, L - 1, np.float32(0.1), np.float32(np.inf)))
        za, zb = pa.copy(), pb.copy()  # subnormal and zero probabilities, signed zeros
        za[: L // 2] = np.float32(1e-45)
        zb[: L // 2] = np.float32(3e-39)
        za[L // 2], zb[L // 2] = np.float32(-0.0), np.float32(0.0)
        out.append(("subnormal", za, zb, L, np.float32(1e-40), np.float32(0.0)))
        out.append(("all zero", np.zeros(L, dtype=np.float32), np.zeros(L, dtype=np.float32), L, np.float32(1.0), np.float32(1.0)))
    return out


@pytest.fixture(scope="module")
def rule_checks(tmp_path_factory):
    """The stand-alone program, plain and under AddressSanitizer + UBSan (run as programs: no preloading of anything)."""
    d = tmp_path_factory.mktemp("prior_rule")
    exes = []
    for name, extra in (("prior_rule_check", []), ("prior_rule_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / name
        # -ffp-contract=off: as the library itself is built (cattus_amd/build.py)
        subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *extra, f"-I{CSRC}",
                               str(HERE / "prior_rule_check.cpp"), "-o", str(exe)])
        exes.append(exe)
    return exes


def _run(exe, path):
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("prior rule ok"), run.stdout[-3000:] + run.stderr[-3000:]
    return run.stdout.splitlines()[:-1]


def _leaf_line(pa, pb, count, va, vb) -> str:
    return "L %d %d %s %s %s\n" % (count, len(pa), _bits(va), _bits(vb), " ".join("%s %s" % (_bits(x), _bits(y)) for x, y in zip(pa, pb)))


def _words(record) -> str:
    return " ".join("%08x" % w for w in np.frombuffer(record.tobytes(), dtype="<u4"))


def test_leaves_agree_with_the_restatement_plain_and_under_sanitizers(rule_checks, tmp_path):
    cases = [case for L in (1, 2, 9, 25, 64, 65, 218, 224, 1024) for case in edge_rows(L)]
    assert {c[3] for c in cases} >= set(COUNTS)
    (tmp_path / "leaves.txt").write_text("".join(_leaf_line(pa, pb, c, va, vb) for _, pa, pb, c, va, vb in cases))
    want = [record_restated(pa, pb, c, va, vb) for _, pa, pb, c, va, vb in cases]
    by_name = {}
    for (name, pa, *_), w in zip(cases, want):
        by_name.setdefault(name, []).append((len(pa), w))
    # the restatement itself, on the named cases
    for L, w in by_name["identical"]:
        assert w["tv"] == 0 and w["regret"] == 0 and w["top_a"] == w["top_b"] and w["max_dp"] == 0 and w["flags"] == 0 and w["count"] == L
    for L, w in by_name["swapped"]:
        assert w["tv"] == 0.5 and w["top_a"] == 0 and w["top_b"] == L - 1 and w["regret"] == 0.5 and w["max_dp"] == 0.5 and w["k_max"] == 0
    for L, w in by_name["ties"]:
        assert w["top_a"] == max(1, L // 2) and w["top_b"] == 0 and w["regret"] >= 0
    for L, w in by_name["legal_count > L"]:
        assert w["flags"] == 4 and w["count"] == L and w["dvalue"] == 2.0
    for L, w in by_name["random c=0"]:
        assert w["flags"] == 2 and w["tv"] == 0 and w["regret"] == 0 and w["count"] == 0
    for name in ("nan on side 0", "inf on side 0", "nan on side 1", "inf on side 1"):
        for L, w in by_name[name]:
            assert w["flags"] & 1 and w["tv"].view(np.uint32) == QNAN and w["regret"].view(np.uint32) == QNAN and (w["flags"] & 8) == (8 if name[-1] == "1" else 0)
    for side in (0, 1):
        for L, w in by_name[f"nan behind c on side {side}"]:
            assert w["flags"] == 8 and w["count"] == L - 1 and np.isfinite(w["tv"])
    for L, w in by_name["subnormal"] + by_name["all zero"]:
        assert w["flags"] == 0 and np.isfinite(w["tv"]) and w["regret"] >= 0
    assert all(w["regret"] >= 0 for w in want if not w["flags"] & 1)
    assert all((w["regret"] == 0) for w in want if not w["flags"] & 1 and w["top_a"] == w["top_b"])
    for exe in rule_checks:
        rows = _run(exe, tmp_path / "leaves.txt")
        assert len(rows) == len(cases)
        for row, w, c in zip(rows, want, cases):
            assert row == _words(w), (c[0], len(c[1]), row, _words(w), w)


def test_the_sum_is_the_waves_sum_not_the_index_order_sum():
    """The order is part of the rule: on a long row the lane-strided sum and the plain ascending sum differ in float64, and the
    restatement gives the former."""
    rng = np.random.default_rng(3)
    pa, pb = softmax_rows(rng, 1, 1024, scale=6.0)
    d = np.abs(pa[0].astype(np.float64) - pb[0].astype(np.float64))
    part = [sum(d[lane::64].tolist(), 0.0) for lane in range(64)]
    for off in (32, 16, 8, 4, 2, 1):
        part = [part[lane] + part[lane ^ off] for lane in range(64)]
    assert np.float32(0.5 * part[0]) == tv_restated(pa[0], pb[0], 1024)
    assert len(set(part)) == 1  # every lane ends with the same bits: an addition's operands commute
    assert part[0] != sum(d.tolist(), 0.0) or part[0] != float(np.sum(d))


def _record(tv, regret=0.0, top_a=0, top_b=0, flags=0) -> np.ndarray:
    r = np.zeros((), dtype=RECORD)
    r["tv"], r["regret"], r["top_a"], r["top_b"], r["flags"], r["count"] = tv, regret, top_a, top_b, flags, 3
    return r


def fold_sequences():
    f32 = np.float32
    up, down = (lambda x: np.nextafter(f32(x), f32(np.inf))), (lambda x: np.nextafter(f32(x), f32(-np.inf)))
    edges = [_record(t) for e in EDGES for t in (down(e), f32(e), up(e))] + [_record(0.0), _record(1.0)]
    rng = np.random.default_rng(11)
    many = [_record(f32(10.0 ** rng.uniform(-8, 0)), f32(10.0 ** rng.uniform(-6, -1)), int(rng.integers(3)), int(rng.integers(3))) for _ in range(300)]
    return {
        "strictly larger replaces": [_record(0.25), _record(0.125), _record(0.5, 0.25, 1, 2), _record(0.375)],
        "first seen kept on ties": [_record(0.0), _record(0.0), _record(0.5, 0.125, 0, 1), _record(0.5, 0.125, 0, 1), _record(0.5)],
        "flagged leaves enter nothing": [_record(0.9, 0.9, 0, 1, flags=1), _record(0.9, 0.9, 0, 1, flags=2), _record(0.25, flags=4), _record(0.125, flags=8)],
        "only flagged": [_record(0.9, flags=1), _record(0.0, flags=2)],
        "edges": edges,
        "many": many,
        "empty": [],
    }


def test_fold_agrees_with_the_restatement_plain_and_under_sanitizers(rule_checks, tmp_path):
    seqs = fold_sequences()
    names = sorted(seqs)
    (tmp_path / "folds.txt").write_text("".join("F " + " ".join(_words(r) for r in seqs[n]) + "\n" for n in names)
                                        + "V " + " ".join("%s %s" % (_bits(a), _bits(b)) for a, b in value_pairs()) + "\n")
    want = {n: fold_restated(seqs[n]) for n in names}
    # the restatement itself
    assert want["strictly larger replaces"]["holder"] == 2 and want["strictly larger replaces"]["max_tv"] == 0.5
    assert want["first seen kept on ties"]["holder"] == 2 and want["first seen kept on ties"]["top1_flips"] == 2
    w = want["flagged leaves enter nothing"]
    assert (w["leaves"], w["nonfinite"], w["empty"], w["top1_flips"], w["sum_tv"], w["holder"]) == (4, 1, 1, 0, 0.375, 2) and w["max_regret"] == 0
    assert want["only flagged"]["holder"] is None and not want["only flagged"]["seeded"] and want["empty"]["leaves"] == 0
    # a tv that equals an edge, as nearly as a float32 can, goes where float64 puts it; one ulp either side is unambiguous
    for k, e in enumerate(EDGES):
        below, at, above = (bucket_restated(t) for t in (np.nextafter(np.float32(e), np.float32(0)), np.float32(e), np.nextafter(np.float32(e), np.float32(1))))
        assert below == k and above == k + 1 and at == (k if float(np.float32(e)) < e else k + 1)
    assert sum(want["edges"]["tv_hist"]) == len(seqs["edges"]) and all(want["edges"]["tv_hist"])
    vl, sv = fold_values_restated(*zip(*value_pairs()))
    assert vl == len(value_pairs()) - 4
    for exe in rule_checks:
        rows = _run(exe, tmp_path / "folds.txt")
        assert len(rows) == len(names) + 1
        for n, row in zip(names, rows):
            g, w = row.split(), want[n]
            assert [int(x) for x in g[:4]] == [w["leaves"], w["top1_flips"], w["nonfinite"], w["empty"]], (n, row, w)
            assert g[4] == np.float64(w["sum_tv"]).tobytes()[::-1].hex() and g[5] == np.float64(w["sum_regret"]).tobytes()[::-1].hex(), (n, row, w)
            assert g[6] == _bits(w["max_tv"]) and g[7] == _bits(w["max_regret"]), (n, row, w)
            assert [int(x) for x in g[8:16]] == w["tv_hist"], (n, row, w)
            assert int(g[16]) == (-1 if w["holder"] is None else w["holder"]), (n, row, w)
        g = rows[-1].split()
        assert int(g[0]) == vl and g[1] == np.float64(sv).tobytes()[::-1].hex()


def value_pairs():
    rng = np.random.default_rng(2)
    v = np.tanh(rng.normal(size=40)).astype(np.float32)
    pairs = [(a, np.float32(a * (1 + 2.0 ** -9))) for a in v]
    pairs += [(np.float32(np.nan), np.float32(0)), (np.float32(0), np.float32(np.inf)), (np.float32(np.inf), np.float32(np.inf)),
              (np.float32(-np.inf), np.float32(0.5)), (np.float32(1.0), np.float32(-1.0)), (np.float32(0.0), np.float32(-0.0))]
    return pairs
