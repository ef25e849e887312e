"""The ragged layout of the leaf server's legal-move lists without a GPU: cattus_amd/csrc/legal_span.h against a numpy restatement.

tests/legal_span_check.cpp is a stand-alone program around the header.  It is built with the host compiler twice -- plain, and with
-fsanitize=address,undefined -- and both are run as programs on a file of cases this test writes.  The header is what the server's
append, legal_softmax_ragged_kernel, verify_priors_kernel's row offsets and the evaluator's fold share; test_server_legal_gpu.py holds
those to it on the device.

The layout: the leaves of a batch keep their policy indices back to back, off [n + 1] with off[0] == 0 marks where each list starts;
leaf i owns [off[i], off[i + 1]).  A list has at most 1024 entries, every one < moves; a table starts at 0 and never descends."""

import subprocess
from pathlib import Path

import numpy as np
import pytest

from cattus_amd.build import CSRC

from test_weight_layout import host_compiler

HERE = Path(__file__).resolve().parent
OK, TOO_LONG, BAD_INDEX, BAD_OFFSETS = 0, 1, 2, 3
MOVES = 1880


@pytest.fixture(scope="module")
def span_checks(tmp_path_factory):
    """The stand-alone program, plain and under AddressSanitizer + UBSan (run as programs: no preloading of anything)."""
    d = tmp_path_factory.mktemp("legal_span")
    exes = []
    for name, extra in (("legal_span_check", []), ("legal_span_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / name
        subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", *extra, f"-I{CSRC}", str(HERE / "legal_span_check.cpp"), "-o", str(exe)])
        exes.append(exe)
    return exes


def _run(exe, path):
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("legal span ok"), run.stdout[-3000:] + run.stderr[-3000:]
    return run.stdout.splitlines()[:-1]


# ---------------------------------------------------------------------------------------- the restatement


def list_fault(idx, moves):
    if len(idx) > 1024:
        return TOO_LONG, 0
    bad = np.flatnonzero(np.asarray(idx, dtype=np.int64) >= moves)
    return (BAD_INDEX, int(bad[0])) if len(bad) else (OK, 0)


def offsets_fault(off):
    off = [int(o) for o in off]
    if off[0] != 0:
        return BAD_OFFSETS, 0
    for i in range(len(off) - 1):
        if off[i + 1] < off[i]:
            return BAD_OFFSETS, i
        if off[i + 1] - off[i] > 1024:
            return TOO_LONG, i
    return OK, 0


def appended(leaves, submits):
    """The table of a batch of `leaves` leaves of which `submits` = [(slot, count)], slots ascending, came with a list."""
    counts = np.zeros(leaves, dtype=np.int64)
    for slot, count in submits:
        counts[slot] = count
    return [0] + np.cumsum(counts).tolist()


def owners(off):
    return (np.searchsorted(np.asarray(off), np.arange(off[-1]), side="right") - 1).tolist()


# ---------------------------------------------------------------------------------------- the cases


def list_cases():
    rng = np.random.default_rng(5)
    cases = [(MOVES, rng.permutation(MOVES)[:c]) for c in (0, 1, 63, 64, 65, 218, 1023, 1024, 1025)]
    for c, at in ((1, 0), (1024, 1023), (218, 100), (1024, 0)):  # an index equal to moves: first, last, inside
        idx = rng.permutation(MOVES)[:c]
        idx[at] = MOVES
        cases.append((MOVES, idx))
    two = rng.permutation(MOVES)[:9]
    two[[3, 7]] = (MOVES + 5, 65535)  # the first offender is reported
    cases += [(MOVES, two), (9, np.arange(9)), (9, np.arange(10)), (65535, np.array([65534])), (1, np.zeros(1025, dtype=np.int64))]
    return cases


def offset_cases():
    return [
        [0], [0, 0], [0, 0, 0, 0], [0, 1], [0, 1024], [0, 1025], [0, 1024, 2048, 2048, 2049], [0, 0, 1, 64, 128, 193, 411, 1434, 2458],
        [1], [1, 2, 3], [5, 5], [0, 5, 4, 9], [0, 3, 3, 2], [0, 10, 0], [0, 4, 1029, 1030], [0, 2000, 1990],  # the first offending leaf is reported: too long, before the descent behind it
        [0, 4294967295],
    ]


def append_cases():
    rng = np.random.default_rng(6)
    cases = [(1, [(0, 0)]), (1, [(0, 1024)]), (3, []), (8, [(s, c) for s, c in enumerate((0, 1, 63, 64, 65, 218, 1023, 1024))]),
             (8, [(1, 5), (3, 0), (5, 7), (7, 1)]), (8, [(0, 3), (2, 4), (4, 0), (6, 9)]), (5, [(4, 2)]), (5, [(0, 2)]), (256, [(s, 1024) for s in range(256)])]
    for _ in range(20):
        leaves = int(rng.integers(1, 40))
        slots = sorted(rng.choice(leaves, size=int(rng.integers(0, leaves + 1)), replace=False).tolist())
        cases.append((leaves, [(s, int(rng.choice([0, 1, 2, 30, 64, 1024]))) for s in slots]))
    return cases


def test_lists_tables_appends_and_owners_plain_and_under_sanitizers(span_checks, tmp_path):
    lists, tables, appends = list_cases(), offset_cases(), append_cases()
    walks = [t for t in tables if offsets_fault(t)[0] == OK] + [appended(leaves, subs) for leaves, subs in appends if leaves <= 40]
    text = "".join("L %d %d %s\n" % (m, len(idx), " ".join(str(int(i)) for i in idx)) for m, idx in lists)
    text += "".join("O %d %s\n" % (len(t) - 1, " ".join(map(str, t))) for t in tables)
    text += "".join("A %d %d %s\n" % (leaves, len(subs), " ".join("%d %d" % sc for sc in subs)) for leaves, subs in appends)
    text += "".join("W %d %s\n" % (len(t) - 1, " ".join(map(str, t))) for t in walks)
    (tmp_path / "cases.txt").write_text(text)
    # the restatement itself, on the issue's named cases
    assert [list_fault(idx, m)[0] for m, idx in lists[:9]] == [OK] * 8 + [TOO_LONG]
    assert [list_fault(idx, m) for m, idx in lists[9:14]] == [(BAD_INDEX, 0), (BAD_INDEX, 1023), (BAD_INDEX, 100), (BAD_INDEX, 0), (BAD_INDEX, 3)]
    assert offsets_fault([1, 2, 3]) == (BAD_OFFSETS, 0) and offsets_fault([0, 5, 4, 9]) == (BAD_OFFSETS, 1) and offsets_fault([0, 1025]) == (TOO_LONG, 0)
    assert offsets_fault([0, 0, 0, 0]) == (OK, 0) and owners([0, 0, 0, 0]) == []  # total == 0: nobody owns anything
    assert owners([0, 0, 3, 3, 4]) == [1, 1, 1, 3]
    assert appended(5, [(1, 3), (3, 1)]) == [0, 0, 3, 3, 4, 4]
    want = ["%d %d" % list_fault(idx, m) for m, idx in lists] + ["%d %d" % offsets_fault(t) for t in tables]
    want += ["%d %s" % (appended(leaves, subs)[-1], " ".join(map(str, appended(leaves, subs)))) for leaves, subs in appends]
    want += [" ".join(map(str, owners(t))) for t in walks]
    for exe in span_checks:
        rows = _run(exe, tmp_path / "cases.txt")
        assert len(rows) == len(want)
        for k, (row, w) in enumerate(zip(rows, want)):
            assert row == w, (k, row[:200], w[:200])
