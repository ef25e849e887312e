"""The observation layouts and the trace record's rule without a GPU: cattus_amd/csrc/tap_layout.h against numpy restatements.

tests/tap_layout_check.cpp is a stand-alone program around the header (the kernels of cattus_hip_tap / cattus_hip_trace include the same
file).  It is built with the host compiler twice -- plain, and with -fsanitize=address,undefined -- and both are run as programs on a
file of cases this test writes.

Layouts.  For every source layout an evaluator can hold the test builds a buffer in which the element of (leaf,
channel, pixel) holds a value made from its own coordinates -- a hash of them as the bits of the stored type, so that bf16's eight bits
are enough -- at the address the restatement below gives, and 0xff bytes (NaNs) everywhere else: unused pixel slots, padding channels,
padding leaves.  The program decodes it through tap_layout.h into f32 [n][C][S*S]; that must be the NCHW array exactly, with the
channels' shifts divided out.  The buffer is read into an allocation of exactly its size, so an address outside it fails under the
sanitizer build.

Records.  Leaves travel as the hex of their floats' bits; the program's 32 bytes per leaf are compared with a float64 restatement of
the rule (include/cattus_hip.h, cattus_trace_record), byte for byte.
"""

import subprocess
from pathlib import Path

import numpy as np
import pytest

from cattus_amd.build import CSRC
from cattus_amd.evaluator import TRACE_RECORD

from test_weight_layout import host_compiler

HERE = Path(__file__).resolve().parent
ROWS_F32, ROWS_BF16, ROWS_F16, ROWS_F16X2, ROWS_WINO_F32, NCHW_F32, HV_F32, HV_BF16 = range(8)  # tap_layout.h, TapLayout
QNAN = 0x7FC00000


@pytest.fixture(scope="module")
def layout_checks(tmp_path_factory):
    """The stand-alone program, plain and under AddressSanitizer + UBSan (run as programs: no preloading of anything)."""
    d = tmp_path_factory.mktemp("tap_layout")
    exes = []
    for name, extra in (("tap_layout_check", []), ("tap_layout_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / name
        # -ffp-contract=off: as the library itself is built (cattus_amd/build.py)
        subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *extra, f"-I{CSRC}",
                               str(HERE / "tap_layout_check.cpp"), "-o", str(exe)])
        exes.append(exe)
    return exes


def _run(exe, path):
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("tap layout ok"), run.stdout[-3000:] + run.stderr[-3000:]
    return run.stdout.splitlines()[:-1]


# ---------------------------------------------------------------------------------------- the layouts, restated


def _coords(n, C, hw):
    return np.ogrid[0:n, 0:C, 0:hw]


def rows_offset(layout, n, C, hw, slots, pitch):
    """Byte offset [n, C, hw] of the stored element (the hi half for f16x2; lo is 64 bytes behind it) in tower rows: row = leaf * slots +
    pixel, `pitch` channels per row."""
    leaf, c, p = _coords(n, C, hw)
    row = leaf * slots + p
    if layout in (ROWS_F32, ROWS_WINO_F32):
        return (row * pitch + c) * 4
    if layout in (ROWS_BF16, ROWS_F16):
        return (row * pitch + c) * 2
    assert layout == ROWS_F16X2  # 128 bytes per 32 channels: [32 hi | 32 lo]
    return row * pitch * 4 + (c // 32) * 128 + (c % 32) * 2


def nchw_offset(n, C, hw):
    leaf, c, p = _coords(n, C, hw)
    return ((leaf * C + c) * hw + p) * 4


def hv_offset(esz, n, vhc, phc, hw, kvp, kpp, hv_pol):
    """The heads' activations: value matrix [leaf][kvp] at element 0, policy matrix [leaf][kpp] at element hv_pol, each in MFMA fragment
    order -- KSTEP = 32 bytes of k, HALF = KSTEP / 2 (kernels.h, HeadsMfma)."""
    leaf, c, p = _coords(n, vhc + phc, hw)
    kstep, half = 32 // esz, 16 // esz
    value = c < vhc
    k = np.where(value, c * hw + p, (c - vhc) * hw + p)
    K = np.where(value, kvp, kpp)
    at = ((((leaf // 32) * (K // kstep) + k // kstep) * 2 + (k % kstep) // half) * 32 + leaf % 32) * half + k % half
    return (np.where(value, 0, hv_pol) + at) * esz


def _hash(n, C, hw, salt):
    leaf, c, p = _coords(n, C, hw)
    h = (leaf * 1000003 + c * 7919 + p * 104729 + salt * 15485863 + 12345).astype(np.uint64)
    h = (h * np.uint64(2654435761)) % np.uint64(1 << 32)
    return (h ^ (h >> np.uint64(13))).astype(np.uint32)


def f16_bits(n, C, hw, salt):
    """A finite f16 per coordinate (exponent field 0..30: subnormals included), as uint16."""
    h = _hash(n, C, hw, salt)
    return ((h & 0x83FF) | (((h >> 10) % 31) << 10)).astype(np.uint16)


def bf16_bits(n, C, hw, salt):
    """A finite bf16 of exponent 2^-20 .. 2^20 per coordinate, as uint16."""
    h = _hash(n, C, hw, salt)
    return ((h & 0x807F) | ((107 + (h >> 8) % 41) << 7)).astype(np.uint16)


def f32_bits(n, C, hw, salt):
    h = _hash(n, C, hw, salt)
    return ((h & np.uint32(0x807FFFFF)) | ((np.uint32(107) + (h >> np.uint32(23)) % np.uint32(41)) << np.uint32(23))).astype(np.uint32)


def _scatter(buf, dtype, offsets, values):
    view = buf.view(dtype)
    esz = np.dtype(dtype).itemsize
    assert (offsets % esz == 0).all() and offsets.max() + esz <= buf.size
    flat = (offsets // esz).ravel()
    assert len(np.unique(flat)) == flat.size  # no two elements share an address
    view[flat] = values.ravel()


def build_case(layout, n, C, hw, shifts, slots=0, pitch=0, heads=None, salt=0):
    """(buffer bytes, expected f32 [n, C, hw], the TapSource fields) of one tensor."""
    src = dict(layout=layout, C=C, hw=hw, slots=slots, pitch=pitch, vhc=0, kvp=0, kpp=0, hv_pol=0)
    if layout in (HV_F32, HV_BF16):
        vhc, phc = heads
        esz = 4 if layout == HV_F32 else 2
        kvp, kpp, leaves = -(-vhc * hw // 16) * 16, -(-phc * hw // 16) * 16, -(-n // 32) * 32
        src.update(vhc=vhc, kvp=kvp, kpp=kpp, hv_pol=leaves * kvp)
        buf = np.full(leaves * (kvp + kpp) * esz, 0xFF, dtype=np.uint8)
        off = hv_offset(esz, n, vhc, phc, hw, kvp, kpp, leaves * kvp)
    elif layout == NCHW_F32:
        buf = np.full(n * C * hw * 4, 0xFF, dtype=np.uint8)
        off = nchw_offset(n, C, hw)
    else:
        esz = 2 if layout in (ROWS_BF16, ROWS_F16) else 4
        buf = np.full(n * slots * pitch * esz, 0xFF, dtype=np.uint8)
        off = rows_offset(layout, n, C, hw, slots, pitch)
    if layout == ROWS_F16X2:
        hi, lo = f16_bits(n, C, hw, salt), f16_bits(n, C, hw, salt + 1)
        _scatter(buf, np.uint16, off, hi)
        _scatter(buf, np.uint16, off + 64, lo)
        value = hi.view(np.float16).astype(np.float32) + lo.view(np.float16).astype(np.float32)  # one f32 addition
    elif layout == ROWS_F16:
        bits = f16_bits(n, C, hw, salt)
        _scatter(buf, np.uint16, off, bits)
        value = bits.view(np.float16).astype(np.float32)
    elif layout in (ROWS_BF16, HV_BF16):
        bits = bf16_bits(n, C, hw, salt)
        _scatter(buf, np.uint16, off, bits)
        value = (bits.astype(np.uint32) << 16).view(np.float32)
    else:
        bits = f32_bits(n, C, hw, salt)
        _scatter(buf, np.uint32, off, bits)
        value = bits.view(np.float32)
    if shifts is not None:
        scaled = value.astype(np.float64) * np.ldexp(1.0, -np.asarray(shifts))[None, :, None]
        value = scaled.astype(np.float32)
        assert (value.astype(np.float64) == scaled).all()  # a power of two: exact
    return buf, np.ascontiguousarray(value, dtype=np.float32), src


def layout_cases():
    cases = []
    salt = 0
    for S in (3, 7, 8, 11):
        hw, slots = S * S, 64 if S <= 8 else 128
        for F in (1, 16, 64, 96, 128):
            pitch = -(-F // 64) * 64
            for n in (1, 3, 5):
                shifts = [(3 * k) % 17 - 4 if k % 3 else 0 for k in range(F)]  # non-zero on two channels of three, either sign
                for layout in (ROWS_F32, ROWS_BF16, ROWS_F16, ROWS_F16X2) + ((ROWS_WINO_F32,) if S == 8 else ()):
                    salt += 1
                    cases.append(build_case(layout, n, F, hw, shifts if salt % 2 else None, slots=slots, pitch=pitch, salt=salt) + (shifts if salt % 2 else None,))
                salt += 1
                cases.append(build_case(NCHW_F32, n, F, hw, None, salt=salt) + (None,))
        for heads in ((1, 1), (8, 8), (16, 16)):
            for n in (1, 3, 5, 37):  # 37: a second 32-leaf tile of the fragment order
                for layout in (HV_F32, HV_BF16):
                    salt += 1
                    cases.append(build_case(layout, n, sum(heads), hw, None, heads=heads, salt=salt) + (None,))
    return cases


def test_every_layout_decodes_to_the_nchw_array_plain_and_under_sanitizers(layout_checks, tmp_path):
    cases = layout_cases()
    assert any(s["kvp"] != s["vhc"] * s["hw"] for _, _, s, _ in cases)  # K of a head is no multiple of 16 somewhere: pad columns exist
    assert {s["layout"] for _, _, s, _ in cases} == set(range(8))
    lines = []
    for i, (buf, want, s, shifts) in enumerate(cases):
        buf.tofile(tmp_path / f"in{i}.bin")
        fields = [s[k] for k in ("layout", "C", "hw", "slots", "pitch", "vhc", "kvp", "kpp", "hv_pol")]
        lines.append("T %s %d %s %s %d %s" % (" ".join(map(str, fields)), want.shape[0], tmp_path / f"in{i}.bin", tmp_path / f"out{i}.bin",
                                             len(shifts or []), " ".join(map(str, shifts or []))))
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    for exe in layout_checks:
        assert _run(exe, tmp_path / "cases.txt") == []
        for i, (_, want, s, _) in enumerate(cases):
            got = np.fromfile(tmp_path / f"out{i}.bin", dtype=np.uint32)
            assert got.size == want.size and (got == want.view(np.uint32).ravel()).all(), (exe.name, s, want.shape)
            (tmp_path / f"out{i}.bin").unlink()


# ---------------------------------------------------------------------------------------- the record, restated


def record_restated(x, ref) -> np.ndarray:
    """One leaf's record in float64 numpy, elements in index order (cumsum adds in that order, as the program's loop does)."""
    x, ref = np.asarray(x, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    words = np.zeros(8, dtype=np.uint32)  # the record's eight 32-bit words
    f32 = words.view(np.float32)
    with np.errstate(all="ignore"):
        d = x.astype(np.float64) - ref.astype(np.float64)
        diff = np.abs(d).astype(np.float32)
        diff = np.where(np.isnan(diff), np.float32(-1), diff)
        at = int(diff.argmax()) if diff.max() > 0 else 0  # argmax: the first index that holds the maximum
        f32[0] = diff[at] if diff.max() > 0 else 0
        words[1], words[2], words[3] = at, x.view(np.uint32)[at], ref.view(np.uint32)[at]
        r64 = ref.astype(np.float64)
        for word, terms in ((4, d * d), (5, r64 * r64)):
            f32[word] = np.sqrt(np.cumsum(terms)[-1] / float(len(x)))
            if np.isnan(f32[word]):
                words[word] = QNAN
    words[6] = int(not (np.isfinite(x).all() and np.isfinite(ref).all()))
    return words.view(TRACE_RECORD)[0]


def record_cases():
    rng = np.random.default_rng(23)
    cases = []
    for count in (1, 2, 9, 64, 49 * 16, 121 * 5):
        for k in range(8):
            ref = (rng.standard_normal(count) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32)
            x = (ref.astype(np.float64) * (1 + rng.standard_normal(count) * 1e-3) + rng.standard_normal(count) * 1e-5).astype(np.float32)
            if k == 1:
                x = ref.copy()  # all equal
            if k == 2 and count >= 3:
                x = ref.copy()
                ref[[count - 1, count // 2]] = np.float32(0.25)  # one maximum at two indices: the lower one is reported
                x[[count - 1, count // 2]] = np.float32(0.75)
            if k == 3:
                x[rng.integers(count)] = np.nan
            if k == 4:
                ref[rng.integers(count)] = np.nan
            if k == 5:
                x[rng.integers(count)] = np.inf
                ref[rng.integers(count)] = -np.inf
            if k == 6:
                i = rng.integers(count)
                x[i] = ref[i] = np.inf  # two equal infinities: a NaN difference that takes no part
            if k == 7:
                x, ref = ref, np.zeros(count, dtype=np.float32)
                x[0] = -0.0
            cases.append((x, ref))
    return cases


def test_records_agree_with_the_restatement_plain_and_under_sanitizers(layout_checks, tmp_path):
    cases = record_cases()
    bits = lambda a: a.view(np.uint32)
    (tmp_path / "records.txt").write_text("".join("R %d %s\n" % (len(x), " ".join("%08x %08x" % (a, b) for a, b in zip(bits(x), bits(r)))) for x, r in cases))
    want = [record_restated(x, r) for x, r in cases]
    # the cases do hold what they are meant to: ties at the lower index, records without a positive difference, non-finite ones
    for (x, _), w in list(zip(cases, want))[2::8]:
        if len(x) >= 3:
            assert w["max_diff"] == 0.5 and w["at"] == len(x) // 2, (len(x), w)
    assert any(w["max_diff"] == 0 and w["at"] == 0 for w in want) and any(np.isinf(w["max_diff"]) for w in want)
    assert any(w["flags"] == 1 and w["rms_diff"].view(np.uint32) == QNAN for w in want) and any(w["flags"] == 0 for w in want)
    assert any(w["flags"] == 1 and np.isfinite(w["max_diff"]) for w in want)
    for exe in layout_checks:
        rows = _run(exe, tmp_path / "records.txt")
        assert len(rows) == len(cases)
        for row, w, (x, _) in zip(rows, want, cases):
            got = np.array([int(v, 16) for v in row.split()], dtype=np.uint32).view(TRACE_RECORD)[0]
            assert got.tobytes() == w.tobytes(), (got, w, len(x))
