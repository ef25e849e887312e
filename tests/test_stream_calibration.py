"""Stream shifts from measured activations, the part without a GPU: the rule, and the network that the estimate misses.

The rule.  weight_layout.h's calibrated_stream_shifts is stream_shifts fed with measured mean squares, then a headroom guard (t_k drops
while t_k > 0 and abs_max_k 2^t_k > 4096).  tests/calibration_rule_check.cpp checks its fixed points itself and prints what it gives on
the cases written here; calibrated_shifts_restated below says the same in Python and must agree on all of them: dead and non-finite
channels, the median rule, lifting into [1, 2), the cap 16, abs_max 2^t just under / at / just over 4096, a guard that stops at 0, a
guarded channel below the global shift, and a random sweep.  test_stream_calibration_gpu.py holds the evaluator to this restatement.

The hidden twin.  stream_shifts' input is an estimate: s_k^2 = the sum of gamma^2 + beta^2 over the BatchNorms that write stream
channel k.  hidden_twin scales what the estimate does not look at -- for every writer of channel k the conv's output row k, the
BatchNorm's running_mean[k] and beta_k by c_k = 2^e_k, gamma_k and running_var[k] left alone; the readers' input weights by 1 / c_k as
helpers.channel_twin does.  BatchNorm(c conv(x)) with mean c mu and the old variance is c (conv(x) - mu) / sqrt(var + eps) gamma + c beta:
the function of channel_twin, and since every product is by a power of two it folds to the same f32 numbers, so (a) the CPU oracle gives
the same bits for both twins; but (b) the estimate sees s_k >= gamma_stem >= 0.75 on every channel and shifts nothing, while the hidden
channels of the Q8 pattern run at 2^-8.  Both are checked on hex7_6x64 and chess2x128 as test_split_range_gpu.py seeds them (SEED 41:
(b) holds on it, no other seed was needed), which keeps the GPU test's inputs inside their own premises."""

import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from cattus_amd.build import CSRC
from cattus_amd.weights import NetDesc, pack_tensors, seeded_tensors
from oracle import oracle

from helpers import CHANNEL_PATTERNS, F32_MAX, F32_MIN_NORMAL, channel_twin
from test_channel_scale_gpu import expected_stream_shifts
from test_f16_tower_gpu import random_planes
from test_split_range_gpu import SEED, desc_of, expected_stream_shift
from test_weight_layout import host_compiler

HERE = Path(__file__).resolve().parent
STREAM_SHIFT_MAX, HEADROOM = 16, 4096.0


def _ilogb(x: float) -> int:
    return math.frexp(x)[1] - 1


def global_shift_restated(s2) -> int:
    """stream_shift_global: S = sqrt(median s2); 0 for S >= 1/2, for S = 0 or not finite and for no channels, else -floor(log2 S), at most 16."""
    s2 = np.asarray(s2, dtype=np.float64)
    if not s2.size:
        return 0
    S = math.sqrt(float(np.median(s2)))
    if not (S > 0 and math.isfinite(S)) or S >= 0.5:
        return 0
    return min(STREAM_SHIFT_MAX, -_ilogb(S))


def calibrated_shifts_restated(rms, abs_max, headroom: float = HEADROOM) -> tuple[int, np.ndarray]:
    """(global shift, t_k per channel) of calibrated_stream_shifts on s2 = rms^2 in float64 (rms, abs_max: what stream_range returns).
    headroom: the guard's bound, 4096 unless the tower is the F(4x4, 3x3) form (163.75, test_winof4_range_gpu.py)."""
    rms, abs_max = np.asarray(rms, dtype=np.float64), np.asarray(abs_max, dtype=np.float64)
    return shifts_of_s2(rms * rms, abs_max, headroom)


def shifts_of_s2(s2, abs_max, headroom: float = HEADROOM) -> tuple[int, np.ndarray]:
    glob = global_shift_restated(s2)
    out = []
    for s2k, mx in zip(s2, abs_max):
        s = math.sqrt(s2k)
        stays = not (s > 0 and math.isfinite(s)) or math.ldexp(s, glob) >= 0.5
        t = glob if stays else min(STREAM_SHIFT_MAX, -_ilogb(s))
        while t > 0 and mx * 2.0**t > headroom:
            t -= 1
        out.append(t)
    return glob, np.array(out, dtype=np.int64)


def _sq(v):
    return [x * x for x in v]


# (what, s2, abs_max, global shift, t_k): the named cases of the issue, with what the rule must give written out
NAMED = [
    ("a unit median, one channel at 2^-8, one dead, one at 2^-3", _sq([1.0, 1.5 * 2.0**-8, 0.0, 2.0, 2.0**-3, 1.0]), [4.0, 2.0**-6, 0.0, 8.0, 0.5, 4.0], 0, [0, 8, 0, 0, 3, 0]),
    ("the median rule: a small median lifts everything, a dead channel with it", _sq([1.5 * 2.0**-8, 1.0, 1.5 * 2.0**-8, 0.0, 1.5 * 2.0**-12, 1.5 * 2.0**-8, 1.5 * 2.0**-8]),
     [2.0**-6, 4.0, 2.0**-6, 0.0, 2.0**-10, 2.0**-6, 2.0**-6], 8, [8, 8, 8, 8, 12, 8, 8]),
    ("an even count: the median is the mean of the middle two", _sq([2.0**-4, 2.0**-4, 1.0, 1.0]), [0.1, 0.1, 2.0, 2.0], 0, [4, 4, 0, 0]),
    ("lifted into [1, 2): 0.99 x 2^-8 needs 9, 1.99 x 2^-8 needs 8", _sq([0.99 * 2.0**-8, 1.99 * 2.0**-8, 1.0, 1.0, 1.0]), [0.01, 0.01, 1.0, 1.0, 1.0], 0, [9, 8, 0, 0, 0]),
    ("just below 1/2 moves, 1/2 stays", _sq([0.49, 0.5, 1.0]), [1.0, 1.0, 1.0], 0, [2, 0, 0]),
    ("the cap", _sq([2.0**-30]), [2.0**-28], 16, [16]),
    ("a non-finite channel is left at the global shift", [1.0, math.inf, 2.0**-16, 1.0], [1.0, 1.0, 2.0**-7, 1.0], 0, [0, 0, 8, 0]),
    ("nothing to go by", [math.nan], [1.0], 0, [0]),
    ("the guard: at 4096 and just under it stays, just over it drops by one", _sq([2.0**-8] * 3 + [1.0] * 4),
     [16.0, float(np.nextafter(16.0, 0.0)), float(np.nextafter(16.0, 17.0)), 1.0, 1.0, 1.0, 1.0], 0, [8, 8, 7, 0, 0, 0, 0]),
    ("the guard drops until it fits and stops at 0", _sq([2.0**-8] * 3 + [1.0] * 4), [33.0, 1e9, math.inf, 1e9, 1.0, 1.0, 1.0], 0, [6, 0, 0, 0, 0, 0, 0]),
    ("a guarded channel below the global shift", _sq([1.5 * 2.0**-8, 1.0, 1.5 * 2.0**-8]), [0.05, 20.0, 0.05], 8, [8, 7, 8]),
]


def random_cases(count: int):
    rng = np.random.default_rng(11)
    for _ in range(count):
        F = int(rng.integers(1, 10))
        s = 2.0 ** rng.uniform(-20, 4, F) * (rng.random(F) > 0.1)  # one channel in ten dead
        mx = s * 2.0 ** rng.uniform(0, 14, F)  # up to 2^14 x rms, a lifted channel's 2^t above that: a fair share meets the guard
        yield list(s * s), list(mx)


@pytest.fixture(scope="module")
def rule_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("calibration_rule") / "calibration_rule_check"
    # -ffp-contract=off: as the library itself is built (cattus_amd/build.py)
    subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", f"-I{CSRC}", str(HERE / "calibration_rule_check.cpp"), "-o", str(exe)])
    return exe


def test_the_rule_holds_its_fixed_points_and_agrees_with_the_restatement(rule_check, tmp_path):
    cases = [(s2, mx) for _, s2, mx, _, _ in NAMED] + list(random_cases(300))
    text = "".join("%d %s\n" % (len(s2), " ".join(float(x).hex() for x in list(s2) + list(mx))) for s2, mx in cases)
    (tmp_path / "cases.txt").write_text(text)
    run = subprocess.run([str(rule_check), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and "calibration rule ok" in run.stdout, run.stdout[-4000:] + run.stderr[-2000:]
    rows = [[int(x) for x in line.split()] for line in run.stdout.splitlines()[: len(cases)]]
    assert len(rows) == len(cases)
    for (what, s2, mx, glob, tk), row in zip(NAMED, rows):
        assert row == [glob, *tk], (what, row)
    guarded = 0
    for (s2, mx), row in zip(cases, rows):
        glob, tk = shifts_of_s2(s2, mx)
        assert row == [glob, *tk], (s2, mx, row, glob, tk)
        guarded += int((tk < shifts_of_s2(s2, [0.0] * len(s2))[1]).sum())
    assert guarded > 50  # the sweep does meet the guard


def test_the_restatement_takes_rms_as_the_evaluator_reports_it():
    rms = np.array([1.0, 1.5 * 2.0**-8, 0.0, 1.0, 2.0], dtype=np.float32)
    glob, tk = calibrated_shifts_restated(rms, np.array([3.0, 0.1, 0.0, 3.0, 5.0], dtype=np.float32))
    assert glob == 0 and list(tk) == [0, 8, 0, 0, 0]


def hidden_twin(desc: NetDesc, tensors: dict, exponents) -> dict:
    """The tensors of a network that computes the function of helpers.channel_twin(desc, tensors, exponents) -- stream channel k x
    c_k = 2^exponents[k] -- with the scale where the estimate of stream_shifts does not look: for every writer of the stream (the stem
    and every block's _conv2 + _bn2) output row k of the conv, running_mean[k] and beta_k x c_k, gamma_k and running_var[k] as they are;
    for every reader (every block's _conv1, both head convs) input channel k / c_k, as channel_twin does.  Powers of two: exact, and a
    product that leaves the f32 normal range raises."""
    e = np.asarray(exponents)
    if e.shape != (desc.filters,) or not np.issubdtype(e.dtype, np.integer):
        raise ValueError(f"hidden_twin: want {desc.filters} integer exponents, got {e.dtype} {e.shape}")
    c = np.ldexp(1.0, e.astype(np.int64))
    out = dict(tensors)

    def scaled(k, factor):
        x = np.asarray(tensors[k], dtype=np.float64) * factor
        a = np.abs(x[x != 0])
        if a.size and not (a.min() >= F32_MIN_NORMAL and a.max() <= F32_MAX):
            raise ValueError(f"hidden_twin: {k} leaves the f32 normal range")
        out[k] = x.astype(np.float32)

    writers = [("_conv1._conv.weight", "_conv1._bn.")] + [(f"_residual_blocks.{i}._conv2.weight", f"_residual_blocks.{i}._bn2.") for i in range(desc.blocks)]
    for conv, bn in writers:
        scaled(conv, c.reshape(-1, 1, 1, 1))
        scaled(bn + "running_mean", c)
        scaled(bn + "bias", c)
    readers = [f"_residual_blocks.{i}._conv1.weight" for i in range(desc.blocks)] + ["_value_head.0._conv.weight", "_policy_head.0._conv.weight"]
    for k in readers:
        scaled(k, (1.0 / c).reshape(1, -1, 1, 1))
    return out


@pytest.mark.parametrize("net", ["hex7_6x64", "chess2x128"])
def test_the_hidden_twin_is_the_channel_twin_to_the_bit_and_the_estimate_misses_it(net):
    d, words = desc_of(net)
    base = seeded_tensors(d, SEED)
    e = CHANNEL_PATTERNS["Q8"](d.filters)
    hidden = e < 0
    assert hidden.sum() == d.filters // 4
    ht, ct = hidden_twin(d, base, e), channel_twin(d, base, e)
    # gamma and the variances are the base network's, the scale sits in the rows, the means and beta
    for p in ["_conv1._bn."] + [f"_residual_blocks.{i}._bn2." for i in range(d.blocks)]:
        assert (ht[p + "weight"] == base[p + "weight"]).all() and (ht[p + "running_var"] == base[p + "running_var"]).all()
        assert (ht[p + "bias"][hidden] == base[p + "bias"][hidden] * np.float32(2.0**-8)).all()
    assert (ht["_conv1._conv.weight"][hidden] == base["_conv1._conv.weight"][hidden] * np.float32(2.0**-8)).all()
    assert (ht["_conv1._conv.weight"][~hidden] == base["_conv1._conv.weight"][~hidden]).all()
    # (a) the same bits as the channel twin, and as the base network, in the oracle's exact f32
    planes = random_planes(d, words, 4, 5)
    want = oracle.OracleNet(pack_tensors(d, ct)).forward(planes)
    got = oracle.OracleNet(pack_tensors(d, ht)).forward(planes)
    base_out = oracle.OracleNet(pack_tensors(d, base)).forward(planes)
    for g, w, b in zip(got, want, base_out):
        assert g.tobytes() == w.tobytes() and g.tobytes() == b.tobytes()
    # (b) the estimate shifts nothing on the hidden twin, and sees the channel twin
    assert expected_stream_shift(d, ht) == 0 and not expected_stream_shifts(d, ht).any()
    assert (expected_stream_shifts(d, ct)[hidden] >= 7).all()


def test_hidden_twin_refuses_what_it_cannot_build():
    d, _ = desc_of("hex7_6x64")
    base = seeded_tensors(d, SEED)
    with pytest.raises(ValueError):
        hidden_twin(d, base, np.zeros(d.filters - 1, dtype=int))
    with pytest.raises(ValueError):
        hidden_twin(d, base, np.full(d.filters, -140))
