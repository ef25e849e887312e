"""The last two operations before a result leaves the evaluator -- the value head's tanh and the legal-move softmax's exp -- over their
whole range, on the CPU: the dial network of helpers.py (a network whose outputs the caller sets through the input planes) and the
oracle's restatements oracle.tanhf / oracle.softmax_legal_det against float64.  test_output_range_gpu.py runs the same leaves and
lists through every head path of the HIP evaluator; what both files share (targets, logit table, lists, bars) is defined here.

Seeded networks keep |value| below 0.3 and logit spreads below 2: tanh stays in its polynomial branch and exp sees [-1.6, 0].  Here
the value targets cross both branch points (0.5 and 10) and every point where exp_pos's rint changes, and the lists reach the
cut-off at -80, exponent edits down to 2^-115 and rows where all but the maximum underflow."""

import functools

import numpy as np
import pytest

from cattus_amd.weights import CHESS, NetDesc, hex_game, pack_tensors
from oracle import oracle

from helpers import DIAL_SHIFT, DIAL_VAR, dial_bits, dial_planes, dial_tensors, forward_f64, value_preactivation_f64

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)

NETS = {
    "chess64": NetDesc(**CHESS, blocks=1, filters=64, vhc=8, phc=8),
    "hex11": NetDesc(**hex_game(11), blocks=1, filters=8, vhc=4, phc=4),  # 128-slot boards, K padded in both FCs
    "chess128": NetDesc(**CHESS, blocks=1, filters=128, vhc=8, phc=8),  # GPU file: the default f16x2 plan above 128 leaves is the Winograd tower
    "chess_wide": NetDesc(**CHESS, blocks=1, filters=16, vhc=8, phc=32),  # GPU file: 40 head channels, the SIMT value kernels
}
CPU_NETS = ["chess64", "hex11"]

# ---------------------------------------------------------------------------------------- the bars
# test_oracle_tanh_accuracy's bar of the f32 tanh against float64's
TANH_RTOL, TANH_ATOL = 5e-7, 1e-9
# the realised pre-activation against the target, in f32 ulps of the target (test_the_dial_does_what_it_says derives it)
DIAL_ULPS = 4
# the legal softmax against the float64 definition: the project's absolute bar (test_eval_legal_softmax_bit_exact_vs_restatement) and a
# relative one on entries above SOFTMAX_REL_FLOOR, 2 x the figure recorded in test_softmax_legal_det_over_the_whole_domain
SOFTMAX_ABS = 1e-6
SOFTMAX_REL_FLOOR = 1e-30
SOFTMAX_REL_RECORDED = 4.0e-6
SOFTMAX_REL = 2 * SOFTMAX_REL_RECORDED


def ulps(t):
    """DIAL_ULPS f32 ulps of each target, as float64 (0 for a target of 0: the ladder's empty sum is exact everywhere)."""
    t = np.abs(np.asarray(t, dtype=np.float32))
    return np.where(t == 0, 0.0, DIAL_ULPS * np.spacing(t).astype(np.float64))


def value_bound(targets, v64):
    """How far an f32 tanh of the f32 pre-activation may lie from forward_f64's value: the tanh bar plus the dial's term through
    tanh' = 1 - v^2."""
    return TANH_RTOL * np.abs(v64) + TANH_ATOL + ulps(targets) * (1.0 - v64 * v64)


# ---------------------------------------------------------------------------------------- value targets
@functools.lru_cache(maxsize=None)
def value_targets() -> np.ndarray:
    """f32 pre-tanh targets, sorted ascending, each with its negative: 487 leaves."""
    pos = [2.0**-20]
    pos += [0.5 - 2.0**-25, 0.5, 0.5 + 2.0**-24]  # the polynomial / exp branch point and its neighbours
    pos += [10.0 - 2.0**-20, 10.0, 10.0 + 2.0**-20]  # the exp / saturation branch point and its neighbours
    pos += [16.0, 32.0]
    for k in range(15):  # where rint(2 |x| log2e) steps from k to k + 1: 2 |x| log2e = k + 1/2
        x = F32(np.log(2.0) / 2 * (2 * k + 1) / 2)
        pos += [float(np.nextafter(x, F32(0))), float(x), float(np.nextafter(x, F32(100)))]
    pos += [float(F32(x)) for x in np.linspace(0.5, 10.0, 190, endpoint=False)[1:]]  # 0.5 itself is above
    pos = sorted(set(pos))
    t = np.array([-x for x in reversed(pos)] + [0.0] + pos, dtype=np.float32)
    assert len(t) <= 512 and (np.diff(t) > 0).all()
    return t


def odd_bitwise(v) -> bool:
    """v(-x) == -v(x) to the bit over the values of value_targets() (symmetric about the middle leaf, whose target is 0)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    mid = len(v) // 2
    return bool(v[mid] == 0 and np.array_equal(np.delete(v, mid).view(np.uint32), np.delete(-v[::-1], mid).view(np.uint32)))


# ---------------------------------------------------------------------------------------- logit table and lists (chess64: 1880 moves)
BAND_VALUES = [-1e-3, -1.0, -10.0, -30.0, -60.0, float(np.nextafter(F32(-80), F32(0))), -80.0, float(np.nextafter(F32(-80), F32(-100))),
               -87.0, -100.0, -104.0, -1000.0, 50.0, 1e4, np.inf, np.nan]
ZEROS, WIDTH = 1100, 48  # moves [0, 1100) hold 0; then one band of 48 moves per BAND_VALUES entry; the 12 moves behind them hold 0
SHIFTED = np.concatenate([np.arange(512), np.arange(ZEROS + 12 * WIDTH, ZEROS + 12 * WIDTH + WIDTH // 2)])  # 512 zeros, half of the 50s


def band(value) -> np.ndarray:
    """The moves whose table entry is ``value`` (0: the first 1100)."""
    if value == 0:
        return np.arange(ZEROS)
    j = [i for i, v in enumerate(BAND_VALUES) if v == value or (value != value and v != v)][0]
    return np.arange(ZEROS + j * WIDTH, ZEROS + (j + 1) * WIDTH)


@functools.lru_cache(maxsize=None)
def logit_table() -> np.ndarray:
    t = np.zeros(NETS["chess64"].moves, dtype=np.float32)
    for j, v in enumerate(BAND_VALUES):
        t[ZEROS + j * WIDTH : ZEROS + (j + 1) * WIDTH] = v
    t.setflags(write=False)
    return t


def expected_logits(shift: bool) -> np.ndarray:
    """The f32 logits of a chess64 dial leaf: the table, the shifted band lowered by 128 in f32, non-finite entries scrubbed."""
    t = logit_table().copy()
    if shift:
        t[SHIFTED] = t[SHIFTED] + F32(DIAL_SHIFT)
    t[~np.isfinite(t)] = -FLT_MAX
    return t


@functools.lru_cache(maxsize=None)
def softmax_lists():
    """[(name, shift bit, uint16 list)]: the edge lists and the random mixes.  A list is one leaf's legal moves."""
    rng = np.random.default_rng(23)
    finite = [v for v in BAND_VALUES if np.isfinite(v)]
    near = np.concatenate([band(0)[600:700]] + [band(v) for v in finite if v not in (50.0, 1e4)])  # maximum 0
    with50 = np.concatenate([near, band(50.0)])  # maximum 50: 0 -> -50, -30 -> exactly -80, -10 -> -60
    everything = np.arange(NETS["chess64"].moves)
    out = [
        ("equal_1024", False, np.arange(1024)),  # 2^-10 exactly
        ("equal_shifted_512", True, np.arange(512)),  # all -128: 2^-9 exactly
        ("max_first", False, np.concatenate([band(1e4)[:1], rng.choice(near, 1023)])),  # [1, 0, ...]
        ("max_middle", False, np.concatenate([band(-1000.0)[:17], band(0)[:1], band(-100.0), band(-87.0)[:5]])),
        ("max_over_shifted", True, np.concatenate([np.arange(300), band(0)[600:601], np.arange(300, 512)])),  # one 0 among 512 x -128
        ("scrubbed_only", False, np.concatenate([band(np.inf), band(np.nan)])),  # uniform 1 / 96
        ("scrubbed_one", False, band(np.nan)[:1]),
        ("cutoff", False, np.concatenate([band(0)[:1], band(BAND_VALUES[6])[:1], band(BAND_VALUES[7])[:1], band(BAND_VALUES[5])[:1]])),
        ("cutoff_under_50", False, np.concatenate([band(-30.0)[:3], band(50.0)[:1], band(-10.0)[:2], band(0)[:2]])),  # -30 - 50 = -80
        ("shifted_band", True, np.concatenate([np.arange(500, 530), band(50.0), band(-60.0)[:4]])),  # 50 - 128 = -78 under 50 and 0
        ("deep_exponent", False, np.concatenate([band(50.0)[:1], band(-10.0)[:40], band(-30.0)[:40], band(-1.0)[:40]])),
    ]
    for n in (1, 63, 64, 65, 218, 1024):
        for pool_name, pool in (("near", near), ("with50", with50), ("all", everything)):
            out.append((f"mix_{pool_name}_{n}", bool(n % 2), rng.choice(pool, n)))
    return [(name, shift, np.asarray(l, dtype=np.uint16)) for name, shift, l in out]


def softmax_f64(logits, idx) -> np.ndarray:
    """calc_moves_probs in float64 on f32 logits: max-subtract, exp, divide by the sum."""
    x = np.asarray(logits, dtype=np.float32)[np.asarray(idx, dtype=np.int64)].astype(np.float64)
    e = np.exp(x - x.max())
    return e / e.sum()


def softmax_errors(probs, want64):
    """(max absolute error, max relative error on entries above SOFTMAX_REL_FLOOR)."""
    d = np.abs(np.asarray(probs, dtype=np.float64) - want64)
    big = want64 > SOFTMAX_REL_FLOOR
    return float(d.max()), float((d[big] / want64[big]).max()) if big.any() else 0.0


def check_softmax(label, probs, logits, idx):
    """The section's bars on one list: finite, within SOFTMAX_ABS and (above the floor) SOFTMAX_REL of the float64 definition, sum 1."""
    want64 = softmax_f64(logits, idx)
    ea, er = softmax_errors(probs, want64)
    assert np.isfinite(probs).all() and (np.asarray(probs) >= 0).all(), label
    assert ea <= SOFTMAX_ABS, (label, ea)
    assert er <= SOFTMAX_REL, (label, er)
    assert abs(float(np.asarray(probs, dtype=np.float64).sum()) - 1.0) <= 1e-5, label
    return ea, er


# ---------------------------------------------------------------------------------------- 1. the dial
@functools.lru_cache(maxsize=None)
def dial(net: str):
    """(desc, tensors, blob) of the dial network of NETS[net]; chess64 carries the logit table and the shifted band."""
    d = NETS[net]
    if net == "chess64":
        tensors, _ = dial_tensors(d, value_targets(), logit_table(), SHIFTED)
    else:
        table = np.linspace(-3.0, 3.0, d.moves).astype(np.float32)
        tensors, _ = dial_tensors(d, value_targets(), table, np.arange(0, d.moves, 2))
    return d, tensors, pack_tensors(d, tensors)


@functools.lru_cache(maxsize=None)
def value_leaves(net: str):
    """(planes, targets, shift bits, forward_f64's logits and values) of the value sweep: computed once, shared, read-only."""
    d, tensors, _ = dial(net)
    t = value_targets()
    shift = (np.arange(len(t)) % 3 == 1)
    planes = dial_planes(d, t, shift, seed=5)
    p64, v64 = forward_f64(d, tensors, planes)
    for a in (planes, shift, p64, v64):
        a.setflags(write=False)
    return planes, t, shift, p64, v64


@pytest.mark.parametrize("net", CPU_NETS)
def test_the_dial_does_what_it_says(net):
    """forward_f64 of the dial tensors gives tanh(target) and the table's logits, lowered by 128 on the band where asked.

    The bound on the realised pre-activation.  Two BatchNorms lie between plane 0 and the ladder (the stem's and the value head
    conv's), each with gamma 1 (or none), mean 0 and running_var DIAL_VAR, the f32 number v with fl32(v + fl32(1e-5)) = 1.  In f32
    the folded scale 1 / sqrtf(v + eps) is exactly 1 and the pre-activation IS the target.  In float64 v + 1e-5 = 1 + d with |d| <=
    2^-25 (half an ulp below 1, the rounding that made the f32 sum 1) + 1e-5 * 2^-25 (eps itself rounded to f32), so each scale is
    1 - d / 2 to first order and the product of the two lies within 2^-25 (1 + 1e-5) of 1: half an f32 ulp of a target just above
    a power of two, a quarter of one just below.  The bar is DIAL_ULPS = 4 ulps: it leaves room for a fold whose f32 sum came
    out one ulp off 1 in both BatchNorms (2 x 1 ulp) and is still 1 / 30 of the tanh bar it is added to."""
    d, tensors, blob = dial(net)
    planes, t, shift, p64, v64 = value_leaves(net)
    assert F32(DIAL_VAR + F32(1e-5)) == F32(1.0)
    pre = value_preactivation_f64(d, tensors, planes)
    t64 = t.astype(np.float64)
    worst = float(np.max(np.abs(pre - t64) / np.where(t == 0, 1.0, np.spacing(np.abs(t)).astype(np.float64))))
    print("%s: realised pre-activation within %.3f f32 ulps of its target" % (net, worst))
    assert (np.abs(pre - t64) <= ulps(t)).all() and (pre[t == 0] == 0).all()
    assert (np.abs(v64 - np.tanh(t64)) <= ulps(t) * (1 - np.tanh(t64) ** 2) + 1e-15).all()
    # logits: the table; on the band of a shifted leaf table - 128 (s_stem s_policy), the same fold term on 128
    table = np.asarray(tensors["_policy_head.2.bias"], dtype=np.float64)
    band_moves = np.flatnonzero(tensors["_policy_head.2.weight"][:, 0])
    for i in (0, 1, 2, len(t) - 1):
        want = table.copy()
        if shift[i]:
            want[band_moves] += DIAL_SHIFT
        ok = np.isfinite(want)
        assert (np.abs(p64[i][ok] - want[ok]) <= ulps(DIAL_SHIFT) * shift[i]).all(), i
        assert (np.isnan(p64[i][~ok]) == np.isnan(want[~ok])).all() and (p64[i][~ok & ~np.isnan(want)] == np.inf).all()


@pytest.mark.parametrize("net", CPU_NETS)
def test_the_oracle_on_the_dial_agrees_with_float64(net):
    """oracle.OracleNet on the dial blob: values within value_bound of forward_f64 (measured: chess64 and hex11 alike, max |dv| 7.2e-8,
    at most 0.16 of the bound), exactly +-1 from |target| = 10 on, odd, monotone; logits exactly the f32 table (lowered on the band,
    scrubbed where it is not finite)."""
    d, tensors, blob = dial(net)
    planes, t, shift, p64, v64 = value_leaves(net)
    p, v = oracle.OracleNet(blob).forward(planes)
    err, bound = np.abs(v.astype(np.float64) - v64), value_bound(t, v64)
    print("%s: oracle vs f64 max |dv| %.3g, max err / bound %.3g" % (net, err.max(), (err / bound).max()))
    assert (err <= bound).all()
    assert (v[t >= 10] == 1).all() and (v[t <= -10] == -1).all() and (np.abs(v) <= 1).all()
    assert odd_bitwise(v)
    assert (np.diff(v) >= 0).all()
    assert np.array_equal(v, np.array([oracle.tanhf(float(x)) for x in t], dtype=np.float32))  # the pre-activation is the target
    table = tensors["_policy_head.2.bias"]
    band_moves = np.flatnonzero(tensors["_policy_head.2.weight"][:, 0])
    for i in range(len(t)):
        want = table.copy()
        if shift[i]:
            want[band_moves] = want[band_moves] + F32(DIAL_SHIFT)
        want[~np.isfinite(want)] = -FLT_MAX
        assert p[i].tobytes() == want.tobytes(), i
    if net == "chess64":
        assert p[0].tobytes() == expected_logits(bool(shift[0])).tobytes() and p[1].tobytes() == expected_logits(bool(shift[1])).tobytes()


def test_the_dial_refuses_what_the_ladder_cannot_hold():
    d = NETS["chess64"]
    for bad in (64.0, 2.0**-27, float(F32(0.1)), 0.1, float("nan"), float("inf"), 32.0 + 2.0**-20):
        with pytest.raises(ValueError):
            dial_planes(d, [0.5, bad])
        with pytest.raises(ValueError):
            dial_tensors(d, [bad])
    assert dial_bits(32.0) == 1 and dial_bits(-32.0) == 1 << 32 and dial_bits(2.0**-26) == 1 << 31 and dial_bits(0.0) == 0
    assert dial_bits(-0.75) == (1 << 38) | (1 << 39)  # -(2^-1 + 2^-2): pixels 32 + 6 and 32 + 7
    with pytest.raises(ValueError):
        dial_tensors(NetDesc(**hex_game(7), blocks=1, filters=8, vhc=4, phc=4))  # 49 pixels: no room for 64 ladder terms
    with pytest.raises(ValueError):
        dial_tensors(d, logit_table=np.zeros(5))


# ---------------------------------------------------------------------------------------- 2. the softmax restatement
def test_softmax_legal_det_over_the_whole_domain():
    """oracle.softmax_legal_det against the float64 definition, on N(0, 1) logits times 1, 10, 40 and 100 at every length and on the
    edge lists of softmax_lists over both rows of expected_logits.

    Recorded here (the restatement is deterministic: these are its figures on any machine): max absolute error 4.4e-7; max relative
    error on entries above 1e-30 3.98e-6 -- half an ulp of the f32 difference logit - max at 64 .. 128 (3.8e-6: an entry above 1e-30
    has a difference above -69.1) plus exp_pos's own 2e-7.  SOFTMAX_REL is twice the recorded 4.0e-6, so an exponent-bit edit that
    goes wrong on a tiny probability (a factor of two) cannot hide under the absolute bar."""
    rng = np.random.default_rng(7)
    worst_a = worst_r = 0.0
    for scale in (1, 10, 40, 100):
        for n in (1, 2, 63, 64, 65, 218, 1024):
            for rep in range(4):
                logits = (rng.standard_normal(1880) * scale).astype(np.float32)
                idx = rng.choice(1880, n, replace=False).astype(np.uint16)
                ea, er = check_softmax((scale, n, rep), oracle.softmax_legal_det(logits, idx), logits, idx)
                worst_a, worst_r = max(worst_a, ea), max(worst_r, er)
    for name, shift, idx in softmax_lists():
        for row in (False, True):
            logits = expected_logits(row)
            ea, er = check_softmax((name, row), oracle.softmax_legal_det(logits, idx), logits, idx)
            worst_a, worst_r = max(worst_a, ea), max(worst_r, er)
    print("softmax_legal_det vs float64: max abs %.3g, max rel above %g: %.3g" % (worst_a, SOFTMAX_REL_FLOOR, worst_r))
    assert worst_r <= SOFTMAX_REL_RECORDED  # the recorded figure is the one the bar was doubled from


def test_softmax_legal_det_on_the_edge_lists_exactly():
    """Where the result is known without arithmetic."""
    lists = {name: (shift, idx) for name, shift, idx in softmax_lists()}

    def run(name):
        shift, idx = lists[name]
        return oracle.softmax_legal_det(expected_logits(shift), idx), idx

    p, _ = run("equal_1024")
    assert (p == F32(2.0**-10)).all()
    p, _ = run("equal_shifted_512")
    assert (p == F32(2.0**-9)).all()
    p, _ = run("max_first")
    assert p[0] == 1 and not p[1:].any()
    p, idx = run("max_middle")
    assert p[17] == 1 and p.sum() == 1 and np.count_nonzero(p) == 1
    p, _ = run("max_over_shifted")
    assert p[300] == 1 and np.count_nonzero(p) == 1
    p, _ = run("scrubbed_only")
    assert (p == F32(1.0) / F32(96.0)).all()  # max = f32::MIN: every difference is 0
    p, _ = run("scrubbed_one")
    assert p.tolist() == [1.0]
    p, _ = run("cutoff")  # 0, -80, -80 - ulp, -80 + ulp: exactly -80 is still evaluated, an ulp below is 0
    assert p[0] == 1 and p[2] == 0 and 0 < p[1] < p[3] < 2e-35
    assert abs(float(p[1]) / np.exp(-80.0) - 1) < 1e-5 and abs(float(p[3]) / np.exp(float(F32(BAND_VALUES[5]))) - 1) < 1e-5
    p, _ = run("cutoff_under_50")
    assert p[3] == 1 and (p[:3] > 0).all() and (p[:3] < 2e-35).all()  # -30 - 50 is exactly -80: still evaluated
    assert (p[4:6] > 1e-27).all() and (p[6:] > 1e-22).all()  # -10 - 50 and 0 - 50 are far above it
