"""ctypes binding of ``libcattus_hip.so`` (include/cattus_hip.h).

``HipEvaluator`` plays the role of the reference's ``NNetwork`` + ``Model`` pair
(engine/src/net/mod.rs:14-72, engine/src/net/model.rs:57-218): ``run_net`` takes the leaves of
one batch and returns ``[(logits, value), ...]``; ``planes_to_tensor`` is the stand-alone
tensor packer (engine/src/net/mod.rs:121-156).  There is no CPU implementation behind these
calls: if the shared library is missing or no HIP device is usable they raise.
"""

from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from .weights import NetDesc, parse_header

import os

_PKG = Path(__file__).resolve().parent
# CATTUS_HIP_LIB selects another build of the same ABI (e.g. the stamped diagnostic build)
LIB_PATH = Path(os.environ.get("CATTUS_HIP_LIB", _PKG / "libcattus_hip.so"))

DTYPE_F32, DTYPE_BF16, DTYPE_F16X2, DTYPE_F16, DTYPE_F16W = 0, 1, 2, 3, 4
# "f16x2": the split-precision tower (pairs of f16 values, 22 significant bits; include/cattus_hip.h); "f16": single-term f16;
# "f16w": single-term f16 in Winograd F(2x2,3x3) form with f32 rows between the layers (CATTUS_DTYPE_F16W: opt-in, bits of its own)
_DTYPES = {"f32": DTYPE_F32, "bf16": DTYPE_BF16, "f16x2": DTYPE_F16X2, "f16": DTYPE_F16, "f16w": DTYPE_F16W}
# "f32w": f32 operands in Winograd F(2x2,3x3) form on the f32 tower's rows (CATTUS_DTYPE_F32W: opt-in, bits of its own).  A table of its own
# beside _DTYPES, which stays the five dtypes it was; the constructor consults both.
DTYPE_F32W = 5
_DTYPES_WINO_F32 = {"f32w": DTYPE_F32W}
# "f16r": the direct single-term f16 tower with the residual stream kept in f32 (CATTUS_DTYPE_F16R: opt-in, bits of its own, dtype f16's
# coverage).  A table of its own again: the two above stay what they were.
DTYPE_F16R = 6
_DTYPES_F16R = {"f16r": DTYPE_F16R}
# "f16r_resident": dtype "f16r"'s arithmetic, bit for bit, as a demand for the one-launch LDS-resident form (CATTUS_DTYPE_F16R_RESIDENT: at most
# 64 filters, where dtype "f16" accepts tower_form "resident").  A table of its own again: the three above stay what they were.
DTYPE_F16R_RESIDENT = 7
_DTYPES_F16R_RESIDENT = {"f16r_resident": DTYPE_F16R_RESIDENT}
# "f32_resident": dtype "f32"'s arithmetic, bit for bit, as a demand for the one-launch LDS-resident form (CATTUS_DTYPE_F32_RESIDENT: at most 64
# filters and 32 planes).  9, not 8: 8 stays unassigned and invalid.  A table of its own again: the four above stay what they were.
DTYPE_F32_RESIDENT = 9
_DTYPES_F32_RESIDENT = {"f32_resident": DTYPE_F32_RESIDENT}

# every symbol include/cattus_hip.h declares
ABI_SYMBOLS = [
    "cattus_hip_create",
    "cattus_hip_destroy",
    "cattus_hip_desc",
    "cattus_hip_eval",
    "cattus_hip_eval_device",
    "cattus_hip_eval_device_lane",
    "cattus_hip_eval_legal",
    "cattus_hip_lane_stream",
    "cattus_hip_submit",
    "cattus_hip_wait",
    "cattus_hip_flush",
    "cattus_hip_apply",
    "cattus_hip_submit_legal",
    "cattus_hip_wait_legal",
    "cattus_hip_apply_legal",
    "cattus_hip_host_alloc",
    "cattus_hip_host_free",
    "cattus_hip_stats",
    "cattus_hip_time_tower",
    "cattus_hip_mfma_sustained",
    "cattus_hip_planes_to_tensor",
    "cattus_hip_planes_to_tensor_device",
    "cattus_hip_last_error",
    "cattus_hip_version",
    "cattus_hip_runtime_note",
    "cattus_hip_tower_kernel",
    "cattus_hip_tail_leaves",
    "cattus_hip_tail_batches",
    "cattus_hip_head_chain",
    "cattus_hip_head_chain_leaves",
    "cattus_hip_head_chain_batches",
    "cattus_hip_fused_heads",
    "cattus_hip_fused_heads_effective",
    "cattus_hip_fused_heads_batches",
    "cattus_hip_stream_range",
    "cattus_hip_create_calibrated",
    "cattus_hip_verify",
    "cattus_hip_verify_stats",
    "cattus_hip_verify_worst_planes",
    "cattus_hip_verify_prior_stats",
    "cattus_hip_verify_worst_prior",
    "cattus_hip_points",
    "cattus_hip_tap",
    "cattus_hip_trace",
    "cattus_hip_compare_outputs",  # include/cattus_hip_diag.h
    "cattus_hip_compare_priors",  # include/cattus_hip_diag.h
    "cattus_hip_create_diag",  # include/cattus_hip_diag.h
    "cattus_hip_create_calibrated_diag",  # include/cattus_hip_diag.h
    "cattus_hip_stream_shift",  # include/cattus_hip_diag.h
    "cattus_hip_stream_shifts",  # include/cattus_hip_diag.h
    "cattus_hip_stem_input",  # include/cattus_hip_diag.h
    "cattus_hip_splitk_plan",  # include/cattus_hip_diag.h
]

# Symbols an OLDER build of the library may lack.  Only a build selected with CATTUS_HIP_LIB may (scripts/fused_heads_time.py times the parent
# commit's library that way); the package's own library must have every symbol.  Calling a method whose symbol is absent raises AttributeError.
ABI_NEWER_SYMBOLS = ("cattus_hip_fused_heads", "cattus_hip_fused_heads_effective", "cattus_hip_fused_heads_batches")


class CattusHipError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"cattus_hip status {status}: {message}")
        self.status = status


class EvalConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("max_batch", C.c_uint32),
        ("plane_words", C.c_uint32),
        ("dtype", C.c_uint32),
        ("flush_us", C.c_uint32),
        ("tower_form", C.c_uint32),
        ("tail_leaves", C.c_uint32),
    ]


TOWER_FORMS = {"auto": 0, "direct": 1, "winograd": 2, "winograd_f4": 3, "direct_splitk": 4}  # cattus_tower_form
# the one-launch LDS-resident tower as a demand (dtype f16: opt-in, the per-layer tower's bits; bf16 / f16x2: where "auto" already runs it)
TOWER_FORMS_RESIDENT = {"resident": 5}
# Diagnostic switches (include/cattus_hip_diag.h).  The library reads none of them from the environment; this binding -- the
# harness of the tests and the timing scripts -- forwards the ones it finds there through cattus_hip_create_diag, so that
# `CATTUS_TOWER64=0 python scripts/...` and monkeypatch.setenv keep working.  CATTUS_WINOGRAD=0/1 (rounds 3-4) maps to tower_form.
DIAG_SWITCHES = ("CATTUS_CONV_CB", "CATTUS_CONV_PBW", "CATTUS_FUSED_STEM", "CATTUS_T64_CH", "CATTUS_T64_LS", "CATTUS_SPLIT_W", "CATTUS_T64S_HEADS",
                 "CATTUS_T64S_SHAPE", "CATTUS_TOWER64", "CATTUS_FORCE_GENERIC", "CATTUS_WINO_INPLACE", "CATTUS_ARENA", "CATTUS_WINO_KERNEL",
                 "CATTUS_WINO_PERSIST", "CATTUS_WINO_SPIN", "CATTUS_STREAM_SHIFT", "CATTUS_SPLITK_WAYS", "CATTUS_T64F_NARROW")


class Stats(C.Structure):
    _fields_ = [
        ("batches", C.c_uint64),
        ("positions", C.c_uint64),
        ("full_batches", C.c_uint64),
        ("run_seconds_ema", C.c_double),
        ("run_seconds_total", C.c_double),
        ("saturated", C.c_uint64),
    ]


class ChannelRange(C.Structure):
    _fields_ = [("rms", C.c_float), ("abs_max", C.c_float)]


class VerifyStats(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("every", C.c_uint32),
        ("batches", C.c_uint64),
        ("leaves", C.c_uint64),
        ("leaves_outside", C.c_uint64),
        ("max_dlogit", C.c_float),
        ("logit", C.c_float),
        ("logit_ref", C.c_float),
        ("move", C.c_uint32),
        ("max_dvalue", C.c_float),
        ("value", C.c_float),
        ("value_ref", C.c_float),
        ("reserved", C.c_uint32),
    ]


class PriorStats(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("reserved", C.c_uint32),
        ("batches", C.c_uint64),
        ("batches_without_legal", C.c_uint64),
        ("leaves", C.c_uint64),
        ("top1_flips", C.c_uint64),
        ("nonfinite", C.c_uint64),
        ("empty", C.c_uint64),
        ("sum_tv", C.c_double),
        ("sum_regret", C.c_double),
        ("max_tv", C.c_float),
        ("max_regret", C.c_float),
        ("tv_hist", C.c_uint64 * 8),
        ("value_leaves", C.c_uint64),
        ("sum_dvalue", C.c_double),
    ]


# one leaf of the prior comparison kernel (include/cattus_hip_diag.h, cattus_hip_compare_priors): flags bit 0 a non-finite probability,
# bit 1 no legal move, bit 2 legal_count > L, bit 3 a non-finite value
PRIOR_RECORD = np.dtype([("tv", "<f4"), ("top_a", "<u4"), ("top_b", "<u4"), ("regret", "<f4"), ("max_dp", "<f4"), ("k_max", "<u4"), ("count", "<u2"),
                         ("flags", "<u2"), ("dvalue", "<f4")])

# one leaf's verdict of the comparison kernel (include/cattus_hip_diag.h, cattus_hip_compare_outputs): flags bit 0 the leaf is
# outside the bar, bit 1 its value is
VERIFY_RECORD = np.dtype([("max_dlogit", "<f4"), ("move", "<u4"), ("dvalue", "<f4"), ("flags", "<u4")])


# one (point, leaf) of HipEvaluator.trace (include/cattus_hip.h, cattus_trace_record): flags bit 0 a non-finite value on either side
TRACE_RECORD = np.dtype([("max_diff", "<f4"), ("at", "<u4"), ("x", "<f4"), ("ref", "<f4"), ("rms_diff", "<f4"), ("rms_ref", "<f4"), ("flags", "<u4"),
                         ("reserved", "<u4")])


class NetDescC(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("planes", "board", "moves", "blocks", "filters", "vhc", "phc", "fc_hidden")]


_lib = None


def load_library():
    """Load libcattus_hip.so from the package directory; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: build it with `python -m cattus_amd.build` "
            "(there is no CPU fallback for the leaf evaluator)"
        )
    L = C.CDLL(str(LIB_PATH))
    u64p, f32p = C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    vp = C.c_void_p
    L.cattus_hip_create.argtypes = [vp, C.c_size_t, C.POINTER(EvalConfig), C.POINTER(vp)]
    L.cattus_hip_create_diag.argtypes = [vp, C.c_size_t, C.POINTER(EvalConfig), C.c_char_p, C.POINTER(vp)]
    L.cattus_hip_create_calibrated.argtypes = [vp, C.c_size_t, C.POINTER(EvalConfig), u64p, C.c_uint32, C.POINTER(vp)]
    L.cattus_hip_create_calibrated_diag.argtypes = [vp, C.c_size_t, C.POINTER(EvalConfig), C.c_char_p, u64p, C.c_uint32, C.POINTER(vp)]
    L.cattus_hip_stream_range.argtypes = [vp, u64p, C.c_uint32, C.POINTER(ChannelRange), C.c_uint32]
    L.cattus_hip_destroy.argtypes = [vp]
    L.cattus_hip_destroy.restype = None
    L.cattus_hip_desc.argtypes = [vp, C.POINTER(NetDescC)]
    L.cattus_hip_eval.argtypes = [vp, u64p, C.c_uint32, f32p, f32p]
    L.cattus_hip_eval_device.argtypes = [vp, vp, C.c_uint32, vp, vp, vp]
    L.cattus_hip_eval_device_lane.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp]
    L.cattus_hip_lane_stream.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
    u16p = C.POINTER(C.c_uint16)
    L.cattus_hip_eval_legal.argtypes = [vp, u64p, C.c_uint32, u16p, u16p, C.c_uint32, f32p, f32p]
    L.cattus_hip_submit.argtypes = [vp, u64p, C.POINTER(C.c_uint64)]
    L.cattus_hip_wait.argtypes = [vp, C.c_uint64, f32p, f32p]
    L.cattus_hip_flush.argtypes = [vp]
    L.cattus_hip_apply.argtypes = [vp, u64p, C.c_uint32, f32p, f32p]
    L.cattus_hip_submit_legal.argtypes = [vp, u64p, u16p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.cattus_hip_wait_legal.argtypes = [vp, C.c_uint64, f32p, f32p]
    L.cattus_hip_apply_legal.argtypes = [vp, u64p, C.c_uint32, u16p, C.POINTER(C.c_uint32), f32p, f32p]
    L.cattus_hip_host_alloc.argtypes = [C.c_size_t]
    L.cattus_hip_host_alloc.restype = vp
    L.cattus_hip_host_free.argtypes = [vp]
    L.cattus_hip_host_free.restype = None
    L.cattus_hip_stats.argtypes = [vp, C.POINTER(Stats)]
    L.cattus_hip_time_tower.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
    L.cattus_hip_mfma_sustained.argtypes = [vp, C.c_double, C.POINTER(C.c_double)]
    L.cattus_hip_planes_to_tensor.argtypes = [C.c_int, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, f32p]
    L.cattus_hip_planes_to_tensor_device.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
    L.cattus_hip_last_error.restype = C.c_char_p
    L.cattus_hip_version.restype = C.c_char_p
    L.cattus_hip_runtime_note.restype = C.c_char_p
    L.cattus_hip_tower_kernel.argtypes = [vp]
    L.cattus_hip_tower_kernel.restype = C.c_char_p
    L.cattus_hip_tail_leaves.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.cattus_hip_tail_batches.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.cattus_hip_head_chain.argtypes = [vp, C.c_uint32]
    L.cattus_hip_head_chain_leaves.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.cattus_hip_head_chain_batches.argtypes = [vp, C.POINTER(C.c_uint64)]
    absent = [name for name in ABI_NEWER_SYMBOLS if not hasattr(L, name)] if "CATTUS_HIP_LIB" in os.environ else []
    if "cattus_hip_fused_heads" not in absent:
        L.cattus_hip_fused_heads.argtypes = [vp, C.c_uint32]
        L.cattus_hip_fused_heads_effective.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.cattus_hip_fused_heads_batches.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.cattus_hip_stream_shift.argtypes = [vp]
    L.cattus_hip_stream_shifts.argtypes = [vp, C.POINTER(C.c_int), C.c_uint32]
    L.cattus_hip_stem_input.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.cattus_hip_splitk_plan.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.cattus_hip_verify.argtypes = [vp, vp, C.c_size_t, C.c_uint32]
    L.cattus_hip_verify_stats.argtypes = [vp, C.POINTER(VerifyStats)]
    L.cattus_hip_verify_worst_planes.argtypes = [vp, u64p]
    L.cattus_hip_compare_outputs.argtypes = [C.c_int, f32p, f32p, f32p, f32p, C.c_uint32, C.c_uint32, vp]
    u32p = C.POINTER(C.c_uint32)
    L.cattus_hip_verify_prior_stats.argtypes = [vp, C.POINTER(PriorStats)]
    L.cattus_hip_verify_worst_prior.argtypes = [vp, u64p, u16p, C.c_uint32, u32p, u32p, u32p]
    L.cattus_hip_compare_priors.argtypes = [C.c_int, f32p, f32p, u16p, C.c_uint32, C.c_uint32, f32p, f32p, vp]
    L.cattus_hip_points.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.cattus_hip_tap.argtypes = [vp, u64p, C.c_uint32, C.c_uint32, f32p, f32p, f32p]
    L.cattus_hip_trace.argtypes = [vp, vp, C.c_size_t, u64p, C.c_uint32, vp, C.c_uint32, f32p, f32p]
    for name in ABI_SYMBOLS:
        if name in absent:
            continue
        fn = getattr(L, name)
        if fn.restype is C.c_int and name not in ("cattus_hip_last_error", "cattus_hip_version", "cattus_hip_runtime_note", "cattus_hip_host_alloc",
                                                   "cattus_hip_tower_kernel"):
            fn.restype = C.c_int
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise CattusHipError(rc, load_library().cattus_hip_last_error().decode(errors="replace"))


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _f32(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def planes_to_tensor(planes: np.ndarray, board: int, batch_size: int, device: int = 0) -> np.ndarray:
    """HIP drop-in for ``planes_to_tensor`` (engine/src/net/mod.rs:121-156).

    planes: uint64 ``[n, C, plane_words]`` -> float32 ``[batch_size, C, S, S]``, rows ``n..`` zero.
    """
    planes = np.ascontiguousarray(planes, dtype=np.uint64)
    n, c, w64 = planes.shape
    out = np.empty((batch_size, c, board, board), dtype=np.float32)
    _check(load_library().cattus_hip_planes_to_tensor(device, _u64(planes), n, c, w64, board, batch_size, _f32(out)))
    return out


def compare_outputs(policy_a, policy_b, value_a, value_b, device: int = 0) -> np.ndarray:
    """The comparison kernel of ``HipEvaluator.verify`` on host arrays (cattus_hip_compare_outputs, include/cattus_hip_diag.h):
    float32 ``[n, M]`` logits and ``[n]`` values of two runtimes, b the reference side -> ``[n]`` records of dtype VERIFY_RECORD."""
    pa, pb = (np.ascontiguousarray(p, dtype=np.float32) for p in (policy_a, policy_b))
    va, vb = (np.ascontiguousarray(v, dtype=np.float32) for v in (value_a, value_b))
    if pa.ndim != 2 or pa.shape != pb.shape or va.shape != (pa.shape[0],) or vb.shape != va.shape:
        raise ValueError("compare_outputs: policies [n, M] and values [n] of both sides")
    out = np.zeros(pa.shape[0], dtype=VERIFY_RECORD)
    _check(load_library().cattus_hip_compare_outputs(device, _f32(pa), _f32(pb), _f32(va), _f32(vb), pa.shape[0], pa.shape[1], out.ctypes.data))
    return out


def compare_priors(probs_a, probs_b, legal_count, value_a, value_b, device: int = 0) -> np.ndarray:
    """The prior comparison kernel of ``HipEvaluator.verify_prior_stats`` on host arrays (cattus_hip_compare_priors,
    include/cattus_hip_diag.h): float32 ``[n, L]`` legal-move softmax rows of two runtimes, b the reference side, uint16 ``[n]`` legal
    counts and ``[n]`` values -> ``[n]`` records of dtype PRIOR_RECORD."""
    pa, pb = (np.ascontiguousarray(p, dtype=np.float32) for p in (probs_a, probs_b))
    va, vb = (np.ascontiguousarray(v, dtype=np.float32) for v in (value_a, value_b))
    cnt = np.ascontiguousarray(legal_count, dtype=np.uint16)
    if pa.ndim != 2 or pa.shape != pb.shape or va.shape != (pa.shape[0],) or vb.shape != va.shape or cnt.shape != va.shape:
        raise ValueError("compare_priors: probs [n, L] of both sides, legal counts [n] and values [n] of both sides")
    out = np.zeros(pa.shape[0], dtype=PRIOR_RECORD)
    _check(load_library().cattus_hip_compare_priors(device, _f32(pa), _f32(pb), cnt.ctypes.data_as(C.POINTER(C.c_uint16)), pa.shape[0], pa.shape[1],
                                                    _f32(va), _f32(vb), out.ctypes.data))
    return out


class HipEvaluator:
    """One network resident on one MI355X.

    Mirrors ``NNetwork::new(model_path, inference_cfg, batch_size, cache)`` (net/mod.rs:24-39) with
    the weight blob in place of the model path and ``{"engine": "hip", "device", "dtype"}`` in place
    of ``InferenceConfig``.
    """

    def __init__(
        self,
        blob: bytes,
        batch_size: int,
        plane_words: int,
        dtype: str = "bf16",
        device: int = 0,
        flush_us: int = 200,
        tower_form: str | None = None,
        switches: dict | None = None,
        calibration=None,
        verify_every: int = 0,
        tail_leaves: int = 0,
        head_chain_leaves: int = 0,
        fused_heads: bool = False,
    ):
        """dtype: "f32" | "bf16" | "f16x2" | "f16" | "f16w" | "f32w" (cattus_dtype).  "f16w" is the single-term f16 tower in Winograd F(2x2,3x3) form with an f32 stream: an 8x8
        board, at least one residual block, a multiple of 64 filters >= 128, tower_form "auto" or "winograd" (both mean it); anything else is refused.
        "f32w" is the f32-operand tower in the same form with the same coverage and the same refusals: the exact tower's stem, U = f32(G g G^T), f32 sums, no
        cap, no stream shift, ``saturated`` stays 0; bits of its own (not the exact tower's); ``verify`` / ``trace`` hold it to the f32 shadow like any other.
        "f16r" (_DTYPES_F16R) is the direct single-term f16 tower with the residual stream kept in f32: dtype "f16"'s weights, shifts, calibration and coverage
        (any board, any filter count), one launch per layer, bits of its own; tower_form "resident" is refused, the other forms (forms of the "f16x2" tower) mean "auto"; calibrated, it keeps
        the BatchNorm estimate's shifts and takes only the headroom guard from the sample, as "f16w" does.
        "f16r_resident" (_DTYPES_F16R_RESIDENT) is "f16r" in ONE LDS-resident launch (tower64_stream_kernel), the same bits: networks of at most 64 filters, where dtype "f16"
        accepts tower_form "resident"; tower_form "auto" and "resident" both mean it, the forms of the "f16x2" tower are ignored, anything it does not cover is refused.
        "f32_resident" (_DTYPES_F32_RESIDENT) is "f32" in ONE LDS-resident launch (tower64_f32_kernel), the same bits and so the CPU oracle's: networks of at most 64
        filters and 32 planes with value + policy head channels <= 32; tower_form "auto" and "resident" both mean it, anything it does not cover is refused; like "f32" it has no shadow
        (``verify`` / ``trace`` are refused) and nothing to calibrate.
        tower_form: "auto" | "direct" | "winograd" | "winograd_f4" | "direct_splitk" (cattus_tower_form; None = "auto", or what CATTUS_WINOGRAD=0/1 in the
        environment says; "winograd_f4", the F(4x4,3x3) form, and "direct_splitk", the direct form with the K walk divided over a workgroup's waves
        for batches of a few leaves, are opt-in only: never what "auto" picks, and each has bits of its own; "resident" (TOWER_FORMS_RESIDENT)
        demands the one-launch LDS-resident tower of a network with at most 64 filters: for dtype "f16" opt-in, with the bits of "auto" and
        one tower launch instead of 1 + 2 * blocks; for "bf16" / "f16x2" accepted where "auto" already runs it; refused everywhere else).  switches: diagnostic switches for cattus_hip_create_diag (None = the CATTUS_* ones found in the
        environment, {} = none).  calibration: sample positions, uint64 ``[n, C, plane_words]`` -- the f16 / f16x2 towers then
        take their stream shifts from the range measured on them instead of from the BatchNorm parameters
        (cattus_hip_create_calibrated; nothing to calibrate for f32 / bf16, which come out as without it, and nothing for "f32w"; "f16w", whose stream is f32, keeps the
        BatchNorm estimate's shifts and takes only the headroom guard from the sample).  verify_every: N >= 1
        checks every Nth batch against a shadow f32 tower (``verify``); 0, the default, builds no shadow and checks nothing.
        tail_leaves: k >= 1 runs batches of at most k leaves of the Winograd F(2x2,3x3) tower on its small-tile kernel (cattus_eval_config.tail_leaves:
        the same bits, more workgroups for a short batch); ignored on every other plan (``tail_leaves()`` says what holds); 0, the default: off.
        head_chain_leaves: k >= 1 runs the f32 heads' FC pair of batches of at most k leaves as short fmaf chains (``head_chain``: the same bits);
        ignored where the heads are not the f32 MFMA heads (``head_chain_leaves()`` says what holds); 0, the default: off.
        fused_heads: True runs the two 1x1 head convs in the tail of the resident "f16" (tower_form "resident") and "f16r_resident" tower
        launch instead of a launch of their own (``fused_heads``: the same bits); ignored on every other plan (``fused_heads_effective()`` says what
        holds); False, the default: off."""
        self.desc: NetDesc = parse_header(blob)
        self.batch_size = int(batch_size)
        self.plane_words = int(plane_words)
        self.dtype = dtype
        self.device = device
        self._lib = load_library()
        self._legal_counts: dict[int, int] = {}  # submit_legal ticket -> its list's length, until wait_legal
        if tower_form is None:
            legacy = os.environ.get("CATTUS_WINOGRAD")
            tower_form = "auto" if not legacy else ("winograd" if legacy[0] == "1" else "direct")
            if tower_form == "winograd" and not (dtype == "f16x2" and self.desc.board == 8 and self.desc.blocks > 0 and self.desc.filters >= 128 and self.desc.filters % 64 == 0):
                tower_form = "auto"  # the environment form was a wish ("where the shape allows it"); the config field is a demand
            if dtype in ("f16w", "f32w"):
                tower_form = "auto"  # the dtype is its form: the environment's wish for the f16x2 tower does not reach it
        if switches is None:
            switches = {k: os.environ[k] for k in DIAG_SWITCHES if k in os.environ}
        self.tower_form = tower_form
        dtype_value = _DTYPES_F32_RESIDENT[dtype] if dtype in _DTYPES_F32_RESIDENT else {**_DTYPES_F16R_RESIDENT, **_DTYPES, **_DTYPES_WINO_F32, **_DTYPES_F16R}[dtype]
        cfg = EvalConfig(C.sizeof(EvalConfig), device, self.batch_size, self.plane_words, dtype_value, flush_us, {**TOWER_FORMS, **TOWER_FORMS_RESIDENT}[tower_form], int(tail_leaves))
        h = C.c_void_p()
        buf = C.create_string_buffer(blob, len(blob))
        text = ";".join(f"{k}={v}" for k, v in switches.items()).encode() if switches else None
        if calibration is not None:
            cal = self._planes(calibration)
            if text:
                _check(self._lib.cattus_hip_create_calibrated_diag(buf, len(blob), C.byref(cfg), text, _u64(cal), len(cal), C.byref(h)))
            else:
                _check(self._lib.cattus_hip_create_calibrated(buf, len(blob), C.byref(cfg), _u64(cal), len(cal), C.byref(h)))
        elif text:
            _check(self._lib.cattus_hip_create_diag(buf, len(blob), C.byref(cfg), text, C.byref(h)))
        else:
            _check(self._lib.cattus_hip_create(buf, len(blob), C.byref(cfg), C.byref(h)))
        self._h = h
        self._blob = blob  # cattus_hip_verify takes it again: the library keeps no host copy
        try:
            if head_chain_leaves:
                self.head_chain(head_chain_leaves)
            if fused_heads:
                self.fused_heads(True)
            if verify_every:
                self.verify(verify_every)
        except Exception:
            self.close()
            raise

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.cattus_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- evaluation -------------------------------------------------------------------------
    def _planes(self, planes) -> np.ndarray:
        planes = np.ascontiguousarray(planes, dtype=np.uint64)
        if planes.ndim != 3 or planes.shape[1:] != (self.desc.planes, self.plane_words):
            raise ValueError(f"planes shape {planes.shape} != [n, {self.desc.planes}, {self.plane_words}]")
        return planes

    def eval(self, planes) -> tuple[np.ndarray, np.ndarray]:
        """planes uint64 ``[n, C, plane_words]`` -> (logits ``[n, M]``, values ``[n]``)."""
        planes = self._planes(planes)
        n = planes.shape[0]
        policy = np.empty((n, self.desc.moves), dtype=np.float32)
        value = np.empty((n,), dtype=np.float32)
        _check(self._lib.cattus_hip_eval(self._h, _u64(planes), n, _f32(policy), _f32(value)))
        return policy, value

    def eval_legal(self, planes, legal_idx, legal_count) -> tuple[np.ndarray, np.ndarray]:
        """``eval`` + ``calc_moves_probs`` (net/mod.rs:100-119) on the device.

        legal_idx uint16 ``[n, L]``, legal_count uint16 ``[n]`` -> (probs ``[n, L]``, values ``[n]``).
        """
        planes = self._planes(planes)
        n = planes.shape[0]
        legal_idx = np.ascontiguousarray(legal_idx, dtype=np.uint16)
        legal_count = np.ascontiguousarray(legal_count, dtype=np.uint16)
        if legal_idx.ndim != 2 or legal_idx.shape[0] != n or legal_count.shape != (n,):
            raise ValueError("legal_idx must be [n, L] and legal_count [n]")
        probs = np.empty(legal_idx.shape, dtype=np.float32)
        value = np.empty((n,), dtype=np.float32)
        u16 = C.POINTER(C.c_uint16)
        _check(
            self._lib.cattus_hip_eval_legal(
                self._h, _u64(planes), n, legal_idx.ctypes.data_as(u16), legal_count.ctypes.data_as(u16),
                legal_idx.shape[1], _f32(probs), _f32(value),
            )
        )
        return probs, value

    def run_net(self, planes) -> list[tuple[np.ndarray, float]]:
        """``NNetwork::run_net`` (net/mod.rs:41-72): one ``(logits, value)`` pair per leaf."""
        policy, value = self.eval(planes)
        return [(policy[i], float(value[i])) for i in range(len(value))]

    def eval_device(self, d_planes: int, n: int, d_policy: int, d_value: int, stream: int = 0, lane: int = 0):
        """Asynchronous evaluation on raw device pointers (all buffers resident in HBM), enqueued on
        ``stream`` (a hipStream_t handle; 0 is HIP's legacy default stream)."""
        _check(self._lib.cattus_hip_eval_device_lane(self._h, lane, d_planes, n, d_policy, d_value, stream))

    def lane_stream(self, lane: int = 0) -> int:
        """Handle of the lane's own stream."""
        st = C.c_void_p()
        _check(self._lib.cattus_hip_lane_stream(self._h, lane, C.byref(st)))
        return st.value or 0

    # -- leaf server (Batcher::apply replacement, util/batch.rs:49-177) ---------------------
    def submit(self, planes_one) -> int:
        p = np.ascontiguousarray(planes_one, dtype=np.uint64).reshape(self.desc.planes, self.plane_words)
        t = C.c_uint64()
        _check(self._lib.cattus_hip_submit(self._h, _u64(p), C.byref(t)))
        return t.value

    def wait(self, ticket: int) -> tuple[np.ndarray, float]:
        policy = np.empty((self.desc.moves,), dtype=np.float32)
        value = C.c_float()
        _check(self._lib.cattus_hip_wait(self._h, ticket, _f32(policy), C.byref(value)))
        return policy, value.value

    def flush(self):
        _check(self._lib.cattus_hip_flush(self._h))

    # the same with calc_moves_probs (net/mod.rs:100-119) on the device: a leaf's legal-move priors come back instead of its logits
    def submit_legal(self, planes_one, legal_idx) -> int:
        """One leaf with its legal moves' policy indices (uint16, at most 1024, each < moves; may be empty) -> ticket for ``wait_legal``."""
        p = np.ascontiguousarray(planes_one, dtype=np.uint64).reshape(self.desc.planes, self.plane_words)
        idx = np.ascontiguousarray(legal_idx, dtype=np.uint16).reshape(-1)
        t = C.c_uint64()
        _check(self._lib.cattus_hip_submit_legal(self._h, _u64(p), idx.ctypes.data_as(C.POINTER(C.c_uint16)), len(idx), C.byref(t)))
        self._legal_counts[t.value] = len(idx)
        return t.value

    def wait_legal(self, ticket: int) -> tuple[np.ndarray, float]:
        """(probs ``[legal_count of that submit]``, value) of a ``submit_legal`` ticket."""
        count = self._legal_counts.get(ticket, 1024)  # a ticket that is not one of submit_legal's: the library refuses it
        probs = np.empty((count,), dtype=np.float32)
        value = C.c_float()
        _check(self._lib.cattus_hip_wait_legal(self._h, ticket, _f32(probs), C.byref(value)))
        self._legal_counts.pop(ticket, None)
        return probs, value.value

    def apply_legal(self, planes, legal_lists) -> tuple[list[np.ndarray], np.ndarray]:
        """``submit_legal`` + ``wait_legal`` for n leaves, blocking (cattus_hip_apply_legal): planes uint64 ``[n, C, plane_words]`` and one
        list of policy indices per leaf -> (one probs array per leaf, values ``[n]``)."""
        planes = self._planes(planes)
        n = planes.shape[0]
        lists = [np.ascontiguousarray(l, dtype=np.uint16).reshape(-1) for l in legal_lists]
        if len(lists) != n:
            raise ValueError("apply_legal: one legal list per leaf")
        off = np.zeros(n + 1, dtype=np.uint32)
        np.cumsum([len(l) for l in lists], out=off[1:])
        probs, value = self.apply_legal_ragged(planes, np.concatenate(lists) if lists else np.zeros(0, dtype=np.uint16), off)
        return [probs[off[i] : off[i + 1]].copy() for i in range(n)], value

    def apply_legal_ragged(self, planes, legal_idx, legal_off) -> tuple[np.ndarray, np.ndarray]:
        """cattus_hip_apply_legal on its own layout: legal_idx uint16 ``[total]``, legal_off uint32 ``[n + 1]`` -> (probs ``[total]``, values ``[n]``)."""
        planes = self._planes(planes)
        n = planes.shape[0]
        idx = np.ascontiguousarray(legal_idx, dtype=np.uint16).reshape(-1)
        off = np.ascontiguousarray(legal_off, dtype=np.uint32).reshape(-1)
        if len(off) != n + 1:
            raise ValueError("apply_legal_ragged: legal_off must have n + 1 entries")
        # a table the library will refuse may point past the list: both buffers cover whatever it names
        total = len(idx)
        need = max(total, int(off.max()), 1)
        idx = np.concatenate([idx, np.zeros(need - len(idx), dtype=np.uint16)])
        probs = np.zeros((need,), dtype=np.float32)
        value = np.empty((n,), dtype=np.float32)
        _check(self._lib.cattus_hip_apply_legal(self._h, _u64(planes), n, idx.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                off.ctypes.data_as(C.POINTER(C.c_uint32)), _f32(probs), _f32(value)))
        return probs[:total], value

    # -- introspection ----------------------------------------------------------------------
    def stats(self) -> dict:
        s = Stats()
        _check(self._lib.cattus_hip_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in Stats._fields_}

    # -- verification against a shadow f32 tower (include/cattus_hip.h, cattus_hip_verify) ----
    def verify(self, every: int, blob: bytes | None = None):
        """Check every ``every``-th batch of eval / eval_legal / the leaf server against an f32 evaluator of the same blob, built
        here on first use (a second copy of the weights in f32; a verified batch costs an f32 pass on top of its own); 0 turns it
        off and keeps the record.  The outputs returned are the evaluator's own either way.  blob: the evaluator's own unless
        given (the library refuses any other)."""
        blob = self._blob if blob is None else blob
        _check(self._lib.cattus_hip_verify(self._h, blob, len(blob), int(every)))

    def verify_stats(self) -> dict:
        """The sticky record: every, batches, leaves, leaves_outside (of the reference's cross-runtime bar: > 0 means what
        saturated > 0 means), max_dlogit with its move and both logits (logit_ref the f32 one), max_dvalue with both values."""
        s = VerifyStats(struct_size=C.sizeof(VerifyStats))
        _check(self._lib.cattus_hip_verify_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in VerifyStats._fields_ if name not in ("struct_size", "reserved")}

    def verify_worst_planes(self) -> np.ndarray:
        """uint64 ``[C, plane_words]``: the leaf that holds max_dlogit (raises with status CATTUS_E_STATE before any was verified)."""
        out = np.zeros((self.desc.planes, self.plane_words), dtype=np.uint64)
        _check(self._lib.cattus_hip_verify_worst_planes(self._h, _u64(out)))
        return out

    def verify_prior_stats(self) -> dict:
        """The priors part of the sticky record (cattus_prior_stats): what the legal-move priors of the verified ``eval_legal`` batches and ``submit_legal`` / ``apply_legal`` leaves and every
        verified batch's values differ by from the exact network's -- batches, batches_without_legal, leaves, top1_flips, nonfinite, empty,
        sum_tv, sum_regret, max_tv, max_regret, tv_hist (upper edges 1e-7 .. 1e-1, inf), value_leaves, sum_dvalue -- and derived from them
        tv_mean and regret_mean over the leaves that entered the sums and dvalue_mean over value_leaves (0.0 where there are none)."""
        s = PriorStats(struct_size=C.sizeof(PriorStats))
        _check(self._lib.cattus_hip_verify_prior_stats(self._h, C.byref(s)))
        out = {name: getattr(s, name) for name, _ in PriorStats._fields_ if name not in ("struct_size", "reserved", "tv_hist")}
        out["tv_hist"] = list(s.tv_hist)
        summed = s.leaves - s.nonfinite - s.empty
        out["tv_mean"] = s.sum_tv / summed if summed else 0.0
        out["regret_mean"] = s.sum_regret / summed if summed else 0.0
        out["dvalue_mean"] = s.sum_dvalue / s.value_leaves if s.value_leaves else 0.0
        return out

    def verify_worst_prior(self, cap: int = 1024) -> dict:
        """The leaf that holds max_tv: ``planes`` uint64 ``[C, plane_words]``, ``legal_idx`` uint16 ``[count]``, ``top`` and ``top_ref``, this
        evaluator's favourite and the exact network's as positions in that list (raises with status CATTUS_E_STATE before any leaf was
        compared, CATTUS_E_INVALID when ``cap`` is below the leaf's legal count)."""
        planes = np.zeros((self.desc.planes, self.plane_words), dtype=np.uint64)
        legal = np.zeros((max(int(cap), 1),), dtype=np.uint16)
        count, top, top_ref = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(self._lib.cattus_hip_verify_worst_prior(self._h, _u64(planes), legal.ctypes.data_as(C.POINTER(C.c_uint16)), int(cap), C.byref(count),
                                                       C.byref(top), C.byref(top_ref)))
        return {"planes": planes, "legal_idx": legal[: count.value].copy(), "top": top.value, "top_ref": top_ref.value}

    # -- layer-level observation (include/cattus_hip.h, cattus_hip_tap / cattus_hip_trace) ----
    def points(self) -> int:
        """P = 2 + 2 * blocks: point 0 the stem's output, 2i + 1 / 2i + 2 block i behind its first conv / its output, P - 1 the head convs'."""
        p = C.c_uint32()
        _check(self._lib.cattus_hip_points(self._h, C.byref(p)))
        return p.value

    def tap(self, planes, point: int, outputs: bool = False):
        """The activations at ``point`` for the leaves ``planes`` (at most batch_size): float32 ``[n, C, S, S]`` in the reference's layout and
        in network units, decoded exactly from whatever this evaluator stores there (C = filters, or vhc + phc at the last point: value
        channels first).  outputs=True: ``(tap, logits, values)`` of that pass.  Not counted as a batch."""
        planes = self._planes(planes)
        n, d = planes.shape[0], self.desc
        if not 0 <= int(point) < 2**32:
            raise ValueError(f"tap: point {point}")
        channels = d.filters if int(point) + 1 < 2 + 2 * d.blocks else d.vhc + d.phc
        out = np.empty((n, channels, d.board, d.board), dtype=np.float32)
        policy, value = np.empty((n, d.moves), dtype=np.float32), np.empty((n,), dtype=np.float32)
        _check(self._lib.cattus_hip_tap(self._h, _u64(planes), n, int(point), _f32(out), _f32(policy) if outputs else None, _f32(value) if outputs else None))
        return (out, policy, value) if outputs else out

    def trace(self, planes, blob: bytes | None = None, points: int | None = None):
        """The leaves ``planes`` (at most batch_size) through this evaluator's arithmetic and through the f32 shadow's in lockstep, compared on
        the device at every point: ``(records, logits, values)``, records a structured array ``[P, n]`` of dtype TRACE_RECORD -- max_diff with
        its index ``at`` = channel * S * S + pixel and both values there (``ref`` the shadow's), rms_diff and rms_ref over the leaf's
        elements, flags bit 0 a non-finite value.  The first point whose rms_diff / rms_ref jumps is where the evaluator leaves the exact
        network.  The shadow is ``verify``'s (built here on first use, from the evaluator's own blob unless ``blob`` is given; the library
        refuses any other).  Not counted as a batch; refused for dtype f32."""
        planes = self._planes(planes)
        n, d = planes.shape[0], self.desc
        blob = self._blob if blob is None else blob
        P = 2 + 2 * d.blocks if points is None else int(points)
        rec = np.zeros((P, n), dtype=TRACE_RECORD)
        policy, value = np.empty((n, d.moves), dtype=np.float32), np.empty((n,), dtype=np.float32)
        _check(self._lib.cattus_hip_trace(self._h, blob, len(blob), _u64(planes), n, rec.ctypes.data, P, _f32(policy), _f32(value)))
        return rec, policy, value

    def tower_kernel(self) -> str:
        """Name of the kernel that runs this evaluator's tower."""
        return self._lib.cattus_hip_tower_kernel(self._h).decode()

    def stream_shift(self) -> int:
        """t: the f16 towers carry the residual stream at 2^t times its size (0 for f32 and bf16; include/cattus_hip_diag.h)."""
        return self._lib.cattus_hip_stream_shift(self._h)

    def stream_shifts(self) -> np.ndarray:
        """t_k per stream channel (filters entries, each >= stream_shift() unless calibration's headroom guard lowered it, or -- under
        tower_form="winograd_f4", whose activations are capped at 655 -- the estimate's ceiling held back a channel far above the
        median: t_k then lies below stream_shift(), never below 0; include/cattus_hip_diag.h)."""
        out = np.zeros(self.desc.filters, dtype=np.intc)
        _check(self._lib.cattus_hip_stream_shifts(self._h, out.ctypes.data_as(C.POINTER(C.c_int)), len(out)))
        return out

    def stream_range(self, planes) -> tuple[np.ndarray, np.ndarray]:
        """(rms ``[filters]``, abs_max ``[filters]``) of the residual stream's channels over the leaves ``planes`` (any number: walked
        in chunks of batch_size), their pixels and the 1 + blocks stream tensors, measured on the exact f32 tower: a dtype f32
        evaluator only (cattus_hip_stream_range)."""
        planes = self._planes(planes)
        out = (ChannelRange * self.desc.filters)()
        _check(self._lib.cattus_hip_stream_range(self._h, _u64(planes), planes.shape[0], out, self.desc.filters))
        a = np.frombuffer(out, dtype=np.float32).reshape(-1, 2)
        return a[:, 0].copy(), a[:, 1].copy()

    def stem_input(self) -> tuple[int, bool]:
        """(input channels of the stem conv as laid out on the device, whether the plane pack runs as its own launch in front of it):
        include/cattus_hip_diag.h.  f16x2 has 32 channels where the stem expands the planes itself, a multiple of 64 where they are
        packed first (more than 32 planes, or CATTUS_FUSED_STEM=0)."""
        channels, packed = C.c_uint32(), C.c_uint32()
        _check(self._lib.cattus_hip_stem_input(self._h, C.byref(channels), C.byref(packed)))
        return channels.value, bool(packed.value)

    def mfma_sustained(self, seconds: float = 1.0) -> float:
        """TFLOP/s the device's matrix pipe sustains on back-to-back MFMAs of this evaluator's tower kind (diagnostic)."""
        t = C.c_double()
        _check(self._lib.cattus_hip_mfma_sustained(self._h, float(seconds), C.byref(t)))
        return t.value

    def splitk_plan(self) -> tuple[int, list[int]]:
        """(W, boundaries) of a tower_form="direct_splitk" evaluator: wave w of a workgroup walks the 32-channel input chunks
        boundaries[w] .. boundaries[w + 1] - 1 of every layer behind the stem (include/cattus_hip_diag.h).  A function of the filter count
        alone (and of CATTUS_SPLITK_WAYS); any other evaluator raises CattusHipError with status -2."""
        ways = C.c_uint32()
        bounds = (C.c_uint32 * 9)()
        _check(self._lib.cattus_hip_splitk_plan(self._h, C.byref(ways), bounds))
        return ways.value, [int(b) for b in bounds[: ways.value + 1]]

    def tail_leaves(self) -> int:
        """``tail_leaves`` as it holds for this evaluator: what it was created with on a Winograd F(2x2,3x3) plan, 0 on every other."""
        k = C.c_uint32()
        _check(self._lib.cattus_hip_tail_leaves(self._h, C.byref(k)))
        return k.value

    def head_chain(self, leaves: int) -> None:
        """``cattus_hip_head_chain``: batches of at most ``leaves`` leaves run value FC1 + FC2 and the policy FC on head_fc_chain_kernel (one output element
        per lane, an fmaf chain in the MFMA's order: the same bits); 0: the MFMA pair for every batch, the default.  More than ``batch_size`` is refused;
        accepted and ignored where the heads are not the f32 MFMA heads ("bf16", more than 32 head channels, a SimpleTwoHeadedModel)."""
        _check(self._lib.cattus_hip_head_chain(self._h, int(leaves)))

    def head_chain_leaves(self) -> int:
        """The ``head_chain`` setting as it holds for this evaluator: 0 where it is off or ignored."""
        k = C.c_uint32()
        _check(self._lib.cattus_hip_head_chain_leaves(self._h, C.byref(k)))
        return int(k.value)

    def head_chain_batches(self) -> int:
        """Batches whose FC pair took the chain form since the evaluator was created."""
        k = C.c_uint64()
        _check(self._lib.cattus_hip_head_chain_batches(self._h, C.byref(k)))
        return int(k.value)

    def fused_heads(self, on: bool) -> None:
        """``cattus_hip_fused_heads``: the resident "f16" (tower_form "resident") and "f16r_resident" towers run the two 1x1 head convs in the tail of their one
        launch, on the f32 rows still in LDS, instead of writing the rows to memory for ``head_conv_kernel<float>`` (the same bits; two launches per pass
        instead of three); False: the launch of their own, the default.  Accepted and ignored on every other plan -- "bf16" and "f16x2" resident towers
        run the head convs in their tails always, "f32_resident" keeps the launch."""
        _check(self._lib.cattus_hip_fused_heads(self._h, 1 if on else 0))

    def fused_heads_effective(self) -> bool:
        """The ``fused_heads`` setting as it holds for this evaluator: False where it is off or ignored."""
        k = C.c_uint32()
        _check(self._lib.cattus_hip_fused_heads_effective(self._h, C.byref(k)))
        return bool(k.value)

    def fused_heads_batches(self) -> int:
        """Passes that ran the head convs in the tower's tail since the evaluator was created."""
        k = C.c_uint64()
        _check(self._lib.cattus_hip_fused_heads_batches(self._h, C.byref(k)))
        return int(k.value)

    def tail_batches(self) -> int:
        """Batches that took the short path (at most ``tail_leaves()`` leaves) since the evaluator was created."""
        k = C.c_uint64()
        _check(self._lib.cattus_hip_tail_batches(self._h, C.byref(k)))
        return k.value

    def time_tower(self, n: int, reps: int) -> tuple[float, int]:
        """(average device microseconds of one tower conv launch, launches per forward)."""
        us, launches = C.c_float(), C.c_uint32()
        _check(self._lib.cattus_hip_time_tower(self._h, n, reps, C.byref(us), C.byref(launches)))
        return us.value, launches.value
