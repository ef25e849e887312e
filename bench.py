#!/usr/bin/env python3
"""Headline benchmark: MCTS node-evaluations per second on the chess 20x256 network, batch 256.

One "step" = one pass of the leaf-evaluation hot path over one batch of 256 synthetic leaf
positions: bitboard planes (already resident in HBM) -> 41 fused 3x3 conv+BN+ReLU launches (the stem
expands the planes itself) -> policy/value heads -> logits + values in HBM.  ``value`` is leaves evaluated per
second summed over all ranks (weak scaling: every GPU runs its own batch stream, as self-play
games shard across GPUs with no collective on the evaluation path).

The headline dtype is ``f16x2``, the split-precision tower: inside the reference's own cross-runtime tolerance per leaf
and, at search level, the visit distributions of the exact-f32 search.

A plain run does only what the headline needs: set-up, the settling steps and the W warm-up steps, the K timed steps, the
outputs of the last timed step when ``--dump-outputs DIR`` is given (``DIR/policy.npy`` [batch, moves] logits and
``DIR/value.npy`` [batch] values, float32; the inputs are seeded, so two builds can be compared output for output), and
the result line.  With ``--full`` the same JSON line also carries
  roofline                the tower kernel's event-timed launches, clock / power under load and the sustained MFMA rate
  two_batches_in_flight   the same K steps on the evaluator's two lanes (``--lanes 2``)
  bf16                    the same steps on the bf16 tower (throughput mode, 8 significant bits), with its own roofline
  f16                     the same steps on the single-term f16 tower (throughput mode, 11 significant bits), with its own roofline
  f32                     the same steps on the exact-f32 tower (bit-identical to the CPU oracle), with its own roofline
  search_agreement        what each reduced-cost tower does to the SEARCH: 800-sim searches of the same positions with
                          the f32 tower and with it (cattus_amd/agreement.py)
  selfplay                BASELINE config 3 end to end: C++ search at 800 sims/move feeding this GPU (bounded sample)
  selfplay_full_games     whole games at a reduced simulation count (a measured games/hour)
  selfplay_config4        BASELINE config 4's shape: 64 concurrent games per GPU, records pooled over RCCL in the timed path
  cpu_baseline            the CPU path on this host's cores: evaluator (oracle C port and torch CPU) and search + oracle network
  roofline_plane_pack     HBM roofline of the stand-alone plane-pack kernel

    python bench.py                       # 1 GPU, defaults: the headline only
    python bench.py --full                # the headline and every measurement above
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
"""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

# kernel arguments in device memory (read by the HIP runtime when it initialises)
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

# dense MFMA peaks, /opt/skills/guides/MI355X_MICROARCH.md: the f16 and bf16 forms issue at the same rate
MFMA_PEAK_TFLOPS = {"f16x2": 2500.0, "bf16": 2500.0, "f16": 2500.0, "f32": 157.3}
# MFMA instructions executed per algorithmic multiply-add term: the split tower computes a_hi w_hi + a_lo w_hi + a_hi w_lo
MFMA_TERMS = {"f16x2": 3, "bf16": 1, "f16": 1, "f32": 1}


def mfma_terms(dtype: str, kernel: str) -> float:
    """MFMA instructions per algorithmic multiply-add of the tower kernel: the Winograd F(2x2, 3x3) form of the split tower needs
    16 instead of 36 products per 2x2 output tile and input channel, each still three f16 terms."""
    return MFMA_TERMS[dtype] * (16.0 / 36.0 if kernel in WINOGRAD_KERNELS else 1.0)


WINOGRAD_KERNELS = ("conv3x3_wino_kernel", "conv3x3_wino4_kernel", "tower_wino4_kernel", "conv3x3_wino8_kernel")
# What the chip's L2s deliver to the CUs when every CU streams rows that its XCD's L2 holds (MI355X_MICROARCH.md, "Indexed rows:
# gather into LDS": 66-73 GB/s per CU, 16.8-18.8 TB/s chip-wide): the roof of a kernel whose loop is a stream of L2-resident operands
L2_DELIVERY_TBPS = (16.8, 18.8)
# (rows, couts) of a workgroup's tile: the bytes a workgroup pulls from L2 per layer are its U block (cout_wg x cin x 16 frequencies x
# (hi, lo) f16 = 64 B per (cout, cin)) + its input rows (rows_wg x cin x 4 B) + its skip tile (rows_wg x cout_wg x 4 B, every second layer)
WINOGRAD_WG_TILE = {"conv3x3_wino_kernel": (128, 128), "conv3x3_wino4_kernel": (256, 64), "tower_wino4_kernel": (256, 64), "conv3x3_wino8_kernel": (256, 64)}


def delivery_roof(kernel: str, filters: int, rows: int, launch_us: float):
    """L2 -> CU delivery of a Winograd tower launch, from the kernel's own constants: bytes every workgroup pulls per launch x
    workgroups / the measured launch duration, against the guide's measured L2 read-out rate."""
    if kernel not in WINOGRAD_WG_TILE or launch_us <= 0:
        return None
    rows_wg, cout_wg = WINOGRAD_WG_TILE[kernel]
    wgs = -(-rows // rows_wg) * (filters // cout_wg)
    u, act, skip = cout_wg * filters * 64, rows_wg * filters * 4, rows_wg * cout_wg * 4 // 2
    per_wg = u + act + skip
    tbps = per_wg * wgs / (launch_us * 1e-6) / 1e12
    return {
        "bytes_per_workgroup": per_wg, "of_which_weights_U": u, "of_which_input_rows": act, "of_which_skip_rows_avg": skip,
        "workgroups": wgs, "bytes_per_launch": per_wg * wgs, "achieved_TBps": tbps,
        "roof_TBps": list(L2_DELIVERY_TBPS), "frac_of_roof": [tbps / L2_DELIVERY_TBPS[1], tbps / L2_DELIVERY_TBPS[0]],
        "roof_source": "MI355X_MICROARCH.md, rows shared through the XCDs' L2s gathered by every CU: 16.8-18.8 TB/s chip-wide",
        "note": "every byte counted once per workgroup that loads it (U is re-read by every workgroup of its cout group: L2 hits, not HBM)",
    }

DTYPE_NOTE = {
    "f16x2": "split precision: operands as pairs of f16 values (22 significant bits), three f16 MFMA terms per product, f32 accumulation, "
             "f32 heads; inside the reference's cross-runtime tolerance (training/tests/test_net_output.py:28-33).  At batch > 128 on 8x8 "
             "boards the tower runs in Winograd F(2x2,3x3) form (roofline.kernel says which): 2.25x fewer MFMAs, same tolerance, the f32 "
             "search's visit counts in 2,048 of 2,048 searches",
    "bf16": "bf16 operands, f32 accumulation: throughput mode, 8 significant bits, outside the reference's tolerance",
    "f16": "single-term f16 operands (weights pre-scaled per output channel), f32 accumulation, f32 heads: throughput mode, 11 significant "
           "bits, outside the reference's tolerance; 99.4 % of the f32 search's moves (bf16: 95 %)",
    "f32": "exact-f32 MFMA tower (v_mfma_f32_32x32x2_f32): bit-identical to the CPU oracle",
}
# node-evals/s one GPU sustains per dtype (sizes the bounded self-play samples; measured round 3)
EVAL_CAPACITY = {"f16x2": 150e3, "bf16": 330e3, "f16": 290e3, "f32": 44e3}

WORKLOADS = {
    # BASELINE.json configs[2]: the configuration the metric is quoted on
    "chess20x256": dict(game="chess", blocks=20, filters=256, vhc=8, phc=8, batch=256, seed=2),
    # configs[1] and configs[4], selectable for extra measurements
    "hex7_6x64": dict(game="hex7", blocks=6, filters=64, vhc=16, phc=16, batch=128, seed=1),
    "chess40x384": dict(game="chess", blocks=40, filters=384, vhc=8, phc=8, batch=512, seed=3),
    # the headline net at other batch sizes (how the fixed cost per launch amortises)
    "chess20x256_b512": dict(game="chess", blocks=20, filters=256, vhc=8, phc=8, batch=512, seed=2),
    "chess20x256_b1024": dict(game="chess", blocks=20, filters=256, vhc=8, phc=8, batch=1024, seed=2),
    "chess20x256_b128": dict(game="chess", blocks=20, filters=256, vhc=8, phc=8, batch=128, seed=2),
    # the reference's own configured nets (training/config/*.yaml): 7x16 and 5x8 filters
    "chess7x16": dict(game="chess", blocks=7, filters=16, vhc=8, phc=8, batch=256, seed=4),
    "hex7_7x16": dict(game="hex7", blocks=7, filters=16, vhc=16, phc=16, batch=128, seed=5),
}

SELFPLAY_SETTINGS = dict(temperature_policy=[(30, 1.0), (9999, 0.0)], prior_noise_alpha=0.03, prior_noise_epsilon=0.25)
SELFPLAY_SETTINGS_TEXT = "temperature 1.0 for 30 moves then 0, Dirichlet noise 0.03/0.25, cache 1e6, batch 256 (training/config/chess_dev.yaml:52-68)"


def make_workload(name: str):
    from cattus_amd import synth
    from cattus_amd.weights import CHESS, NetDesc, hex_game, seeded_blob

    w = WORKLOADS[name]
    if w["game"] == "chess":
        d = NetDesc(**CHESS, blocks=w["blocks"], filters=w["filters"], vhc=w["vhc"], phc=w["phc"])
        planes = synth.random_chess_planes(w["batch"], w["seed"])
    else:
        d = NetDesc(**hex_game(7), blocks=w["blocks"], filters=w["filters"], vhc=w["vhc"], phc=w["phc"])
        planes = synth.random_hex_planes(w["batch"], 7, w["seed"])
    return d, seeded_blob(d, w["seed"]), planes


# ------------------------------------------------------------------------------------------ CPU baseline


def cpu_baseline(blob, planes, budget_s: float = 12.0):
    """The CPU path on this host, bounded samples.  `evaluator`: the oracle network (oracle/oracle_net.c, a plain C
    port of the same arithmetic, OpenMP over leaves) on the bench leaves, on every CPU this process may use
    (cgroup quota, not the affinity mask) and on one thread.  `selfplay`: the C++ search of this repository with
    the oracle network behind its network callback (no Python in the loop), one search thread per CPU -- the
    reference's threading model -- on hex7 6x64 and chess 20x256, games cut after a few plies so that each
    sample costs about `budget_s`.  The reference's own Rust path cannot be built on this box (no Rust toolchain)."""
    from cattus_amd import selfplay as sp
    from cattus_amd.weights import NetDesc, hex_game, seeded_blob
    from oracle import oracle

    cores = oracle.default_threads()
    net = oracle.OracleNet(blob)

    def timed(n, threads):
        t0 = time.perf_counter()
        net.forward(planes[:n], threads=threads)
        return time.perf_counter() - t0

    timed(min(len(planes), cores), cores)  # warm-up: thread pool, scratch buffers
    dt1 = timed(1, 1)
    n1 = int(max(1, min(8, 2.0 / dt1)))
    dt1 = timed(n1, 1)
    n = cores
    dt = timed(n, cores)
    n = int(min(len(planes), max(cores, (budget_s * n / dt) // cores * cores)))
    dt = timed(n, cores)
    oracle_entry = {"value": n / dt, "cores": cores, "kind": "port", "what": "oracle/oracle_net.c: plain C restatement of the f32 arithmetic, OpenMP over leaves",
                    "one_thread": n1 / dt1, "sample": f"{n} leaves on {cores} threads in {dt:.1f} s; {n1} leaves on one thread in {dt1:.1f} s"}
    # The same network as a plain torch module on the CPU (cattus_amd/torch_model.py: this repository's own module with the
    # reference checkpoint's key names; fp32, oneDNN convolutions) -- the fair CPU evaluator figure: a tuned CPU library, not a
    # scalar port.  The reference's own runtimes (ORT / tract / ExecuTorch) are not in this image.
    torch_entry = None
    try:
        import torch

        from cattus_amd.torch_model import PolicyValueNet

        d = PolicyValueNet.from_blob(blob).desc
        tnet = PolicyValueNet.from_blob(blob)
        bits = np.unpackbits(planes.view(np.uint8).reshape(len(planes), d.planes, -1), axis=-1, bitorder="little")
        x = torch.from_numpy(bits[..., : d.hw].reshape(len(planes), d.planes, d.board, d.board).astype(np.float32))
        old_threads = torch.get_num_threads()

        def ttimed(nn_, threads, reps=1):
            torch.set_num_threads(threads)
            with torch.no_grad():
                t0 = time.perf_counter()
                for _ in range(reps):
                    tnet(x[:nn_])
                return time.perf_counter() - t0

        ttimed(min(len(x), 2 * cores), cores)  # warm-up: oneDNN primitive creation, thread pool
        nt = len(x)  # whole bench batches, repeated until the sample costs about budget_s
        tdt = ttimed(nt, cores)
        reps = int(max(1, min(200, budget_s * 0.8 / tdt)))
        tdt = ttimed(nt, cores, reps)
        nt *= reps
        ttimed(1, 1)
        nt1 = int(max(1, min(64, 3.0 / max(ttimed(1, 1), 1e-3))))
        tdt1 = ttimed(nt1, 1)
        torch.set_num_threads(old_threads)
        torch_entry = {"value": nt / tdt, "cores": cores, "kind": "port", "what": f"cattus_amd/torch_model.py on torch {torch.__version__} CPU (fp32, oneDNN)",
                       "one_thread": nt1 / tdt1, "sample": f"{nt} leaves in batches of {len(x)} on {cores} threads in {tdt:.1f} s; {nt1} leaves on one thread in {tdt1:.1f} s"}
    except Exception as exc:  # noqa: BLE001 - the baseline is a report, not the product
        torch_entry = {"error": repr(exc)}
    best = max([e for e in (oracle_entry, torch_entry) if e and "value" in e], key=lambda e: e["value"])
    out = {
        "value": best["value"],
        "unit": "node-evals/s",
        "cores": cores,
        "kind": "port",
        "sample": best["what"] + ": " + best["sample"],
        "evaluator": {"oracle_c": oracle_entry, "torch_cpu": torch_entry},
    }

    # ---- the path: search + network, one search thread per CPU, each blocking on its own leaf (batch_size 1)
    def path(game, oblob, oplanes, words, sims, settings):
        onet = oracle.OracleNet(oblob)
        onet.forward(oplanes[:cores], threads=cores)
        t0 = time.perf_counter()
        onet.forward(oplanes[: 4 * cores], threads=cores)
        rate = 4 * cores / (time.perf_counter() - t0)
        games = max(2, cores // 2 * 2)
        # bounded sample: every game is cut after `plies` plies so that the leg costs about budget_s at that rate
        plies = int(max(1, min(64, budget_s * rate / (games * sims))))
        fn, ctx, keep = onet.callback(plane_words=words, threads=1)
        cfg = sp.make_config(sim_num=sims, batch_size=1, threads=cores, concurrent_games=games, cache_size=1000000, eval_threads=cores,
                             max_game_plies=plies, seed=1, **settings)
        t0 = time.perf_counter()
        res = sp.run_self_play(game, cfg, sp.Net.raw(fn, ctx, keep), None, games, keep_records=False)
        secs = time.perf_counter() - t0
        return {"node_evals_per_sec": res["node_evals"] / secs, "plies_per_sec": res["positions"] / secs, "games": games,
                "sims_per_move": sims, "max_game_plies": plies, "games_adjudicated_at_ply_limit": int(res["adjudicated"]),
                "cores": cores, "seconds": secs, "evaluator_only_rate": rate}

    from cattus_amd import synth

    dh = NetDesc(**hex_game(7), blocks=6, filters=64, vhc=16, phc=16)
    out["selfplay"] = {
        "hex7_6x64": path("hex7", seeded_blob(dh, 1), synth.random_hex_planes(4 * cores, 7, 1), 2, 100, {}),
        # 64 simulations per move instead of the GPU leg's 800: one 800-sim move per game would already cost minutes here
        "chess20x256": path("chess", blob, planes, 1, 64, SELFPLAY_SETTINGS),
        "note": "C++ search (this repository) + oracle network through the C callback, one blocking search thread per CPU, batch_size 1; "
                "games are cut after max_game_plies plies (bounded sample)",
    }
    return out


# ------------------------------------------------------------------------------------------ plane pack roofline


def pack_roofline(torch, ev_lib, dev, stream, leaves: int = 262144, reps: int = 20):
    """HBM roofline of the stand-alone plane-pack kernel (reference layout, f32 NCHW; the drop-in for
    planes_to_tensor, engine/src/net/mod.rs:121-156): chess planes for `leaves` positions (1.25 GB of
    output, far beyond the 256 MiB Infinity Cache), timed with events on the launch stream.
    Algorithmic bytes per leaf = 18*8 in + 18*64*4 out = 4752."""
    import ctypes as C

    planes = torch.randint(0, 2**62, (leaves, 18, 1), dtype=torch.int64, device=dev)
    out = torch.empty((leaves, 18, 8, 8), dtype=torch.float32, device=dev)

    def launch():
        rc = ev_lib.cattus_hip_planes_to_tensor_device(planes.data_ptr(), leaves, 18, 1, 8, leaves, out.data_ptr(), C.c_void_p(stream.cuda_stream))
        assert rc == 0

    with torch.cuda.stream(stream):
        for _ in range(3):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            launch()
        e1.record(stream)
        e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    nbytes = leaves * 4752
    # spot check against the definition
    host = out[:4].cpu().numpy().reshape(4, 18, 64)
    bits = planes[:4].cpu().numpy().view("uint64").reshape(4, 18)
    for b in range(4):
        for c in range(18):
            want = [(int(bits[b, c]) >> i) & 1 for i in range(64)]
            assert host[b, c].astype(int).tolist() == want
    achieved = nbytes / (us * 1e-6) / 1e9
    return {
        "kernel": "planes_to_tensor_nchw64_kernel",
        "bound": "hbm",
        "achieved": achieved,
        "peak": 8000.0,
        "unit": "GB/s",
        "frac": achieved / 8000.0,
        # MI355X_MICROARCH.md measures 6.29 TB/s for a float4 copy and 6.0-6.2 TB/s for plain store streams: what a
        # write-dominated kernel (144 B in, 4,608 B out per leaf) can reach of the 8 TB/s specification
        "achievable": 6300.0,
        "frac_of_achievable": achieved / 6300.0,
        "traffic": measured_traffic("planes_to_tensor_nchw64_kernel", "any")[0],
        "traffic_source": measured_traffic("planes_to_tensor_nchw64_kernel", "any")[1],
        "avg_launch_us": us,
        "leaves_per_launch": leaves,
        "bytes_per_leaf": 4752,
        "note": "stand-alone planes_to_tensor drop-in (cattus_hip_planes_to_tensor_device, reference layout); inside the forward pass "
                "the planes are expanded by the stem conv's loader waves straight into LDS (no separate launch, no packed tensor in HBM)",
    }


TRAFFIC_FILE = "profiles/r05_pmc_hbm_traffic.json"


def kernels_sha256() -> str:
    """Identity of the kernel CODE the traffic counters were collected on: sha256 of the kernel sources (device_common.h,
    kernels.h, kernels.hip, kernels_t64s.hip, kernels_wino.hip, kernels_wino4.hip, kernels_wino8.hip) with their `//` comments and all white space removed (an edited
    comment does not make a measurement stale; the files have no block comments and no `//` inside a string literal)."""
    names = ("device_common.h", "kernels.h", "kernels.hip", "kernels_t64s.hip", "kernels_wino.hip", "kernels_wino4.hip", "kernels_wino8.hip")
    text = "".join((ROOT / "cattus_amd" / "csrc" / name).read_text() for name in names)
    code = "".join("".join(line.split("//", 1)[0].split()) for line in text.splitlines())
    return hashlib.sha256(code.encode()).hexdigest()


def measured_traffic(kernel: str, dtype: str = "f16x2"):
    """(HBM-side bytes per launch, where they come from) from the committed rocprofv3 PMC passes (separate --pmc
    FETCH_SIZE / WRITE_SIZE runs, gfx950 x2 fetch correction: scripts/collect_profiles.sh + scripts/make_traffic_json.py).
    The counters cannot be collected inside this process, so the file carries the sha256 of kernels.hip it was
    collected on: when the kernels have changed since, the figure is withheld (None) rather than reported stale."""
    try:
        with open(ROOT / TRAFFIC_FILE) as f:
            t = json.load(f)
        entry = t["by_dtype"][dtype][kernel]
    except (OSError, KeyError, ValueError):
        return None, f"no PMC pass for this kernel / dtype in {TRAFFIC_FILE}"
    if t.get("kernels_sha256") != kernels_sha256():
        return None, f"withheld: {TRAFFIC_FILE} was collected on another version of kernels.hip (re-run scripts/collect_profiles.sh)"
    return entry["traffic_bytes_per_launch"], f"{TRAFFIC_FILE} (rocprofv3 --pmc passes, commit {t.get('commit', '?')}, same kernels.hip)"


# ------------------------------------------------------------------------------------------ self-play legs


def search_threads(sp, world: int) -> int:
    """Search threads of one rank: its CPU share (the cgroup quota split over the ranks, or -- once cattus_amd.affinity
    has pinned the rank -- its own mask) minus room for the two evaluation threads, the HIP runtime's threads and the
    main thread (15 search threads on a 16-CPU share starved them: 261 k vs 337 k node-evals/s)."""
    share = min(sp.available_cpus() // max(1, min(world, 8)), len(os.sched_getaffinity(0)))
    return max(1, share - 4)


def selfplay_leg(blob, dtype, local_rank, rank, world, *, games, slots, sims, max_game_plies, keep_records, pool, torch, dev, batch=256):
    """Real self-play on this rank's shard of the games: C++ search + evaluation cache + this GPU's evaluator
    through cattus_hip_eval (host buffers, PCIe included), the reference's self-play settings.  With `pool`
    the records of all ranks are pooled on rank 0 by cattus_amd.dist.pool_records (gather) and the counters
    all-reduced, inside the timed region."""
    from cattus_amd import dist as cdist
    from cattus_amd import selfplay as sp
    from cattus_amd.evaluator import HipEvaluator

    # search threads: the CPU share of this rank minus room for the two evaluation threads, the HIP runtime's
    # threads and the main thread (15 search threads on a 16-CPU share starved them: 261 k vs 337 k node-evals/s)
    threads = search_threads(sp, world)
    # model.batch_size as a user would configure it for this many concurrent games (one leaf per tree in flight: a batch can never
    # hold more than there are games, and with two batches in flight it holds well under half of them); the evaluator picks its
    # kernels by it (the Winograd form of the f16x2 tower above 128, the small tiles of the direct kernels up to there)
    bsz = min(batch, slots)
    with HipEvaluator(blob, batch_size=bsz, plane_words=1, dtype=dtype, device=local_rank) as ev:
        cfg = sp.make_config(sim_num=sims, batch_size=bsz, threads=threads, concurrent_games=slots, cache_size=1000000,
                             first_game=rank, game_stride=world, seed=1, max_game_plies=max_game_plies,
                             **SELFPLAY_SETTINGS)  # random streams are per global game index
        if world > 1:  # all ranks start the leg together: its rate is the sum of the ranks' evaluations over the slowest rank's time
            import torch.distributed as dist

            dist.barrier()
        t0 = time.perf_counter()
        res = sp.run_self_play("chess", cfg, sp.Net.hip(ev), None, games, keep_records=keep_records)
        play_s = time.perf_counter() - t0
        pooled, pool_s = None, 0.0
        if pool:
            import torch.distributed as dist

            t1 = time.perf_counter()
            recs, _meta = cdist.pool_records(res["record_bytes"], res["record_meta"], device=dev)  # on rank 0; dev: where the collectives run
            tot = cdist.reduce_counters(res, device=dev)
            torch.cuda.synchronize()
            pool_s = time.perf_counter() - t1
            if recs is not None:  # rank 0 holds the pooled set
                pooled = dict(records=int(len(recs)), bytes=int(recs.size), draws=tot["draws"], p1=tot["player1_wins"], p2=tot["player2_wins"])
                assert len(recs) == tot["positions"]
    return dict(seconds=play_s + pool_s, play_seconds=play_s, pool_seconds=pool_s, games=games, node_evals=res["node_evals"],
                batches=res["activation_count"], positions=res["positions"], threads=threads, slots=slots, sims=sims,
                adjudicated=int(res["adjudicated"]), cache_hits=res["cache_hits"],
                steady_rate=res["steady_node_evals"] / max(res["steady_seconds"], 1e-9), pooled=pooled)


def reduce_leg(leg, torch, dev, world):
    """Sum / max the per-rank figures of a self-play leg; returns the JSON object (identical on all ranks)."""
    import torch.distributed as dist

    t = torch.tensor([leg["seconds"], leg["games"], leg["node_evals"], leg["batches"], leg["positions"], leg["steady_rate"],
                      leg["adjudicated"], leg["pool_seconds"], leg["cache_hits"]], dtype=torch.float64, device=dev)
    tmax = t.clone()
    per_rank = [leg["node_evals"] / max(leg["seconds"], 1e-9)]
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        mine = torch.tensor(per_rank, dtype=torch.float64, device=dev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [float(x.item()) for x in allr]
    secs = float(tmax[0].item())
    games, evals, batches, plies = (float(t[i].item()) for i in (1, 2, 3, 4))
    out = {
        "node_evals_per_sec": evals / secs,
        # while >= 3/4 of the concurrent-game slots still have a game to play, i.e. without the drain at the end of
        # this fixed-size run when batches can no longer be filled (sum over GPUs)
        "steady_node_evals_per_sec": float(t[5].item()),
        "plies_per_sec": plies / secs,
        "games": int(games),
        "games_adjudicated_at_ply_limit": int(t[6].item()),
        "sims_per_move": leg["sims"],
        "plies_per_game": plies / max(1.0, games),
        "batch_fill": evals / max(1.0, batches),
        "cache_hit_rate": float(t[8].item()) / max(1.0, float(t[8].item()) + evals),
        "concurrent_games_per_gpu": leg["slots"],
        "host_threads_per_gpu": leg["threads"],
        "seconds": secs,
        # what the collectives saw: the process group's size and backend, and every rank's own rate
        "ranks": dist.get_world_size() if dist.is_initialized() else 1,
        "collective_backend": dist.get_backend() if dist.is_initialized() else None,
        "node_evals_per_sec_per_rank": per_rank,
    }
    return out


# ------------------------------------------------------------------------------------------ ranks


def spawn_ranks(n: int, argv: list[str]) -> int:
    """One process per GPU (the fan-out of training/self-play/src/self_play.rs:109-137, over processes instead of threads):
    start `python -m torch.distributed.run --nproc-per-node n bench.py <argv>` as a CHILD of this process, pass rank 0's JSON
    line through on stdout and return the launcher's exit status.  Never an exec: the caller has not touched the GPU, and a
    process that has must not be replaced."""
    import socket
    import subprocess

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL between processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "1")             # what torchrun would set (and warn about); the ranks size their own pools
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve()), *argv]
    print("bench.py: starting %d ranks: %s" % (n, " ".join(cmd)), file=sys.stderr, flush=True)
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True)
    lines = []
    for line in proc.stdout:
        try:
            if "metric" in json.loads(line):
                lines.append(line.strip())
                continue
        except ValueError:
            pass
        sys.stderr.write(line)  # anything else a rank or a library wrote to stdout
    rc = proc.wait()
    if len(lines) != 1:
        print(f"bench.py: expected one result line from rank 0, got {len(lines)} (launcher exit status {rc})", file=sys.stderr)
        return rc or 1
    out = json.loads(lines[0])
    if out.get("n_gpus") != n:
        print(f"bench.py: the ranks reported n_gpus={out.get('n_gpus')}, asked for {n}", file=sys.stderr)
        return rc or 1
    sys.stdout.write(lines[0] + "\n")
    sys.stdout.flush()
    return rc


# ------------------------------------------------------------------------------------------ main


def main():
    # stdout carries exactly ONE line, the result JSON: native libraries write to file descriptor 1 too (RCCL prints a
    # version banner when its first communicator comes up), so everything else this process prints goes to stderr
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dtype", choices=["f16x2", "bf16", "f16", "f32"], default="f16x2", help="tower of the headline `value` (default: the split-precision tower)")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="chess20x256")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs as DIR/policy.npy and DIR/value.npy (float32)")
    ap.add_argument("--settle-seconds", type=float, default=0.4,
                    help="untimed steps run for this long IN FRONT of the W warm-up steps (the clock governor needs longer than W steps to settle); 0 = none")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement behind the headline (roofline, two lanes, other towers, search agreement, self-play, "
                         "plane pack, CPU baseline); the options below shape that part only")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-smi", action="store_true", help="do not sample the device's clock / power under load beside the roofline")
    ap.add_argument("--lanes", type=int, choices=[1, 2], default=2,
                    help="2 = also time the K steps with two batches in flight (extra object; `value` stays single-stream)")
    ap.add_argument("--selfplay-seconds", type=float, default=40.0, help="time budget of the 800-sim self-play leg (0 = skip all self-play legs)")
    ap.add_argument("--selfplay-sims", type=int, default=800, help="simulations per move of the end-to-end leg (BASELINE config 3: 800)")
    ap.add_argument("--agreement-plies", type=int, default=4, help="searched plies per game of the search agreement leg (0 = skip)")
    ap.add_argument("--no-f32", action="store_true", help="skip the f32 (bit-exact) object")
    ap.add_argument("--no-bf16", action="store_true", help="skip the bf16 (throughput mode) object")
    ap.add_argument("--no-f16", action="store_true", help="skip the f16 (single-term f16 throughput mode) object")
    ap.add_argument("--side-legs-timeout", type=float, default=480.0,
                    help="seconds the legs behind the headline may take before a watchdog prints the line with what is there and ends the process "
                         "(the default keeps a --full run inside 10 minutes; its legs take about 3)")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py: --steps must be >= 1 and --warmup >= 0")
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:
            # `python bench.py --gpus N` without a launcher: this process -- which has not imported torch, loaded
            # libcattus_hip.so or made any HIP call -- starts N fresh ranks and relays rank 0's line
            os.dup2(json_fd, 1)
            raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))
    elif int(os.environ["WORLD_SIZE"]) != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={os.environ['WORLD_SIZE']} ranks: "
                         "refusing to report a line for a job of another size")

    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the leaf evaluator has no CPU path")
    # Rehearsal of the N > 1 code path on a box with one GPU (never for a quoted number): BENCH_REHEARSAL=1 puts
    # every rank on device 0 and runs the collectives over gloo on host tensors.
    rehearsal = os.environ.get("BENCH_REHEARSAL") == "1"
    if rehearsal:
        local_rank = 0
    if not rehearsal and local_rank >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: rank {rank} wants cuda:{local_rank} but this node shows {torch.cuda.device_count()} devices "
                         "(BENCH_REHEARSAL=1 puts every rank on device 0, for plumbing tests only)")
    # one process per GPU: a disjoint share of the host's CPUs for this rank, on its GPU's NUMA node where sysfs tells
    # (before any thread of the evaluator or the search exists; cattus_amd/affinity.py)
    from cattus_amd import affinity

    cpu_share = affinity.pin_rank(int(os.environ.get("LOCAL_RANK", "0")), local_world,
                                  None if rehearsal else affinity.torch_pci_bus_ids(local_world) if local_world > 1 else None)
    torch.cuda.set_device(local_rank)
    import torch.distributed as dist

    headline = args.workload == "chess20x256"
    want_pg = world > 1 or (args.full and headline and args.selfplay_seconds > 0)  # config 4's leg pools records over RCCL, also on one rank
    pg_note = None
    if want_pg:
        import datetime

        # every collective of this job carries a deadline: a rank that died leaves the others an error, not a hang
        pg_timeout = datetime.timedelta(seconds=float(os.environ.get("BENCH_PG_TIMEOUT", "600")))
        try:
            if rehearsal:
                dist.init_process_group("gloo", timeout=pg_timeout)
            elif world > 1:
                dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank), timeout=pg_timeout)
            else:
                dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{29400 + os.getpid() % 500}", rank=0, world_size=1,
                                        device_id=torch.device("cuda", local_rank), timeout=pg_timeout)
            pg_note = {"backend": dist.get_backend(), "ranks": dist.get_world_size(), "timeout_s": pg_timeout.total_seconds()}
        except Exception as exc:  # noqa: BLE001
            if world > 1:
                raise  # N ranks without a process group cannot report one job
            # one rank: only the config-4 leg wanted it; the headline does not
            pg_note = {"error": f"{type(exc).__name__}: {exc}"}
    if world > 1 and dist.get_world_size() != args.gpus:
        raise SystemExit(f"bench.py: process group of {dist.get_world_size()} ranks, --gpus {args.gpus}")

    from cattus_amd.evaluator import HipEvaluator

    d, blob, planes = make_workload(args.workload)
    batch = len(planes)
    plane_words = planes.shape[2]
    dev = torch.device("cuda", local_rank)
    cdev = torch.device("cpu") if rehearsal else dev  # where the collectives' tensors live
    d_planes = torch.from_numpy(planes.view(np.int64)).to(dev)
    stream = torch.cuda.Stream(device=dev)  # everything timed runs on this stream (not the legacy default stream)

    def sync_all():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if world > 1:
            t = torch.tensor([x], dtype=torch.float64, device=cdev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())
        return x

    def gather_over_ranks(x):
        """x of every rank, in rank order (the GPUs of a node do not hold the same clock under the tower: the job's rate is the
        slowest one's, and this says which)."""
        if world > 1:
            t = [torch.zeros(1, dtype=torch.float64, device=cdev) for _ in range(world)]
            dist.all_gather(t, torch.tensor([x], dtype=torch.float64, device=cdev))
            return [float(v.item()) for v in t]
        return [x]

    def under_load_clock_and_power(step):
        """(sclk MHz, socket power W) while `step` keeps the GPU busy, read from the amdgpu driver's sysfs files of this rank's
        device (what rocm-smi prints; plain file reads: no child process); None where the files are missing."""
        import glob
        import re
        import statistics

        from cattus_amd.affinity import torch_pci_bus_ids

        try:
            ids = torch_pci_bus_ids(local_rank + 1)
            base = f"/sys/bus/pci/devices/{ids[local_rank]}" if ids else None
            if not base or not os.path.exists(base + "/pp_dpm_sclk"):
                return None
            power_files = glob.glob(base + "/hwmon/hwmon*/power1_average") + glob.glob(base + "/hwmon/hwmon*/power1_input")
            sclk, power = [], []
            for _ in range(100):
                step()
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 1.5:
                for _ in range(20):
                    step()
                m = re.search(r"(\d+)Mhz\s*\*", open(base + "/pp_dpm_sclk").read())
                if m:
                    sclk.append(int(m.group(1)))
                if power_files:
                    power.append(int(open(power_files[0]).read()) / 1e6)
                torch.cuda.synchronize()
            if not sclk:
                return None
            return dict(sclk_mhz=int(statistics.median(sclk)), socket_power_w=round(statistics.median(power), 1) if power else None,
                        samples=len(sclk))
        except Exception:  # noqa: BLE001 - a diagnostic; the measurement does not depend on it
            return None

    def time_evaluator(dtype, steps, warmup, lanes=1, settle_s=0.0, extras=True, keep_outputs=False):
        """K steps of the hot path on the `dtype` tower -> dict(elapsed = seconds for the K steps (max over ranks),
        launch_us = event-stamped tower launch duration, launches per step, ...).  `extras` = False leaves out everything
        behind the timed steps (tower launch timing, clock and power, sustained MFMA rate, the two-lane pass); `keep_outputs`
        adds the last timed step's (policy, value) as host arrays."""
        ev = HipEvaluator(blob, batch_size=batch, plane_words=plane_words, dtype=dtype, device=local_rank)
        d_policy = torch.empty((batch, d.moves), dtype=torch.float32, device=dev)
        d_value = torch.empty((batch,), dtype=torch.float32, device=dev)

        def step():
            ev.eval_device(d_planes.data_ptr(), batch, d_policy.data_ptr(), d_value.data_ptr(), stream.cuda_stream)

        # Settling run, untimed, in FRONT of the W warm-up steps: the driver times 20 steps behind 5 warm-up steps, i.e.
        # a few tens of milliseconds after the process touched the GPU for the first time, and the clock governor needs
        # longer than that (round 2: 322 k node-evals/s in that window, 359 k over the 400 steps behind it).  It is
        # reported (`effective_warmup_steps`, `settle`), and its own rate is in the line for comparison.
        settle_steps, settle_ms = 0, None
        if settle_s > 0:
            sync_all()
            t0 = time.perf_counter()
            while True:
                for _ in range(20):
                    step()
                settle_steps += 20
                torch.cuda.synchronize()
                if time.perf_counter() - t0 >= settle_s:
                    break
            sync_all()
            settle_ms = max_over_ranks(time.perf_counter() - t0) / settle_steps * 1e3
        for _ in range(warmup):
            step()
        sync_all()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()  # this rank's own K steps, before it waits for the others at the closing barrier
        own = time.perf_counter() - t0
        sync_all()
        elapsed = max_over_ranks(time.perf_counter() - t0)
        own_all = gather_over_ranks(own)
        # sanity: the timed kernels produced real numbers
        assert bool(torch.isfinite(d_policy).all()) and bool(torch.isfinite(d_value).all())
        outputs = (d_policy.cpu().numpy(), d_value.cpu().numpy()) if keep_outputs else None
        # roofline of the dominant kernel (3x3 conv tower launch): event-stamped launch durations of the same
        # forward, taken right behind the timed region so that the device is in the same state as for `value`
        launch_us, launches = ev.time_tower(batch, 20 if dtype != "f32" else 5) if rank == 0 and extras else (0.0, 1)
        # clock and power while the same steps keep running (sysfs, rank 0, best effort): the 2.5 PF peak is a
        # 2.4 GHz figure, and under its MFMA kernels the part holds less
        smi = under_load_clock_and_power(step) if rank == 0 and extras and not args.no_smi else None
        # what THIS device's matrix pipe sustains on nothing but back-to-back MFMAs of the tower's kind (1 s; rank 0)
        sustained = ev.mfma_sustained(1.0) if rank == 0 and extras and not args.no_smi else None
        elapsed2 = None
        if lanes == 2 and extras:
            # the same K steps with two batches in flight (evaluator lanes 0/1 on two streams), as the self-play
            # driver runs the evaluator: one batch's kernel tails overlap the other's heads
            d_policy2, d_value2 = torch.empty_like(d_policy), torch.empty_like(d_value)
            which = os.environ.get("BENCH_LANE_STREAMS", "lane")  # the evaluator's own lane streams, or two torch streams
            if which == "torch":
                handles = [stream.cuda_stream, torch.cuda.Stream(device=dev).cuda_stream]
            else:
                handles = [ev.lane_stream(0), ev.lane_stream(1)]
            both = [(0, handles[0], d_policy, d_value), (1, handles[1], d_policy2, d_value2)]

            def step2(i):
                lane, st, pol, val = both[i & 1]
                ev.eval_device(d_planes.data_ptr(), batch, pol.data_ptr(), val.data_ptr(), st, lane=lane)

            for i in range(max(2, warmup // 2 * 2)):
                step2(i)
            sync_all()
            t0 = time.perf_counter()
            for i in range(steps):
                step2(i)
            sync_all()
            elapsed2 = max_over_ranks(time.perf_counter() - t0)
            assert bool((d_policy2 == d_policy).all()) and bool((d_value2 == d_value).all())  # lanes agree bit for bit
        kernel = ev.tower_kernel()
        ev.close()
        return dict(elapsed=elapsed, own_all=own_all, steps=steps, launch_us=launch_us, launches=launches, elapsed2=elapsed2, kernel=kernel,
                    settle_steps=settle_steps, settle_ms=settle_ms, smi=smi, sustained=sustained, outputs=outputs)

    def roofline(dtype, r):
        """Dominant kernel = the tower conv launch.  `achieved` counts ALGORITHMIC flops (2 x multiply-adds of the
        network: SURVEY.md section 8d) per launch over the launch's measured duration; `peak` is the dense MFMA peak of
        the operand type the kernel issues.  The split tower issues 3 MFMA terms per algorithmic multiply-add, so the
        share of the matrix pipe it keeps busy is 3 x frac (`mfma_pipe_frac`)."""
        flop_per_launch = d.conv_flops_per_position() * batch / r["launches"]
        achieved = flop_per_launch / (r["launch_us"] * 1e-6) / 1e12
        peak = MFMA_PEAK_TFLOPS[dtype]
        traffic, source = measured_traffic(r["kernel"], dtype) if headline else (None, "collected for the headline workload only")
        smi = r.get("smi")
        under_load = None
        if smi:
            # the peak above is clock 2.4 GHz x 1,024 SIMDs x FLOP per cycle: scaled to the clock the part holds under this
            # kernel it says what share of the ELAPSED matrix-pipe cycles the kernel fills
            scale = smi["sclk_mhz"] / 2400.0
            under_load = dict(smi, source="amdgpu sysfs (pp_dpm_sclk, hwmon power1_average) of this device while the same steps run (untimed); what rocm-smi prints",
                              peak_at_this_clock=peak * scale, mfma_pipe_frac_at_this_clock=mfma_terms(dtype, r["kernel"]) * achieved / (peak * scale))
        sustained = None
        if r.get("sustained"):
            # the nominal peak is a 2.4 GHz figure; under MFMA load the part's power management sets the clock.  A kernel of
            # nothing but back-to-back MFMAs of this kind (one wave per SIMD, operands in registers, ~50 us launches for 1 s)
            # is what the pipe can deliver on THIS device, measured in this run right behind the timed steps
            sustained = dict(tflops=r["sustained"], frac_of_nominal=r["sustained"] / peak,
                             mfma_pipe_frac_of_sustained=mfma_terms(dtype, r["kernel"]) * achieved / r["sustained"],
                             how="cattus_hip_mfma_sustained: back-to-back MFMAs of the tower's kind on every SIMD, no memory traffic, 1 s")
        deliv = delivery_roof(r["kernel"], d.filters, batch * 64, r["launch_us"]) if d.board == 8 else None
        # which roof the kernel is under, from the kernel: the 16-frequency Winograd kernel streams 2 MB of U per CU and layer and sits at
        # ~0.9 of what the L2s deliver -- its MFMA fraction is quoted against a roof it cannot touch, so the line says so
        bound = "l2_delivery" if deliv and deliv["frac_of_roof"][0] >= 0.75 else "mfma"
        return {
            "kernel": r["kernel"],
            "bound": bound,
            "bound_note": "l2_delivery: the loop is a stream of L2-resident operands into the CUs (`delivery`), the matrix pipe waits for it; "
                          "`frac` stays the MFMA fraction on algorithmic FLOPs for comparison across kernels" if bound != "mfma" else
                          # the contract's roof for a tower is the matrix pipe; what keeps THIS kernel from it is neither roof on the line
                          ("mfma is the roof priced here; what the kernel sits under is the issue rate of its one wave per SIMD -- per 48 MFMAs "
                           "(1,536 pipe cycles) the wave issues ~360 other instructions whose costs add up to ~2,300 cycles "
                           "(profiles/r05_gap_cost_probe.txt, DESIGN.md section 3 K1w4) -- and, with two waves per SIMD, socket power (K1w8)"
                           if r["kernel"] in ("tower_wino4_kernel", "conv3x3_wino4_kernel") else None),
            "delivery": deliv,
            "achieved": achieved,
            "peak": peak,
            "unit": "TFLOP/s",
            "frac": achieved / peak,
            "traffic": traffic,
            "traffic_source": source,
            "avg_launch_us": r["launch_us"],
            "avg_launch_note": "per-launch start / stop HIP events (hipExtLaunchKernelGGL) on the launches of the same forward, in a pass of "
                               "its own right behind the timed steps: the stamps cost ~0.5 us per launch, so launches_per_step x avg_launch_us "
                               "can exceed ms_per_step by 1-2 % -- `achieved` and `frac` are low by that much, never high.  tower_wino4_kernel runs every "
                               "layer behind the stem in ONE launch: its duration (+ the stem's) is divided by the 1 + 2 x blocks layers, i.e. "
                               "avg_launch_us is per LAYER and launches_per_step counts layers",
            "launches_per_step": r["launches"],
            "flop_per_launch": flop_per_launch,
            "mfma_terms_per_multiply_add": mfma_terms(dtype, r["kernel"]),
            "mfma_pipe_frac": mfma_terms(dtype, r["kernel"]) * achieved / peak,
            "peak_of": "f16 / bf16 32x32x16 MFMA, dense, at the 2.4 GHz peak clock" if dtype != "f32" else "f32 32x32x2 MFMA, at the 2.4 GHz peak clock",
            "under_load": under_load,
            "sustained": sustained,
        }

    def side_object(dtype, r):
        return {
            "value": world * batch * r["steps"] / r["elapsed"],
            "unit": "node-evals/s",
            "ms_per_step": r["elapsed"] / r["steps"] * 1e3,
            "steps": r["steps"],
            "dtype": dtype,
            "note": DTYPE_NOTE[dtype],
            "roofline": roofline(dtype, r),
        }

    main_r = time_evaluator(args.dtype, args.steps, args.warmup, args.lanes, args.settle_seconds, extras=args.full,
                            keep_outputs=rank == 0 and args.dump_outputs is not None)
    if main_r["outputs"] is not None:
        # the arrays a caller of cattus_hip_eval_device receives (at most 1,024 x 1,880 logits: under 8 MB per workload)
        dump = Path(args.dump_outputs)
        dump.mkdir(parents=True, exist_ok=True)
        np.save(dump / "policy.npy", main_r["outputs"][0].astype(np.float32))
        np.save(dump / "value.npy", main_r["outputs"][1].astype(np.float32))

    # ---- the headline is complete here.  Everything behind it (--full) is a side leg: each runs inside run_leg(), so an exception
    # becomes an {"error": ...} object in the line instead of taking the headline with it, and a watchdog prints the line
    # with what is there if the legs hang (a rank that died inside a collective of a leg leaves the others waiting).
    out = {}
    if rank == 0:
        value = world * batch * args.steps / main_r["elapsed"]
        out = {
            "metric": "MCTS node-evals/sec (chess 20x256 net, batch 256)",
            "value": value,
            "unit": "node-evals/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": main_r["elapsed"] / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "dtype_note": DTYPE_NOTE[args.dtype],
            "data": "synthetic leaf positions + seeded random-init weights",
            "config": {
                "workload": f"{args.workload}: ConvNetV1 {d.blocks}x{d.filters}, board {d.board}, "
                f"{d.planes} planes, {d.moves} moves, batch {batch} leaves/GPU, evaluator-only (planes, logits and values resident in HBM: "
                "no PCIe, no search; the rate with both is `selfplay.node_evals_per_sec` of --full)",
                "per_gpu_batch": batch,
                "flop_per_leaf": d.flops_per_position(),
            },
            "per_gpu_value": value / world,
            # each rank's own rate over its K steps, before the closing barrier (`value` is the job's: K steps of every rank in
            # the slowest rank's time)
            "per_rank_value": [batch * args.steps / t for t in main_r["own_all"]],
            "effective_warmup_steps": args.warmup + main_r["settle_steps"],
            "host": {"cpus_of_this_rank": len(cpu_share), "ranks_on_this_node": local_world},
            "process_group": pg_note,
        }
        if args.full:
            out["roofline"] = roofline(args.dtype, main_r)
        out["whole_step_mfma_frac"] = d.flops_per_position() * batch / (main_r["elapsed"] / args.steps) / 1e12 / MFMA_PEAK_TFLOPS[args.dtype]
        if main_r["settle_ms"] is not None:
            out["settle"] = {"steps": main_r["settle_steps"], "ms_per_step": main_r["settle_ms"], "value": world * batch / (main_r["settle_ms"] * 1e-3),
                             "note": "untimed steps in front of the W warm-up steps (clock governor); their own rate, for comparison with `value`"}
        if main_r["elapsed2"] is not None:
            out["two_batches_in_flight"] = {
                "value": batch * world * args.steps / main_r["elapsed2"],
                "ms_per_step": main_r["elapsed2"] / args.steps * 1e3,
                "note": "same K steps alternating between the evaluator's two lanes on two streams",
            }

    import threading

    emit_lock = threading.Lock()
    emitted = [False]

    def emit():
        """Rank 0 writes THE line, once."""
        with emit_lock:
            if emitted[0] or rank != 0:
                return
            emitted[0] = True
            sys.stdout.flush()
            os.write(json_fd, (json.dumps(out) + "\n").encode())

    def watchdog():
        # the side legs hang (a collective whose peer is gone, a wedged leg): the headline is measured -- print it and leave
        print(f"bench.py: rank {rank}: side legs exceeded --side-legs-timeout {args.side_legs_timeout:.0f} s; "
              "printing the line with what is there", file=sys.stderr, flush=True)
        out["side_legs_error"] = f"watchdog: side legs exceeded {args.side_legs_timeout:.0f} s"
        emit()
        os._exit(0 if rank == 0 else 3)

    timer = threading.Timer(args.side_legs_timeout, watchdog)
    timer.daemon = True
    timer.start()

    def run_leg(name, fn):
        """-> fn()'s result, or None after recording {"error": ...} under `name` (rank 0) when it raised."""
        try:
            return fn()
        except Exception as exc:  # noqa: BLE001 - a side leg must not take the headline with it
            import traceback

            traceback.print_exc()
            out[name] = {"error": f"{type(exc).__name__}: {exc}"}
            return None

    for dtype, skip, div in (("bf16", args.no_bf16, 1), ("f16", args.no_f16, 1), ("f32", args.no_f32, 10)):
        if dtype == args.dtype or skip or not args.full:
            continue
        k = max(5, args.steps // div)

        def side(dtype=dtype, k=k, div=div):
            r = time_evaluator(dtype, k, max(2, args.warmup // div), settle_s=0.2 if dtype in ("bf16", "f16") else 0.0)
            return side_object(dtype, r) if rank == 0 else None

        obj = run_leg(dtype, side)
        if obj is not None:
            out[dtype] = obj

    # ---- reduced-cost towers vs f32 at SEARCH level (rank 0): 800-sim searches of the same positions with each tower
    def agreement_leg():
        from cattus_amd import agreement as ag
        from cattus_amd import selfplay as sp

        games = 16
        t0 = time.perf_counter()
        with HipEvaluator(blob, batch_size=games, plane_words=1, dtype="f32", device=local_rank, flush_us=100) as ev32:
            cfg = sp.make_config(sim_num=800, temperature_policy=[(9999, 0.0)], cache_size=1000000)
            opens = ag.random_openings("chess", games, 2, seed=7)
            ta = ag.run_traces("chess", cfg, sp.Net.hip_batched(ev32), opens, 2, args.agreement_plies)
        lines = [op + [c for c, _ in t] for op, t in zip(opens, ta)]
        agreement = {}
        for dtype in [args.dtype] + ([] if args.no_bf16 or args.dtype == "bf16" else ["bf16"]) + ([] if args.no_f16 or args.dtype == "f16" else ["f16"]):
            # created as the timed evaluator of that dtype is (same max_batch => same tower form, same kernel): the line pairs a kernel's
            # throughput with THAT kernel's search accuracy (the leaf server runs the 16 threads' leaves as partial batches of it)
            with HipEvaluator(blob, batch_size=batch, plane_words=1, dtype=dtype, device=local_rank, flush_us=100) as evx:
                tb = ag.run_traces("chess", cfg, sp.Net.hip_batched(evx), lines, 2, args.agreement_plies)
                kernel = evx.tower_kernel()
            agreement[dtype] = ag.compare_traces(ta, tb)
            agreement[dtype]["tower_kernel"] = kernel
            agreement[dtype]["max_batch"] = batch
        agreement.update(games=games, sims_per_move=800, searched_plies_per_game=args.agreement_plies, seconds=time.perf_counter() - t0,
                         note="f32 plays; each tower searches the same positions (teacher-forced, trees carried over); greedy move choice, noise "
                              "off. tests/test_search_parity_gpu.py runs 16 plies per game and bounds these numbers; larger samples: "
                              "profiles/r03_search_agreement.json")
        return agreement

    if args.full and headline and args.agreement_plies > 0 and rank == 0 and args.dtype != "f32":
        obj = run_leg("search_agreement", agreement_leg)
        if obj is not None:
            out["search_agreement"] = obj

    # ---- end-to-end self-play legs (all ranks; each plays its own shard of the games)
    def selfplay_legs():
        from cattus_amd import selfplay as sp

        threads = search_threads(sp, world)
        # BASELINE config 3 as written: 800 sims/move, batch 256; 1536 concurrent games (two batches in flight and four
        # more in the making); every game is cut after `plies` plies so that the leg fits its time budget (a whole
        # 800-sim game of ~290 plies costs ~170 k evaluations)
        capacity = min(EVAL_CAPACITY[args.dtype], threads * 60e3)  # evaluations/s this rank can expect: GPU-bound or host-bound
        conc = 1536
        plies = int(max(3, min(64, args.selfplay_seconds * capacity / (conc * 0.75 * args.selfplay_sims))))
        leg = selfplay_leg(blob, args.dtype, local_rank, rank, world, games=conc, slots=conc, sims=args.selfplay_sims, max_game_plies=plies,
                           keep_records=False, pool=False, torch=torch, dev=cdev)
        sp_out = reduce_leg(leg, torch, cdev, world)
        sp_out.update(max_game_plies=plies, settings=SELFPLAY_SETTINGS_TEXT, dtype=args.dtype,
                      note="bounded sample: every game is adjudicated after max_game_plies plies; games_per_hour_estimate = plies_per_sec "
                           "* 3600 / (plies per whole game measured in selfplay_full_games) -- an ESTIMATE; measured whole games at 800 sims: "
                           "profiles/r03_e2e_whole_games_800sims.json")
        out["selfplay"] = sp_out
        # whole games, reduced simulation count: a measured games/hour
        full_sims = 64
        full_games = int(min(1024, max(64, 25.0 * capacity / (190.0 * full_sims)))) // 2 * 2
        # batch_size 128: ~300 sequential searches fill ~120 slots per batch (measured: batch_fill), so a 256-leaf evaluator would run
        # half empty all the way -- and in the f16x2 tower's Winograd form, which is built for full batches
        leg = selfplay_leg(blob, args.dtype, local_rank, rank, world, games=full_games, slots=full_games, sims=full_sims, max_game_plies=0,
                           keep_records=False, pool=False, torch=torch, dev=cdev, batch=128)
        sp_full = reduce_leg(leg, torch, cdev, world)
        sp_full.update(games_per_hour=sp_full["games"] * 3600.0 / sp_full["seconds"], settings=SELFPLAY_SETTINGS_TEXT.replace("batch 256", "batch 128"),
                       dtype=args.dtype)
        sp_out["games_per_hour_estimate"] = sp_out["plies_per_sec"] * 3600.0 / max(1.0, sp_full["plies_per_game"])
        out["selfplay_full_games"] = sp_full
        # BASELINE config 4's shape: 64 concurrent games per GPU (sequential search: at most 64 leaves per batch), records
        # kept and pooled over RCCL (gather to rank 0) with the counters all-reduced, all inside the timed region
        pool = dist.is_initialized()
        leg = selfplay_leg(blob, args.dtype, local_rank, rank, world, games=64, slots=64, sims=args.selfplay_sims, max_game_plies=6,
                           keep_records=True, pool=pool, torch=torch, dev=cdev)
        sp_c4 = reduce_leg(leg, torch, cdev, world)
        sp_c4.update(max_game_plies=6, pool_seconds=leg["pool_seconds"], pooled=leg["pooled"], settings=SELFPLAY_SETTINGS_TEXT.replace("batch 256", "batch 64"),
                     dtype=args.dtype,
                     note="64 games per GPU, records gathered on rank 0 and counters all-reduced through torch.distributed 'nccl' (= RCCL) inside "
                          "the timed region; one leaf per tree in flight, so a batch holds at most 64 leaves"
                          + ("" if pool else "; NO process group came up on this box (see process_group): nothing was pooled"))
        out["selfplay_config4"] = sp_c4

    if args.full and headline and args.selfplay_seconds > 0:
        run_leg("selfplay_legs", selfplay_legs)

    if rank == 0 and args.full:
        if headline:
            def pack_leg():
                from cattus_amd import evaluator as ev_mod

                return pack_roofline(torch, ev_mod.load_library(), dev, stream)

            obj = run_leg("roofline_plane_pack", pack_leg)
            if obj is not None:
                out["roofline_plane_pack"] = obj
        if world == 1 and not args.no_cpu_baseline:
            obj = run_leg("cpu_baseline", lambda: cpu_baseline(blob, planes))
            if obj is not None:
                out["cpu_baseline"] = obj
    timer.cancel()
    emit()

    if dist.is_initialized():
        try:
            dist.destroy_process_group()
        except Exception:  # noqa: BLE001 - the line is out; a peer that is gone must not turn the exit status red
            pass


if __name__ == "__main__":
    main()
