#!/usr/bin/env python3
"""bench.py -- stereo frames/sec (extract+match) on KITTI-00-shaped 1241x376 pairs, MI355X.

One "step" = one pass of the hot path (pyramid+blur, FAST, quadtree, orientation+rBRIEF for the left and
right image, then searchByStereo) over one batch of `--pairs` synthetic stereo pairs that are already
resident in HBM when the timed region starts.  Contract: `python bench.py --gpus N --steps K --warmup W`
prints ONE JSON line on rank 0 (see the task statement).  N>1: launched by torch.distributed.run, one
rank per GPU, frames sharded per rank (weak scaling), one RCCL gather of the per-pair results at the end
of the sequence inside the timed region.

`--sequence F` runs BASELINE config 4 instead: a sequence of F stereo pairs cut into contiguous blocks per rank (sharding.frame_range),
each rank streaming its block from page-locked host memory through orbfe_stream_submit in batches of <= --pairs, and ONE gather of
the per-frame records (left keypoints + descriptors + right_u + depth, 152 KB per frame) to rank 0 over RCCL, inside the timed region.

A plain run does only what the headline figure needs: set-up, warm-up, the K timed steps, the outputs of the last step when
`--dump-outputs DIR` is given, and the line (metric, value, unit, higher_is_better, dtype, ms_per_step and the step loop's
configuration).  It leaves GPU_MAX_HW_QUEUES as the caller set it; `--full` and `--sequence` raise it to 16 for the streaming legs.  Everything else -- the checks of the last batch against the committed digests, the per-stage profile and the
rooflines, the extra legs and the CPU baseline -- runs with `--full` only.

`--dump-outputs DIR` writes what the last timed step computed, as a caller of orbfe_stereo_batch_device receives it, to DIR/<name>.npy
(float32 / float64; rank 0's shard): the keypoint counts and match counts of every pair, and keypoints, descriptors, right_u and depth of
a fixed, seeded sample of pairs (at most 64 MB in all).  The inputs depend on the arguments only, so two builds can be compared file by file.

Extra objects in the JSON line (`--full`):
  host_io       the same step fed from page-locked HOST memory and delivering its results to host memory (orbfe_stream_submit:
                upload of batch k+1 and download of batch k-1 under the compute of batch k) -- the PCIe-inclusive rate; `value`
                itself is device-resident
  roofline      dominant kernel: algorithmic bytes per launch / mean launch duration (HIP events on the
                library's stream) against the 8 TB/s HBM peak
  cpu_baseline  the CPU oracle (oracle/, -O3 -march=native, 2 threads exactly like Frame.cc:100-105)
                timed on this box's host cores over a bounded sample of the same frames (rank 0, N=1 only)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from benchlib.common import (BF, FX, H, HBM_PEAK_GBPS, NFEAT, NLEVELS, PCIE_PEAK_GBPS, SCALE, TH_HI, TH_LO, W, _StdoutToStderr,  # noqa: E402
                             algorithmic_bytes, spawn_ranks)
from benchlib.host_io import host_io_leg  # noqa: E402
from benchlib.legs import ba_leg, cfg3_leg, latency_leg  # noqa: E402
from benchlib.sequence_leg import run_sequence_mode, sequence_batch, sequence_job  # noqa: E402
from benchlib.sweep import content_sweep  # noqa: E402


DUMP_SEED, DUMP_SAMPLE_PAIRS = 20251015, 32


def dump_outputs(ctx, counts, n_matches, out_dir):
    """The last step's results as a caller of orbfe_stereo_batch_device receives them (slots 2p / 2p + 1 = left / right image of pair p),
    as DIR/<name>.npy in float32 / float64: the keypoint counts [pairs][2] and match counts of every pair; keypoints [x y size angle
    response octave class_id], descriptors (one value per byte), right_u and depth of a fixed, seeded sample of pairs (entries past a
    slot's count are zero).  About 21 MB at 2000 features."""
    os.makedirs(out_dir, exist_ok=True)
    n_pairs = len(n_matches)
    pairs = np.sort(np.random.default_rng(DUMP_SEED).choice(n_pairs, min(n_pairs, DUMP_SAMPLE_PAIRS), replace=False))
    nf = ctx.n_features
    kps = np.zeros((len(pairs), 2, nf, 7), np.float32)
    desc = np.zeros((len(pairs), 2, nf, 32), np.float32)
    ru = np.zeros((len(pairs), nf), np.float64)
    dp = np.zeros((len(pairs), nf), np.float64)
    for i, p in enumerate(pairs):
        k, d, c = ctx.fetch_batch(2 * int(p), 2)
        for e in range(2):
            n = int(c[e])
            kps[i, e, :n] = np.stack([k[e, :n][f].astype(np.float32) for f in k.dtype.names], axis=-1)
            desc[i, e, :n] = d[e, :n]
        r, z, _ = ctx.fetch_stereo_batch(int(p), 1)
        ru[i, :int(c[0])] = r[0, :int(c[0])]
        dp[i, :int(c[0])] = z[0, :int(c[0])]
    out = {"counts": np.asarray(counts, np.float64).reshape(n_pairs, 2), "n_matches": np.asarray(n_matches, np.float64),
           "sample_pairs": pairs.astype(np.float64), "keypoints": kps, "descriptors": desc, "right_u": ru, "depth": dp}
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prewarm-seconds", type=float, default=3.0,
                    help="untimed steps run before the W warm-up steps until this much wall time has passed: the GPU needs "
                         "~0.3 s of sustained load to leave its idle clocks (measured: first 30 steps 13 %% slower)")
    ap.add_argument("--pairs", type=int, default=512, help="stereo pairs per step (per GPU)")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="budget of the cpu_baseline leg (0 = skip)")
    ap.add_argument("--host-io-steps", type=int, default=-1, help="steps of the host_io leg (-1: min(--steps, 200), 0: skip)")
    ap.add_argument("--sequence", type=int, default=0,
                    help="run a whole sequence of this many stereo pairs (BASELINE config 4: 4541), sharded over the ranks, instead of the "
                         "fixed-batch step loop")
    ap.add_argument("--sequence-unique", type=int, default=512, help="distinct synthetic frames behind the sequence (frame f = f mod this)")
    ap.add_argument("--unique", type=int, default=0,
                    help="distinct stereo pairs in the step's batch (0 = --pairs: every pair of a step is a different synthetic frame, as the "
                         "reference reads a new image pair every iteration, example/Stereo/KittiStereo.cc:28-33; 16 = the tiling of rounds 1-5, "
                         "whose 15 MB of level-0 pixels stay in the Infinity Cache)")
    ap.add_argument("--sequence-leg", type=int, default=4541,
                    help="frames of the sequence job reported beside the step loop (`sequence` object: BASELINE config 4 -- 4541 stereo pairs cut "
                         "into blocks over the ranks, the per-frame records brought to one host memory); 0 skips it")
    ap.add_argument("--sequence-exchange", choices=["shared", "gather"], default="shared",
                    help="how the per-frame records of a sequence job reach one place: 'shared' = every rank drains its windows into one "
                         "page-locked POSIX shared-memory segment over its own PCIe link, the collective carries 16 B per frame; 'gather' = "
                         "the records are gathered on rank 0 over the collective and drained over rank 0's link")
    ap.add_argument("--sequence-window", type=int, default=1, help="batches per gather window of the sequence job (sharding.WindowGather)")
    ap.add_argument("--only-leg", default="", help="(internal) run ONE extra leg (cfg3 | ba | latency) in this process and print its JSON object: "
                    "--full runs the latency leg this way, in a child started WITHOUT GPU_MAX_HW_QUEUES -- the streaming legs of the "
                    "parent want 16 hardware queues, a caller that processes one frame at a time has the runtime's default, ~50 us per frame "
                    "faster (ADVICE r4)")
    ap.add_argument("--content-steps", type=int, default=40,
                    help="timed steps per content class of the content sweep (config.content_sweep: rect / camera / saturated / sparse, every "
                         "pair verified against the golden digests); 0 skips it")
    ap.add_argument("--legs", default="cfg3,ba,latency", help="comma-separated extra legs of the default line (north_star beyond the stereo step): "
                    "cfg3 (2000x2000 Hamming), ba (config-5 edge evaluation / normal equations / local BA / pose-only), latency (one pair, host "
                    "to host, in the reference's call shape); '' skips them")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the checks of the last batch against the golden digests, the "
                         "per-stage profile and rooflines, host_io, the sequence job, the content sweep, the CPU baseline and the --legs")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write the last step's outputs (rank 0's shard) to DIR/<name>.npy in float32 / float64")
    args = ap.parse_args()
    if (args.full or args.sequence > 0) and not args.only_leg:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # before the first HIP call: one hardware queue per stream of the streaming legs
                                                            # (= orbfe_recommended_hw_queues(); the library only warns, it cannot set it).  The
                                                            # one-frame latency leg runs in a child WITHOUT it (--only-leg): what a drop-in user has
    if args.dump_outputs and args.sequence > 0:
        raise SystemExit("bench.py: --dump-outputs writes the step loop's outputs; it is not available with --sequence")

    if args.only_leg:
        dev_id = int(os.environ.get("LOCAL_RANK", "0"))
        leg = {"cfg3": cfg3_leg, "ba": ba_leg, "latency": latency_leg}[args.only_leg](dev_id)
        print(json.dumps(leg))
        return

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` outside a launcher: start N ranks (one per GPU) as CHILD processes -- before anything in this process
        # has touched the GPU -- relay rank 0's JSON line and exit with the worst child status
        raise SystemExit(spawn_ranks(args.gpus))

    # The synthetic frames of this rank, generated ONCE, outside every clock, by a child process (tools/gen_frames.py: forked workers):
    # rank r owns frames [r U, (r + 1) U) of every step (weak scaling), U = --unique distinct pairs (default: all --pairs of a step);
    # the sequence legs read frames f mod --sequence-unique, which on rank 0 are the same arrays.
    from benchlib.common import generate_pairs_child, golden_digests
    rank_env = int(os.environ.get("RANK", "0"))
    n_unique = min(args.pairs, args.unique if args.unique > 0 else args.pairs)
    U_seq = max(1, min(args.sequence_unique, 4541))
    t_gen = time.perf_counter()
    step_frames = list(range(rank_env * n_unique, (rank_env + 1) * n_unique)) if args.sequence <= 0 else []
    seq_frames = list(range(U_seq)) if (args.sequence > 0 or (args.full and args.sequence_leg > 0)) else []
    wanted = sorted(set(step_frames) | set(seq_frames))
    frame_cache = generate_pairs_child(wanted)   # (a child process forks the workers: this one may already carry a profiler's library)
    t_gen = time.perf_counter() - t_gen

    # The one-frame latency leg runs NOW, in a child process, while nothing else holds a context on the GPU (the r5
    # record's p99 of 0.8 - 1.0 ms were this leg's C++ harness running beside the idle contexts of this process and of the leg's own
    # Python half).  The child is started WITHOUT GPU_MAX_HW_QUEUES: the setting a one-frame-at-a-time caller has (recorded in the leg).
    latency_result = None
    if args.full and args.sequence <= 0 and args.gpus == 1 and rank_env == 0 and "latency" in [x for x in args.legs.split(",") if x]:
        import subprocess
        env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
        env["LOCAL_RANK"] = os.environ.get("LOCAL_RANK", "0")
        t_lat = time.perf_counter()
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-leg", "latency"], env=env, capture_output=True, text=True, timeout=1200)
        try:
            latency_result = json.loads(r.stdout.strip().split("\n")[-1])
            latency_result["leg_seconds"] = round(time.perf_counter() - t_lat, 1)
        except Exception:   # noqa: BLE001
            raise SystemExit("bench.py: latency leg (child process) failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])

    import torch
    import torch.distributed as dist

    # ONE JSON line on stdout is the contract, and native libraries write there too (RCCL's version banner when its first communicator
    # comes up): from here on file descriptor 1 points at stderr, and the line goes to the saved descriptor at the very end
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    def emit(line):
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(line) + "\n").encode())

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s) (WORLD_SIZE)")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (the front end has no CPU fallback)")
    # test hooks (a 1-GPU box cannot run RCCL with two ranks): ORBFE_BENCH_ONE_DEVICE=1 puts every rank on cuda:0 and
    # ORBFE_BENCH_BACKEND=gloo exchanges through host memory -- same control flow, used only to rehearse the N > 1 path
    backend = os.environ.get("ORBFE_BENCH_BACKEND", "nccl")
    if os.environ.get("ORBFE_BENCH_ONE_DEVICE") == "1":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    xdev = dev if backend == "nccl" else torch.device("cpu")  # where the tensors of the collectives live
    # The process group is initialised with ONE rank too (backend nccl = RCCL): the sequence-level gather then really goes through
    # RCCL on every box this runs on, and torch's bundled RCCL is known to live with liborbfe_hip.so in one process before an 8-GPU
    # node ever sees the pair.  A failure to initialise with one rank is reported in the line (`rccl`), not fatal.
    collective, rccl_note = world > 1, None
    if world > 1:
        with _StdoutToStderr():
            if backend == "nccl":
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
                probe = torch.ones(4, device=dev)
                dist.all_reduce(probe)   # the communicator (and its banner) comes up here, not inside a timed region
                torch.cuda.synchronize()
            else:
                dist.init_process_group(backend, rank=rank, world_size=world)
    elif backend == "nccl" and os.environ.get("ORBFE_BENCH_NO_PG") != "1":
        try:
            import socket
            if "MASTER_PORT" not in os.environ:
                sk = socket.socket()
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
                sk.close()
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            with _StdoutToStderr():
                dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
                probe = torch.ones(4, device=dev)
                dist.all_reduce(probe)
                torch.cuda.synchronize()
            collective, rccl_note = True, "process group of 1 rank over RCCL: the gathers of this run executed as RCCL collectives"
        except Exception as ex:   # noqa: BLE001 -- reported, the single-rank path needs no collective
            rccl_note = f"init_process_group('nccl', world_size=1) failed: {type(ex).__name__}: {ex}"
            collective = False

    from orb_slam2_ros2_amd import synth
    from orb_slam2_ros2_amd._lib import Context

    if args.sequence > 0:
        line = run_sequence_mode(args, rank, local_rank, world, dev, xdev, backend, collective, frame_cache)
        if rank == 0:
            line["rccl"] = rccl_note
            emit(line)
        if dist.is_initialized():
            dist.destroy_process_group()
        return

    B = args.pairs
    # the batch: n_unique distinct pairs (default B: all different), tiled to B when fewer
    lefts = [frame_cache[f][0] for f in step_frames]
    rights = [frame_cache[f][1] for f in step_frames]
    reps = (B + n_unique - 1) // n_unique
    left_h = np.stack((lefts * reps)[:B])
    right_h = np.stack((rights * reps)[:B])
    d_left = torch.from_numpy(left_h).to(dev)
    d_right = torch.from_numpy(right_h).to(dev)

    ctx = Context(W, H, NFEAT, NLEVELS, SCALE, TH_HI, TH_LO, device_id=local_rank, max_images=2 * B)

    def step():
        ctx.stereo_batch_device(d_left.data_ptr(), d_right.data_ptr(), W, W * H, B, FX, BF)

    class _Raw:  # zero-copy torch view of one of the library's device buffers
        def __init__(self, p, n):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (p, False), "version": 2}

    res = ctx.device_results()
    d_counts = torch.as_tensor(_Raw(res["counts"], 2 * B), device=dev)
    d_nmatch = torch.as_tensor(_Raw(res["n_match"], B), device=dev)

    def gather_results():
        """Sequence-level exchange: the per-pair records of this rank's shard -> rank 0, one RCCL gather
        over xGMI at the end of the sequence.  Frames are independent, so nothing else crosses GPUs."""
        summary = torch.empty(B, 4, dtype=torch.int32, device=dev)
        summary[:, 0] = d_counts[0::2]
        summary[:, 1] = d_counts[1::2]
        summary[:, 2] = d_nmatch
        summary[:, 3] = rank
        if not collective:
            return [summary]
        summary = summary.to(xdev)
        out = [torch.empty_like(summary) for _ in range(world)] if rank == 0 else None
        dist.gather(summary, out, dst=0)
        return out

    def sync_all():
        ctx.sync()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(3):
        step()
    ctx.sync()

    if args.full:
        n_cand_img = sum(len(ctx.debug_candidates(0, l)) for l in range(NLEVELS))  # FAST candidates of one image (slot 0)
        per_image_bytes, match_bytes, pair_bytes = algorithmic_bytes(ctx, n_cand_img)

        # per-stage device time (HIP events on the library stream), every kernel timed ALONE, in an untimed pass: this picks the
        # dominant stage and fills `all_stages`
        ctx.profile_enable(1)
        for _ in range(max(3, min(args.steps, 10))):
            step()
        ctx.sync()
        prof = ctx.profile_read()
        ctx.profile_enable(0)
        stages = {k: (ms / n if n else 0.0) for k, (ms, n) in prof.items() if n}
        images_per_launch = 2 * B
        stage_bytes = {k: per_image_bytes[k] * images_per_launch for k in per_image_bytes}
        stage_bytes["stereo"] = match_bytes * B
        dom = max((k for k in stages if k in stage_bytes), key=lambda k: stages[k])
        stage_id = {"resize": 0, "blur": 1, "fast": 2, "quadtree": 3, "orient_brief": 4, "stereo": 5}[dom]

    # warm-up of the exchange: the first torch indexing / RCCL call initialises lazily (tens of ms).  BEFORE the sustained load below, not
    # between it and the clock: the chip's clocks sag within milliseconds of idling, and a 20-step run (0.1 s) is over before they are back
    gather_results()
    ctx.sync()
    # sustained load right in front of the clock (the stage pass above runs every kernel alone between synchronisations: the chip falls
    # back towards its idle clocks there, and the first ~30 steps after that are up to 13 % slower -- a 20-step run would time exactly those)
    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < args.prewarm_seconds:
        for _ in range(4):
            step()
        ctx.sync()
    for _ in range(args.warmup):
        step()
    sync_all()
    # the timed region runs the production schedule (blur under the quadtree, stereo match of a batch under the front of the next);
    # with --full the dominant stage alone carries HIP events on the stream it is launched on, so its duration is measured LIVE in this
    # region -- the figure the rocprofv3 kernel trace of this command shows for the same kernels
    if args.full:
        ctx.profile_enable(2 + stage_id)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    ctx.sync()
    t_steps = time.perf_counter() - t0
    gathered = gather_results()
    sync_all()
    dt = time.perf_counter() - t0
    if args.full:
        live = ctx.profile_read()
        ctx.profile_enable(0)
    if world > 1:
        tmax = torch.tensor([dt], dtype=torch.float64, device=xdev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())

    if args.dump_outputs and rank == 0:
        dump_outputs(ctx, d_counts.cpu().numpy(), d_nmatch.cpu().numpy(), args.dump_outputs)

    total_pairs = args.steps * B * world
    fps = total_pairs / dt
    line = {
        "metric": "stereo frames/sec (extract+match) KITTI-00 1241x376; HBM GB/s vs roofline",
        "value": fps,
        "unit": "stereo pairs/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic",
    }
    if not args.full:
        line["config"] = {
            "workload": f"Single 1241x376 KITTI-shaped stereo pair, 8-level pyramid, 2000 FAST+rBRIEF keypoints per image, searchByStereo; "
                        f"batched ({B} pairs per step, {n_unique} of them distinct synthetic frames).  `value` is DEVICE-RESIDENT; the checks, "
                        "rooflines, host_io, sequence job, content sweep, CPU baseline and extra legs run with --full",
            "io": "device-resident",
            "pairs_per_step_per_gpu": B,
            "distinct_pairs_per_step": n_unique,
            "steps_only_ms_per_step": t_steps / args.steps * 1e3, "exchange_and_barrier_ms": (dt - t_steps) * 1e3,
            "n_features": NFEAT,
            "levels": NLEVELS,
            "frame_generation_seconds": round(t_gen, 2),
        }
        line["rccl"] = rccl_note
        ctx.close()
        if rank == 0:
            emit(line)
        if dist.is_initialized():
            dist.destroy_process_group()
        return

    # sanity: the last batch produced features and matches, and the gathered summaries agree with the fetched results
    nm, ru, dp, _, _ = ctx.fetch_stereo(0)
    kps, _ = ctx.fetch_features(0)
    assert len(kps) > 0 and nm > 0, "front end produced no features/matches"
    if rank == 0:
        g0 = gathered[0].cpu().numpy()
        assert g0[0, 0] == len(kps) and g0[0, 2] == nm, "gathered summary disagrees with the fetched results"
        assert all(int(g[:, 2].min()) > 0 for g in (t.cpu().numpy() for t in gathered)), "a rank produced a pair without matches"

    # every pair of the last timed batch against the committed digests (tests/golden/golden_v5.json: sha256 of keypoints, descriptors,
    # right_u, depth and match count per frame, made by the oracle): no oracle needed here, a fraction of a second, outside the clock
    from orb_slam2_ros2_amd.digest import batch_digests
    gold, hexn = golden_digests(step_frames)   # tests/golden/golden_v5.json: the oracle's digest of every frame of the 4541-pair sequence
    kps_all, desc_all, cnt_all = ctx.fetch_batch(0, 2 * B)
    ru_all, dp_all, nm_all = ctx.fetch_stereo_batch(0, B)
    digests = [d[:hexn] for d in batch_digests(kps_all, desc_all, cnt_all, ru_all, dp_all, nm_all)]
    want = [gold[p % n_unique] for p in range(B)]
    wrong = [p for p in range(B) if want[p] is not None and digests[p] != want[p]]
    if wrong:
        raise SystemExit(f"bench.py: rank {rank}: {len(wrong)} of {B} pairs differ from the golden digests (first: pair {wrong[0]})")
    verified = sum(w is not None for w in want)
    if world > 1:
        v = torch.tensor([verified], dtype=torch.int64, device=xdev)
        dist.all_reduce(v)
        verified = int(v.item())
    del kps_all, desc_all, ru_all, dp_all

    host_io = None
    hio_steps = min(args.steps, 200) if args.host_io_steps < 0 else args.host_io_steps
    if hio_steps > 0:
        host_io = host_io_leg(ctx, left_h, right_h, B, hio_steps, want, world, sync_all, dist, torch, xdev)

    seq_leg = None
    if args.sequence_leg > 0:
        F_leg = args.sequence_leg   # the whole job, cut into blocks over the ranks (BASELINE config 4: 4541)
        U_leg = U_seq
        B_leg = sequence_batch((F_leg + world - 1) // world, B)
        t_seq, _, n_chk, xinfo = sequence_job(ctx, F_leg, B_leg, U_leg, rank, world, dev, xdev, backend, collective, window=max(1, args.sequence_window),
                                              exchange=args.sequence_exchange, frame_cache=frame_cache)
        # ... and the same job with the OTHER exchange beside it: north_star names the RCCL-over-xGMI gather of the
        # records; the default drains every rank's records over its own PCIe link.  Both in every line, so that the first multi-GPU run
        # reports the two side by side.
        other = "gather" if args.sequence_exchange == "shared" else "shared"
        t_oth, _, n_chk_o, xinfo_o = sequence_job(ctx, F_leg, B_leg, U_leg, rank, world, dev, xdev, backend, collective, window=max(1, args.sequence_window),
                                                 exchange=other, frame_cache=frame_cache)
        if rank == 0 and xinfo.get("records_sha256") != xinfo_o.get("records_sha256"):
            raise SystemExit(f"bench.py: sequence: the record stores of the two exchanges differ ({args.sequence_exchange}: {xinfo.get('records_sha256')}, "
                             f"{other}: {xinfo_o.get('records_sha256')})")
        seq_other = {"frames": F_leg, "pairs_per_s": F_leg / t_oth, "seconds": t_oth, "exchange": xinfo_o, "records_checked_against_host_path": n_chk_o,
                     "collective_executed": bool(collective)}
        seq_leg = {"frames": F_leg, "pairs_per_s": F_leg / t_seq, "seconds": t_seq, "result_bytes": F_leg * ctx.record_bytes(), "exchange": xinfo,
                   "other_exchange": seq_other,
                   "pairs_per_batch": B_leg, "batches_per_window": max(1, args.sequence_window), "collective_executed": bool(collective),
                   "records_checked_against_host_path": n_chk, "records_checked_for_repeat_consistency": max(0, F_leg - min(U_leg, F_leg)),
                   "what": "BASELINE config 4: contiguous blocks of frames per rank, page-locked host images -> extraction + stereo match "
                           "-> per-frame records packed on the device -> (exchange.payload) under the next window's compute, collective = " +
                           (("RCCL" if collective else "none: single rank, no process group") if backend == "nccl" else backend) +
                           ", all inside the timed region; `python bench.py --sequence 4541` runs the same job as the whole line"}

    sweep = None
    if rank == 0 and world == 1 and args.content_steps > 0:
        sweep = content_sweep(ctx, B, dev, (left_h, right_h), args.content_steps, want)

    live_ms, live_n = live[dom]
    stages_inline = dict(stages)
    if live_n:
        stages[dom] = live_ms / live_n
    dom_ms = stages[dom]
    achieved = stage_bytes[dom] / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0

    line.update({
        "verified_pairs": verified,   # pairs of the last timed batch (all ranks) whose results equal the committed golden digests
        "host_io": host_io,
        "sequence": seq_leg,
        "config": {
            "workload": "Single 1241x376 KITTI-shaped stereo pair, 8-level pyramid, 2000 FAST+rBRIEF keypoints per image, "
                        f"searchByStereo; batched ({B} pairs per step, {n_unique} of them distinct synthetic frames).  `value` is DEVICE-RESIDENT: the images are in HBM when the clock starts "
                        "and the results stay there; the rate of SURVEY 8(d)'s protocol -- page-locked host images in, full results back in host "
                        "memory, PCIe both ways inside the clock -- is config.host_io_pairs_per_s, the whole-sequence job (BASELINE config 4, "
                        "host images in, per-frame records out) config.sequence_pairs_per_s",
            "io": "device-resident",   # images are in HBM when the clock starts, results stay there (see host_io for the PCIe-inclusive rate)
            "host_io_pairs_per_s": host_io["pairs_per_s"] if host_io else None,
            "h2d_GBps": host_io["h2d_GBps"] if host_io else None,
            "d2h_GBps": host_io["d2h_GBps"] if host_io else None,
            "pcie_frac": (host_io["h2d_GBps"] / PCIE_PEAK_GBPS) if host_io else None,   # upload direction, per GPU, of 63 GB/s (PCIe 5.0 x16)
            "sequence_pairs_per_s": seq_leg["pairs_per_s"] if seq_leg else None,
            "content_sweep": sweep,
            "pairs_per_step_per_gpu": B,
            # the end-of-sequence exchange (summary gather + barrier) is INSIDE the clock: its share of a K-step run, so that a short run
            # (the driver's 20 steps) and a long one (the default 300) can be compared
            "steps_only_ms_per_step": t_steps / args.steps * 1e3, "exchange_and_barrier_ms": (dt - t_steps) * 1e3,
            "n_features": NFEAT,
            "levels": NLEVELS,
            "parallelism": f"frames sharded over {world} GPU(s), RCCL gather of per-pair results at sequence end",
            "algorithmic_bytes_per_pair": pair_bytes,          # 20 012 776 for this shape (no quadtree term)
            "quadtree_record_bytes_per_pair": 2 * per_image_bytes["quadtree"],   # candidate records read + selections written (prices the stage only)
            "pipeline_hbm_GBps": pair_bytes * fps / world / 1e9,
            "pipeline_hbm_frac": pair_bytes * fps / world / 1e9 / HBM_PEAK_GBPS,
            "stage_ms_per_launch": {k: round(v, 4) for k, v in stages_inline.items()},
        },
        "roofline": {
            "kernel": dom,
            "bound": "hbm",
            "achieved": achieved,
            "peak": HBM_PEAK_GBPS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBPS,
            "traffic": None,
            "algorithmic_bytes_per_launch": stage_bytes[dom],
            "avg_launch_ms": dom_ms,
            "images_per_launch": images_per_launch,
            # k_fast runs once per pyramid level (per-level LDS carve-up): the "launch" priced here is the level sweep of one
            # batch, i.e. NLEVELS k_fast launches, the small levels on a second stream BESIDE the large ones.  Their rocprofv3
            # durations therefore overlap: the matching trace figure is the union of the launches' intervals per step (column
            # UnionNs / steps of profiles/*_kernel_stats.csv, tools/kernel_stats_from_db.py), not average x NLEVELS
            "kernel_launches_per_step": {"fast": NLEVELS, "orient_brief": 4, "resize": 1, "blur": 1, "quadtree": 1, "stereo": 3}[dom],
            "avg_launch_ms_alone": stages_inline[dom],
            "rocprof_match": ("union of the k_fast launches of a step (UnionNs / steps in the newest profiles/r*_kernel_stats.csv); LIVE figure of the "
                              "production schedule: the level-0 blur runs beside FAST on the second stream (avg_launch_ms_alone: nothing beside it)")
                             if dom == "fast" else "sum of the stage's kernels per step in the newest profiles/r*_kernel_stats.csv",
            "all_stages": {k: {"ms": round(stages_inline[k], 4), "GBps": round(stage_bytes[k] / (stages_inline[k] * 1e-3) / 1e9, 1)}
                           for k in stages_inline if k in stage_bytes and stages_inline[k] > 0},
        },
    })

    # The dominant kernel and the whole step against the VALU ISSUE ceiling (committed rocprofv3 SQ_* pass), and the dominant kernel's
    # memory-side traffic (committed FETCH_SIZE / WRITE_SIZE passes): benchlib/profile_reader.py
    from benchlib.profile_reader import add_traffic, add_valu_roofline
    add_valu_roofline(line, dom, dom_ms, dt / args.steps, B)
    add_traffic(line, dom, stage_bytes, B, images_per_launch)

    # What DESIGN.md / README.md claim, as SCALAR keys of `config` (the driver's record keeps the scalars of `config`
    # and drops nested objects -- config.content_sweep, config.stage_ms_per_launch and the roofline_valu object never reached BENCH_r05.json)
    cfgd = line["config"]
    cfgd["distinct_pairs_per_step"] = n_unique
    cfgd["frame_generation_seconds"] = round(t_gen, 2)
    for k, v in stages_inline.items():
        cfgd[f"stage_{k}_ms"] = round(v, 4)            # the stage's kernels ALONE (HIP events, untimed pass)
    cfgd[f"stage_{dom}_live_ms"] = round(dom_ms, 4)     # the dominant stage inside the timed region (= roofline.avg_launch_ms)
    if sweep:
        for cls in ("rect", "camera", "saturated", "sparse"):
            if cls in sweep:
                cfgd[f"content_{cls}_pairs_per_s"] = round(sweep[cls]["pairs_per_s"], 1)
        cfgd["content_worst_over_best"] = round(sweep["worst_over_best"], 4)
    rv = line.get("roofline_valu")
    if rv:
        cfgd["valu_pipeline_frac"] = round(rv.get("pipeline_frac", 0.0), 4)
        cfgd["valu_pipeline_frac_at_measured_clock"] = round(rv.get("pipeline_frac_at_measured_clock", 0.0), 4)
        cfgd[f"{dom}_valu_frac"] = round(rv["frac"], 4)
        if "issue_classes" in rv:
            cfgd[f"{dom}_valu_frac_class_weighted"] = round(rv["issue_classes"]["frac_class_weighted"], 4)
    if line["roofline"].get("traffic"):
        cfgd[f"{dom}_traffic_over_algorithmic"] = round(line["roofline"]["traffic_over_algorithmic"], 3)

    if rank == 0 and world == 1 and args.cpu_seconds > 0:
        from oracle import pyoracle
        so = pyoracle.build(fast=True, out_dir=os.path.join("/tmp", f"orb_oracle_{os.getuid()}"))
        orc = pyoracle.Oracle(so)
        orc.stereo_frame(lefts[0], rights[0], want_outputs=False)  # warm-up
        n_done, t_cpu0 = 0, time.perf_counter()
        while True:
            i = n_done % n_unique
            m = orc.stereo_frame(lefts[i], rights[i], NFEAT, NLEVELS, SCALE, TH_HI, TH_LO, FX, BF, math_mode=0, threads=2,
                                 want_outputs=False)
            assert m >= 0
            n_done += 1
            if time.perf_counter() - t_cpu0 >= args.cpu_seconds or n_done >= 400:
                break
        t_cpu = time.perf_counter() - t_cpu0
        line["cpu_baseline"] = {
            "value": n_done / t_cpu,
            "unit": "stereo pairs/s",
            "cores": 2,
            "kind": "port",
            "caveat": "a scalar C++ restatement of the reference's algorithm (oracle/): no OpenCV SIMD paths (resize / blur / FAST), so the real "
                      "reference would be faster on the same cores and gpu_over_cpu overstates the gap; the >= 30x target holds under any "
                      "reasonable correction, the kernel-quality figure is roofline / roofline_valu, not this ratio",
            "sample": f"{n_done} synthetic 1241x376 stereo pairs, oracle/orb_oracle.cpp -O3 -march=native, L/R extract on 2 threads "
                      f"(Frame.cc:100-105), pairs sequential; host has {os.cpu_count()} cores",
        }
        line["config"]["gpu_over_cpu"] = fps / (n_done / t_cpu)
        # (ii) of SURVEY 8d, the throughput-fair figure: pairs distributed over the host cores of this box's share (one pair per
        # thread, L/R extraction sequential inside it), same oracle, same inputs; reported beside the reference-shaped one
        from concurrent.futures import ThreadPoolExecutor
        n_thr = max(1, min(len(os.sched_getaffinity(0)), 16))
        t_all0 = time.perf_counter()
        t_end = t_all0 + max(2.0, args.cpu_seconds / 2)

        def _worker(w):
            n = 0
            while time.perf_counter() < t_end:
                i = (w + n) % n_unique
                assert orc.stereo_frame(lefts[i], rights[i], NFEAT, NLEVELS, SCALE, TH_HI, TH_LO, FX, BF, math_mode=0, threads=1,
                                        want_outputs=False) >= 0
                n += 1
            return n

        with ThreadPoolExecutor(n_thr) as pool:
            n_all = sum(pool.map(_worker, range(n_thr)))
        t_all = time.perf_counter() - t_all0
        line["cpu_baseline"]["all_cores"] = {"value": n_all / t_all, "unit": "stereo pairs/s", "cores": n_thr,
                                             "sample": f"{n_all} pairs over {n_thr} threads, one pair per thread"}
        line["config"]["gpu_over_cpu_all_cores"] = fps / (n_all / t_all)
    line["rccl"] = rccl_note
    ctx.close()
    if rank == 0 and world == 1:
        legs = [x for x in args.legs.split(",") if x]
        t_legs = time.perf_counter()
        if "cfg3" in legs:
            line["cfg3"] = cfg3_leg(local_rank)
        if "ba" in legs:
            line["ba"] = ba_leg(local_rank)
        if "latency" in legs and latency_result is not None:
            line["latency"] = latency_result   # (measured at the very start of this run, before this process touched the GPU: see above)
        line["legs_seconds"] = time.perf_counter() - t_legs
    if rank == 0:
        emit(line)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
