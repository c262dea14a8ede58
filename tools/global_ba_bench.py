#!/usr/bin/env python3
"""Measures orbfe_ba_global_optimize (Optimizer::globalOptimization on the device) on trajectory maps of 30 .. 1500 keyframes
(ba_synth.make_trajectory_problem: 20 points per keyframe, 3 loop keyframes, Huber kernels, 5 % outliers, keyframe 0 fixed), optimize(10),
and writes ONE JSON line (and profiles/global_ba_bench.json with --out).
Each size: host -> host time of the C call through the Python binding with solver 2 (block-CSR + PCG; median, p99), the Levenberg
trials and the CG iterations per trial, and one call with ORBFE_GBA_PHASES set for the split into build / Schur / PCG / evaluate and the
number of launches (wall time with the stream synchronised after every phase: the split's sum exceeds the unsynchronised call).
The comparison is the path a caller had before: orbfe_ba_local_optimize(10, 0) on the same problem in the same run (solver 1 is that
call).  It is run while the next size is predicted, by n^3 from the last one, to finish in about ten seconds; past that it is recorded
as not run.  Where both ran, iterations must agree and the estimates are compared.
A second table varies the number of CG iterations enqueued between two reads of the solver's state (ORBFE_PCG_CHUNK) at 250 and 1000
keyframes: the default in csrc/orbfe_gba.hip comes from it.
The expectation this tool tests is in DESIGN 4.25, written before anything was measured.  There is no CPU figure for g2o: g2o is not
available where this runs, and none is invented.
Usage: python tools/global_ba_bench.py [--out profiles/global_ba_bench.json] [--sizes 30,60,...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orb_slam2_ros2_amd import ba_synth  # noqa: E402
from orb_slam2_ros2_amd._lib import Context, GBA_DENSE_MAX_FREE  # noqa: E402

PER_KF, ITERATIONS, DENSE_BUDGET_S = 20, 10, 10.0


def summary(s):
    ms = np.asarray(s) * 1e3
    return {"median": round(float(np.median(ms)), 3), "p99": round(float(np.percentile(ms, 99)), 3), "n": len(ms)}


def timed(f, reps, warmup):
    out = []
    for _ in range(reps + warmup):
        t0 = time.perf_counter()
        f()
        out.append(time.perf_counter() - t0)
    return out[warmup:]


def pose_dist(a, b):
    s = np.sign((a[:, :4] * b[:, :4]).sum(1, keepdims=True))
    return float(max(np.abs(a[:, :4] - s * b[:, :4]).max(), np.abs(a[:, 4:] - b[:, 4:]).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="30,60,120,250,500,1000,1500")
    ap.add_argument("--chunks", default="16,64,256,1024")
    a = ap.parse_args()
    ctx = Context(640, 480, n_features=500, max_images=1)
    res = {"tool": "global_ba_bench", "unit": "ms", "iterations_asked": ITERATIONS, "points_per_keyframe": PER_KF,
           "auto_threshold_in_this_build": GBA_DENSE_MAX_FREE, "g2o_cpu_ms": None,
           "g2o_cpu_note": "not measured: g2o is not available where this tool runs"}
    problems = {}
    last_dense = None                                   # (n, seconds) of the last dense call
    for n in (int(v) for v in a.sizes.split(",")):
        pr = ba_synth.make_trajectory_problem(100 + n, n, PER_KF)
        fixed = np.zeros(n, np.uint8)
        fixed[0] = 1
        problems[n] = (pr, fixed)
        reps, warmup = (10, 2) if n <= 250 else (3, 1)
        sparse = lambda: ctx.ba_global_optimize(pr, fixed, ITERATIONS, solver=2)
        g = sparse()
        trials, cg, rejected = (int(v) for v in g["cg_stats"])
        nnzb = int(ctx.debug_ba_reduced_bsr(pr, fixed, 1.0)["col"].size)
        r = {"keyframes": n, "non_fixed": n - 1, "points": int(pr["points"].shape[0]), "edges": int(pr["edge_pose"].size), "blocks": nnzb,
             "block_fill": round(nnzb / float((n - 1) ** 2), 4), "iterations": g["iters"], "trials": trials, "rejected_by_solver": rejected,
             "cg_iterations": cg, "cg_iterations_per_trial": round(cg / max(trials, 1), 1)}
        r["sparse_host_ms"] = summary(timed(sparse, reps, warmup))
        os.environ["ORBFE_GBA_PHASES"] = "1"
        t0 = time.perf_counter()
        sparse()
        r["sparse_synchronised_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        del os.environ["ORBFE_GBA_PHASES"]
        ph = Context.ba_global_phases()
        r["sparse_split_ms_synchronised"] = dict(zip(("build", "schur", "pcg", "evaluate"), (round(float(v), 3) for v in ph[:4])))
        r["sparse_launches_and_copies"] = int(ph[4])
        r["pcg_share"] = round(float(ph[2] / max(ph[:4].sum(), 1e-9)), 3)
        predicted = None if last_dense is None else last_dense[1] * (n / last_dense[0]) ** 3
        if predicted is not None and predicted > DENSE_BUDGET_S:
            r["dense_host_ms"] = None
            r["dense_note"] = f"not run: predicted {predicted:.0f} s by n^3 from {last_dense[1]:.2f} s at {last_dense[0]} keyframes"
        else:
            dense = lambda: ctx.ba_local_optimize(pr, fixed, ITERATIONS, 0)
            t0 = time.perf_counter()
            d = dense()
            first = time.perf_counter() - t0
            last_dense = (n, first)
            if first > DENSE_BUDGET_S:
                r["dense_host_ms"] = {"median": round(first * 1e3, 3), "p99": round(first * 1e3, 3), "n": 1}
                r["dense_note"] = "one call only: it took longer than the budget"
            else:
                t = timed(dense, reps if first < 1.0 else 2, 1 if first < 1.0 else 0)
                last_dense = (n, float(np.median(t)))
                r["dense_host_ms"] = summary(t)
            assert int(d["iters"][0]) == g["iters"], (n, d["iters"], g["iters"])
            r["sparse_vs_dense_max_abs_diff"] = {"poses": pose_dist(g["poses"], d["poses"]), "points": float(np.abs(g["points"] - d["points"]).max())}
            assert r["sparse_vs_dense_max_abs_diff"]["poses"] < 1e-6 and r["sparse_vs_dense_max_abs_diff"]["points"] < 1e-6
            r["dense_over_sparse"] = round(r["dense_host_ms"]["median"] / r["sparse_host_ms"]["median"], 3)
        res[f"global_ba_{n}"] = r
        print(f"# {n}: {json.dumps(r)}", file=sys.stderr, flush=True)
    sweep = {}
    for n in (250, 1000):
        if n not in problems:
            continue
        pr, fixed = problems[n]
        row = {}
        for chunk in (int(v) for v in a.chunks.split(",")):
            os.environ["ORBFE_PCG_CHUNK"] = str(chunk)
            row[str(chunk)] = summary(timed(lambda: ctx.ba_global_optimize(pr, fixed, ITERATIONS, solver=2), 3, 1))["median"]
        del os.environ["ORBFE_PCG_CHUNK"]
        sweep[str(n)] = row
    res["chunk_sweep_host_ms_median"] = sweep
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
