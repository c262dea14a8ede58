#!/usr/bin/env python3
"""Measures the EPnP RANSAC sets (orbfe_pnp, _lib.PnPSet) and writes ONE JSON line (and profiles/pnp_bench.json with --out).
Each case times Tracking::trackReLocalize's step-3 loop host to host (every iterate call from Python, n = 5 per call, round-robin over
the candidates that are not exhausted), median / p90 over --reps fresh sets after --warmup; set creation (one upload) is reported apart.
  fail_20x200      20 candidates x 200 points of pure outliers: every budget (100 hypotheses) spent -- a failing relocalisation
  success_round1   20 x 200 with candidate 0 at 10 % outliers: its first call succeeds (a refine passes, the loop stops)
  fail_30x1000     30 candidates x 1000 points of pure outliers
launches / hypotheses are the set's own counters (orbfe_pnp_stats) for one run of the case.
Usage: python tools/pnp_bench.py [--reps 50] [--out profiles/pnp_bench.json]
Device time per kernel: rocprofv3 --kernel-trace --stats -d DIR -- python tools/pnp_bench.py --reps 20"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pnp_restatement as P  # noqa: E402  (scene generator and the loop shape)
from orb_slam2_ros2_amd._lib import PnPSet, pnp_engine  # noqa: E402


def make(seed, K, N, outliers):
    rng = np.random.default_rng(seed)
    xs, us, os_ = [], [], []
    for k in range(K):
        x, u, o, _, _ = P.scene(rng, N, outlier=outliers[k])
        xs.append(x)
        us.append(u)
        os_.append(o)
    off = np.arange(K + 1, dtype=np.int64) * N
    return off, np.concatenate(xs), np.concatenate(us), np.concatenate(os_)


def run_case(K, N, outliers, reps, warmup):
    data = [make(100 + r, K, N, outliers) for r in range(reps + warmup)]
    loop, create, stats = [], [], None
    for r, (off, xyz, uv, oc) in enumerate(data):
        pnp_engine(1)
        t0 = time.perf_counter()
        s = PnPSet(off, xyz, uv, oc, P.SIGMA2, P.CAM)
        t1 = time.perf_counter()

        def it(p, n):
            d = s.iterate(p, n)
            return d[0], d[1], d[2], d[4]
        log = P.tracking_loop(it, K, 5, lambda p, pose, inl: len(set(inl)) * 2 >= N)
        t2 = time.perf_counter()
        if r >= warmup:
            create.append(t1 - t0)
            loop.append(t2 - t1)
            stats = (*s.stats(), len(log))
        s.close()
    us = np.array(loop) * 1e6
    return {"candidates": K, "points": N, "loop_us": {"median": round(float(np.median(us)), 1), "p90": round(float(np.percentile(us, 90)), 1),
                                                      "n": len(us)},
            "create_us_median": round(float(np.median(create)) * 1e6, 1), "launch_sequences": stats[0], "hypotheses": stats[1],
            "iterate_calls": stats[2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"tool": "pnp_bench",
           "fail_20x200": run_case(20, 200, [1.0] * 20, a.reps, a.warmup),
           "success_round1": run_case(20, 200, [0.1] + [1.0] * 19, a.reps, a.warmup),
           "fail_30x1000": run_case(30, 1000, [1.0] * 30, a.reps, a.warmup)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
