#!/usr/bin/env python3
"""Measures orbfe_pose_graph_optimize (Optimizer::optimizeEssentialGraph on the device) on loop-closure graphs of 100, 500 and 1000
keyframes with about 4 edges per vertex (tests/essential_graph_cases.py: chain, covisibility to the 2nd, 3rd and 4th neighbour, a
corrected group, loop edges), optimize(20) as the reference calls it, and writes ONE JSON line (and profiles/essential_graph_bench.json
with --out).
Each size: host -> host time of the C call through the Python binding (median, p99), a second series with the context's stage events on
for the device time between the events around the loop, and one call with ORBFE_PG_PHASES set for the split into build / assemble /
solve / evaluate (wall time with the stream synchronised after every phase: the split's sum exceeds the unsynchronised call).  Before
timing, every result is checked: chi2 must have fallen by more than 1e6 (the graphs are consistent, the minimum is 0); the 100-keyframe
result is compared with the restatement (tests/essential_graph_restatement.py) within 1e-6.
The estimate this tool tests is in DESIGN 4.24, written before anything was measured.  There is no CPU figure for g2o: g2o is not
available where this runs, and none is invented.
Usage: python tools/essential_graph_bench.py [--out profiles/essential_graph_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import essential_graph_cases as K  # noqa: E402
import essential_graph_restatement as R  # noqa: E402
from orb_slam2_ros2_amd._lib import Context  # noqa: E402


def summary(s):
    ms = np.asarray(s) * 1e3
    return {"median": round(float(np.median(ms)), 3), "p99": round(float(np.percentile(ms, 99)), 3), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="100,500,1000")
    a = ap.parse_args()
    ctx = Context(640, 480, n_features=500, max_images=1)
    res = {"tool": "essential_graph_bench", "unit": "ms", "iterations_asked": 20, "g2o_cpu_ms": None,
           "g2o_cpu_note": "not measured: g2o is not available where this tool runs"}
    for n in (int(v) for v in a.sizes.split(",")):
        reps, warmup = (30, 3) if n <= 100 else ((10, 2) if n <= 500 else (5, 1))
        g = K.make_graph(n - 1, hops=(2, 3, 4))
        args = K.args(g)
        chi0 = float(R.edge_chi2(R.errors(R.Graph(*args), g["estimates"])).sum())
        est, chi2, stats = ctx.pose_graph_optimize(*args)
        assert chi2.sum() * 1e6 < chi0, (n, chi0, chi2.sum())
        r = {"keyframes": n, "non_fixed": n - 1, "edges": int(len(g["edges"])), "iterations": stats[0], "trials": stats[1],
             "chi2_initial": chi0, "chi2_final": float(chi2.sum())}
        if n <= 100:
            want = R.optimize(*args, iterations=6)
            got = ctx.pose_graph_optimize(*args, iterations=6)
            r["max_abs_diff_to_restatement_6_iterations"] = float(np.abs(got[0] - want["est"]).max())
            assert r["max_abs_diff_to_restatement_6_iterations"] < 1e-6 and got[2] == (want["iterations"], want["trials"])
        host = []
        for i in range(reps + warmup):
            t0 = time.perf_counter()
            ctx.pose_graph_optimize(*args)
            host.append(time.perf_counter() - t0)
        r["host_ms"] = summary(host[warmup:])
        ctx.profile_enable(2 + 7)           # the "ba" stage only
        ctx.profile_read(True)
        dev = []
        for i in range(reps + warmup):
            ctx.pose_graph_optimize(*args)
            ms, k = ctx.profile_read(True)["ba"]
            dev.append(ms * 1e-3 / max(k, 1))
        ctx.profile_enable(False)
        r["device_ms_between_events"] = summary(dev[warmup:])
        os.environ["ORBFE_PG_PHASES"] = "1"
        t0 = time.perf_counter()
        ctx.pose_graph_optimize(*args)
        r["synchronised_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        del os.environ["ORBFE_PG_PHASES"]
        ph = ctx.debug_pose_graph_phases()
        r["split_ms_synchronised"] = dict(zip(("build", "assemble", "solve", "evaluate"), (round(v, 3) for v in ph)))
        r["solve_share"] = round(ph[2] / max(sum(ph), 1e-9), 3)
        res[f"essential_graph_{n}"] = r
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
