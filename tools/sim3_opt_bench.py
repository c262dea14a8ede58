#!/usr/bin/env python3
"""Measures orbfe_sim3_optimize (Optimizer::OptimizeSim3 on the device) at n = 60, 200 and 600 pairs, and orbfe_pose_only_optimize at
2 n edges in the same run as the yardstick, and writes ONE JSON line (and profiles/sim3_opt_bench.json with --out).
Each case: host -> host time of the C call through the Python binding (median, p99) over --reps calls after --warmup, then a second
series with the context's stage events on for the device time between the events around the launch.  Before timing, every Sim3 result
is compared with the restatement (tests/sim3_opt_restatement.py: flags equal, estimate within 1e-6).
The estimate this tool tests (made before anything was measured): a 200-pair problem costs what orbfe_pose_only_optimize costs at a
similar edge count times a small factor for the 13 evaluations of a linearisation, i.e. a few hundred microseconds host to host;
`estimate` in the output says whether that held (ratio <= 5 and under 1000 us at n = 200).  There is no CPU figure for g2o: g2o is not
available where this runs, and none is invented.
Usage: python tools/sim3_opt_bench.py [--reps 300] [--out profiles/sim3_opt_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sim3_opt_restatement as R  # noqa: E402
from orb_slam2_ros2_amd import ba_synth  # noqa: E402
from orb_slam2_ros2_amd._lib import Context  # noqa: E402

KEYS = ("pc", "pm", "uv_c", "uv_m", "info_c", "info_m", "cam", "model")


def summary(us):
    us = np.asarray(us) * 1e6
    return {"median": round(float(np.median(us)), 1), "p99": round(float(np.percentile(us, 99)), 1), "n": len(us)}


def timed(ctx, call, reps, warmup):
    host = []
    for i in range(reps + warmup):
        t0 = time.perf_counter()
        call()
        host.append(time.perf_counter() - t0)
    ctx.profile_enable(2 + 7)           # the "ba" stage only, in the production schedule
    ctx.profile_read(True)
    dev = []
    for i in range(reps + warmup):
        call()
        ms, k = ctx.profile_read(True)["ba"]
        dev.append(ms * 1e-3 / max(k, 1))
    ctx.profile_enable(False)
    return {"host_us": summary(host[warmup:]), "device_us_between_events": summary(dev[warmup:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = Context(640, 480, n_features=500, max_images=1)
    res = {"tool": "sim3_opt_bench", "checked_against_restatement": True, "g2o_cpu_us": None,
           "g2o_cpu_note": "not measured: g2o is not available where this tool runs"}
    for n in (60, 200, 600):
        p = ba_synth.make_sim3_problem(11, n, n // 10, 0.5)
        args = tuple(p[k] for k in KEYS)
        want = R.optimize_sim3(*args)
        got = ctx.sim3_optimize(*args)
        assert got[0] == want["n_inliers"] and np.array_equal(got[2], want["flags"].astype(bool))
        assert np.abs(got[3] - want["est"]).max() < 1e-6
        r = timed(ctx, lambda: ctx.sim3_optimize(*args), a.reps, a.warmup)
        r.update(pairs=n, iterations=want["iterations"], trials=want["trials"], inliers=want["n_inliers"])
        q = ba_synth.make_pose_problem(seed=7, n=2 * n)
        pa = (q["Xw"], q["meas"], q["info"], q["sigma2"], q["pose"], q["fx"], q["fy"], q["cx"], q["cy"], q["bf"])
        y = timed(ctx, lambda: ctx.pose_only_optimize(*pa), a.reps, a.warmup)
        y["edges"] = 2 * n
        r["pose_only_yardstick"] = y
        r["host_ratio_to_yardstick"] = round(r["host_us"]["median"] / y["host_us"]["median"], 2)
        res[f"sim3_opt_{n}"] = r
    ctx.close()
    r200 = res["sim3_opt_200"]
    held = r200["host_ratio_to_yardstick"] <= 5 and r200["host_us"]["median"] < 1000
    res["estimate"] = {"what": "200 pairs: a small factor (<= 5) over orbfe_pose_only_optimize at 400 edges and a few hundred us (< 1000) host to host",
                       "held": bool(held)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
