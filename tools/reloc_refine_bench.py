#!/usr/bin/env python3
"""Measures the relocalisation refine of one PnP hypothesis (Context.reloc_refine_stored) against the four-call path it
replaces -- Context.pose_only_optimize, Context.search_in_area_features with the frame's features uploaded, then both again, with the
post-check and the 10 / 50 decisions in numpy in between (tests/reloc_refine_restatement.py run on the device calls) -- in ONE process per
case, Python binding on both sides, and writes ONE JSON line (and --out).
  inliers30    2000 frame features x 2000 keyframe features, about 30 PnP inliers: search, second optimisation (ACCEPT_2)
  inliers100   the same with about 100 PnP inliers: accepted after the first optimisation (ACCEPT_1)
Per case: the two routes' verdicts and final assignments are compared first; then median / p99 of --reps runs of each, alternating (host
to host); the bare C call of the one call; device milliseconds between events, the MATCH and BA stages of each route (separate
repetitions); the bytes each route uploads.
Every case runs in a child process of its own under a time limit, and a case is started only if the one before it succeeded.
Usage: python tools/reloc_refine_bench.py [--reps 200] [--out profiles/reloc_refine_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"inliers30": dict(n_seed=30), "inliers100": dict(n_seed=100)}
LIMIT_S = 240


def stats(t):
    return {"median": round(float(np.median(t)), 4), "p99": round(float(np.percentile(t, 99)), 4)}


def alternate(f, g, reps, warmup):
    """reps runs of f and of g, one after the other in turn, so that both see the same box at the same moment"""
    for _ in range(warmup):
        f(), g()
    tf, tg = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t1 = time.perf_counter()
        g()
        t2 = time.perf_counter()
        tf.append((t1 - t0) * 1e3), tg.append((t2 - t1) * 1e3)
    return tf, tg


class DeviceCalls:
    """the two array-level calls of the four-call path behind the oracle's signatures, counting what they upload"""

    def __init__(self, ctx):
        self.ctx, self.up, self.calls = ctx, 0, 0

    def pose_only_optimize(self, Xw, meas, info, sigma2, pose, fx, fy, cx, cy, bf):
        self.up += len(Xw) * (24 + 24 + 8 + 4) + 56
        self.calls += 1
        return self.ctx.pose_only_optimize(Xw, meas, info, sigma2, pose, fx, fy, cx, cy, bf)

    def search_in_area_ex(self, kps, desc, bounds, qxy, radius, lo, hi, q_desc, exclude):
        self.up += len(kps) * (kps.itemsize + 32 + 1) + len(qxy) * (8 + 4 + 1 + 1 + 32)
        self.calls += 1
        return self.ctx.search_in_area_features(kps, desc, qxy, radius, lo, hi, q_desc, exclude, bounds=bounds, want_hits=True)


def case(name, reps, warmup):
    import reloc_refine_restatement as rr
    import reloc_refine_scenes as sc
    from oracle.pyoracle import Oracle
    from orb_slam2_ros2_amd import synth
    from orb_slam2_ros2_amd._lib import Context, KeyframeStore
    orc = Oracle()
    n_seed = CASES[name]["n_seed"]
    n = len(sc.frame(orc, 3)["lk"])
    s = sc.build(orc, image_seed=3, n_seed=n_seed, n_near=1300, n_dup=60, n_fill=n - n_seed - 3 - 1300 - 60, seed_noise=0.01, mode="up")
    ctx = Context(sc.W, sc.H, n_features=sc.NF, max_images=2)
    (kps, desc), _ = ctx.extract_batch(list(synth.stereo_pair(3)))
    assert np.array_equal(kps, s["kps"]) and np.array_equal(desc, s["desc"])
    st = KeyframeStore(sc.W, sc.H)
    st.add(sc.KF_ID, s["kf_kps"], s["kf_desc"], bounds=sc.BOUNDS)
    dev = DeviceCalls(ctx)

    def one():
        return ctx.reloc_refine_stored(0, st, sc.KF_ID, s["good"], s["pos"], s["kf_Rcw"], s["kf_tcw"], s["held"], s["Rcw"], s["tcw"], s["cam"],
                                       s["bounds"], s["sigma2"], s["inv_sigma2"], s["baseline"], right_u=s["right_u"])

    four = lambda: rr.refine(dev, s)  # noqa: E731
    a, b = four(), one()
    up_four, calls_four = dev.up, dev.calls
    assert a["verdict"] == b["verdict"] and np.array_equal(a["final_assigned"], b["final_assigned"]), "the one call and the four calls disagree"
    t_four, t_one = alternate(four, one, reps, warmup)
    bare = lambda: ctx.lib.orbfe_reloc_refine_stored(*ctx._reloc_args)  # noqa: E731
    t_bare, _ = alternate(bare, lambda: None, reps, warmup)
    # device time between events (separate repetitions), one stage at a time in the production schedule
    device = {"one_call": {}, "four_calls": {}}
    for stage, key in ((6, "match"), (7, "ba")):
        ctx.profile_enable(2 + stage)
        ctx.profile_read(reset=True)
        for _ in range(reps):
            bare()
        device["one_call"][key] = round(ctx.profile_read(reset=True)[key][0] / reps, 4)
        for _ in range(reps):
            four()
        device["four_calls"][key] = round(ctx.profile_read(reset=True)[key][0] / reps, 4)
        ctx.profile_enable(0)
    N, NF, nl = len(s["good"]), sc.NF, 8
    res = {"case": f"{s['n_kp']} frame features x {N} keyframe features, {int(b['n_edges'][0])} PnP inliers", "equal": True,
           "verdict": b["verdict_name"], "n_inliers": [int(v) for v in b["n_inliers"]], "n_added": [int(v) for v in b["n_added"]], "reps": reps,
           "four_calls_ms": stats(t_four), "one_call_ms": stats(t_one), "one_call_bare_c_ms": stats(t_bare), "device_ms": device,
           "bytes_up": {"one_call": N * (1 + 12) + NF * (4 + 8) + 2 * nl * 4, "four_calls": up_four}, "device_calls": {"one_call": 1, "four_calls": calls_four},
           "one_call_not_slower": bool(np.median(t_one) <= np.median(t_four))}
    st.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="(internal) run one case in this process and print its JSON")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(case(a.case, a.reps, a.warmup)))
        return
    out = {}
    for name in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                           capture_output=True, text=True, timeout=LIMIT_S)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.exit(f"case {name} failed with status {r.returncode}; nothing further was started\n" + (r.stdout + r.stderr)[-2000:])
        out[name] = json.loads(line[0][len("RESULT "):])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
