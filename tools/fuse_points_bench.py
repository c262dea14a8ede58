#!/usr/bin/env python3
"""Measures the forward fuse over stored keyframes (Context.fuse_points_into_keyframes_stored) against the chain of calls
it replaces -- per keyframe Context.project_map_points, the radius / window in numpy, Context.search_in_area_features with the
keyframe's features uploaded -- in ONE process per shape, Python binding on both sides, and writes ONE JSON line (and --out).
  loop   30 keyframes x 5000 loop points x 2000 features (LoopClosing::correctLoop, th 4, ratio 0.8)
  single  1 keyframe  x 3000 points      x 2000 features (the forward fuse of LocalMapping::fuseMapPoints, th 3, ratio 0.6)
Per shape: the two routes' tables are compared first; then median / p99 of --reps runs of each, alternating (host to host); the bare C
call of the one call; device milliseconds between events -- the one call's two kernels apart, the chain's MATCH stage as a whole
(separate repetitions); the bytes each route copies up and down; the share of pairs that survive the projection.
Every shape runs in a child process of its own under a time limit, and a shape is started only if the one before it succeeded.
Usage: python tools/fuse_points_bench.py [--reps 200] [--out profiles/fuse_points_bench.json]"""
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

SHAPES = {"loop": dict(K=30, m=5000, n=2000, th=4.0, ratio=0.8), "single": dict(K=1, m=3000, n=2000, th=3.0, ratio=0.6)}
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


def case(name, reps, warmup):
    import fuse_points_scenes as sc
    from orb_slam2_ros2_amd._lib import Context, KeyframeStore
    P = SHAPES[name]
    K, m, th, ratio = P["K"], P["m"], P["th"], P["ratio"]
    S = sc.seeded(40, K=K, m=m, n=P["n"], n_pts=9000)
    kfs, pts, sf = S["kfs"], S["pts"], np.asarray(S["sf"], np.float32)
    assert all(len(kf["kps"]) == P["n"] for kf in kfs)
    ctx = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
    st = KeyframeStore(sc.W, sc.H, 8)
    ids = list(range(1, K + 1))
    for i, kf in zip(ids, kfs):
        st.add(i, kf["kps"], kf["desc"], bounds=kf["bounds"])
    poses = sc.poses(kfs)
    usable = pts["usable"].astype(bool)
    traffic = {"up": 0, "down": 0, "survivors": 0}

    def chain(count=False):
        bi_all, bd_all = np.full((K, m), -1, np.int32), np.zeros((K, m), np.int32)
        for k, kf in enumerate(kfs):
            pr = ctx.project_map_points(pts["pos"], pts["view_dir"], pts["max_dist"], pts["min_dist"], kf["Rcw"], kf["tcw"], sc.CAM, kf["bounds"])
            rows = np.flatnonzero(usable & pr["visible"].astype(bool))
            lvl = pr["level"][rows].astype(np.int32)
            base = np.where(pr["cos_theta"][rows] > np.float32(0.998), np.float32(2.5), np.float32(4.0))
            radius = ((base * np.float32(th)).astype(np.float32) * (sf[lvl] * sf[lvl])).astype(np.float32)
            lo, hi = np.maximum(0, lvl - 1).astype(np.int8), np.minimum(7, lvl + 1).astype(np.int8)
            if count:
                traffic["up"] += m * 32 + len(kf["kps"]) * (kf["kps"].itemsize + 32) + len(rows) * (8 + 4 + 1 + 1 + 32)
                traffic["down"] += m * (8 + 4 + 4 + 1 + 1) + len(rows) * 16
                traffic["survivors"] += len(rows)
            if not len(rows):
                continue
            bi, bd, sd, nc = ctx.search_in_area_features(kf["kps"], kf["desc"], pr["uv"][rows], radius, lo, hi, pts["desc"][rows], None, bounds=kf["bounds"])[:4]
            ok = (nc > 0) & (bd < 50) & (bd.astype(np.float32) / sd.astype(np.float32) < np.float32(ratio))
            bi_all[k, rows[ok]], bd_all[k, rows[ok]] = bi[ok], bd[ok]
        return bi_all, bd_all

    out = (np.zeros((K, m), np.int32), np.zeros((K, m), np.int32))
    one = lambda: ctx.fuse_points_into_keyframes_stored(st, ids, poses, pts, sc.CAM, sf, th, ratio, 50, out=out)  # noqa: E731
    a, b = chain(count=True), one()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "the one call and the chain disagree"
    matches = int((b[0] >= 0).sum())
    t_chain, t_one = alternate(chain, one, reps, warmup)
    bare = lambda: ctx.lib.orbfe_fuse_points_into_keyframes_stored(*ctx._fuse_points_args)  # noqa: E731
    t_bare, _ = alternate(bare, lambda: None, reps, warmup)
    # device time between events (separate repetitions): the MATCH stage alone, in the production schedule
    ctx.profile_enable(2 + 6)
    ctx.profile_read(reset=True)
    k_proj, k_search = [], []
    for _ in range(reps):
        bare()
        p, s = ctx.fuse_points_kernel_ms()
        k_proj.append(p), k_search.append(s)
    one_stage = ctx.profile_read(reset=True)["match"][0] / reps
    for _ in range(reps):
        chain()
    chain_stage = ctx.profile_read(reset=True)["match"][0] / reps
    ctx.profile_enable(0)
    up_one = 4 + K * 120 + len(sf) * 4 + m * (1 + 12 + 12 + 4 + 4 + 32)
    res = {"case": f"{K} keyframes x {m} points x {P['n']} features, th {th}, ratio {ratio}", "equal": True, "matches": matches, "reps": reps,
           "survivor_share": round(traffic["survivors"] / (K * m), 4),
           "chain_ms": stats(t_chain), "one_call_ms": stats(t_one), "one_call_bare_c_ms": stats(t_bare),
           "device_ms": {"one_call": {"k_fusepts_project": round(float(np.median(k_proj)), 4), "k_fusepts_search": round(float(np.median(k_search)), 4),
                                      "match_stage": round(one_stage, 4)},
                         "chain": {"match_stage": round(chain_stage, 4)}},
           "bytes": {"one_call": {"up": up_one, "down": K * m * 8}, "chain": {"up": traffic["up"], "down": traffic["down"]}},
           "one_call_not_slower": bool(np.median(t_one) <= np.median(t_chain))}
    st.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="(internal) run one shape in this process and print its JSON")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(case(a.case, a.reps, a.warmup)))
        return
    out = {}
    for name in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                           capture_output=True, text=True, timeout=LIMIT_S)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.exit(f"shape {name} failed with status {r.returncode}; nothing further was started\n" + (r.stdout + r.stderr)[-2000:])
        out[name] = json.loads(line[0][len("RESULT "):])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
