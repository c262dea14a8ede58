#!/usr/bin/env python3
"""Measures orbfe_create_new_map_points (Context.create_new_map_points) and writes ONE JSON line (and the file given by --out).
Case: one current keyframe + 10 neighbours x 2000 features (tests/tri_scenes.scene).  fused_ms: host to host of one call, median / p99
over --reps after --warmup.  upload_bytes: what the call copies to the device (its arrays, 256-byte aligned).  host_route_ms: in the same
process, today's route -- ten searchForTriangulation calls through the existing matcher (frontend.ORBMatcher, one device brute force
and one synchronisation each), then the numpy restatement's geometry (cosines, branch, triangulation, checkMapPoint), loop 2 and
the tail on the host -- median over --host-reps (Python: not the reference's C++ loop).
Device time per kernel: rocprofv3 --kernel-trace --stats -d DIR -- python tools/tri_bench.py --reps 50 --host-reps 0
Usage: python tools/tri_bench.py [--reps 200] [--host-reps 3] [--out profiles/tri_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tri_scenes as ts  # noqa: E402
import triangulation_restatement as tr  # noqa: E402
from orb_slam2_ros2_amd._lib import Context  # noqa: E402
from orb_slam2_ros2_amd.frontend import ORBMatcher  # noqa: E402


def upload_bytes(cur, nbs):
    """what orbfe_tri.hip copies: the TriKf table (184 bytes each, static_assert there), then every array 256-byte aligned"""
    a = lambda b: (b + 255) // 256 * 256 if b else 256  # noqa: E731
    tot = a(184 * (len(nbs) + 1)) + a(4 * len(ts.SF)) + a(len(cur["kps"])) + a(12 * len(cur["kps"]))
    for k in [cur] + nbs:
        n, (nodes, offs, feats) = len(k["kps"]), k["fv"]
        tot += a(28 * n) + a(32 * n) + a(4 * len(nodes)) + a(4 * len(offs)) + a(4 * len(feats)) + a(n) + 2 * a(8 * n)
    return tot


def host_route(ctx, cur, nbs):
    """today's route: per neighbour one searchForTriangulation through the existing matcher (device brute force, one synchronisation
    each), then the restatement's per-match geometry (cosines, branch, triangulation, checkMapPoint) and loop 2 / the tail on the host"""
    m = ORBMatcher(0.6, False)

    def match(c, nb):
        bow = dict(desc_f=c["desc"], desc_kf=nb["desc"], featvec_f=tr.featvec_dict(c["fv"]), featvec_kf=tr.featvec_dict(nb["fv"]),
                   good_f=(c["flags"] & 1) != 0, inmap_f=(c["flags"] & 2) != 0, good_kf=(nb["flags"] & 1) != 0,
                   inmap_kf=(nb["flags"] & 2) != 0)
        return m.searchForTriangulation(ctx, bow, c["kps"], nb["kps"], c["Tcw"], c["Twc"], nb["Tcw"], nb["Twc"], ts.k_inv(), ts.SF)
    recs, tail, _, _ = tr.create_new_map_points(cur, nbs, ts.CAM, ts.k_inv(), ts.BL, ts.SF, match=match)
    return len(recs), len(tail)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cur, nbs, _ = ts.scene(0, n_nb=10, n=2000)
    ctx = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
    run = lambda: ctx.create_new_map_points(cur, nbs, ts.CAM, ts.k_inv(), ts.BL, ts.SF)  # noqa: E731
    for _ in range(a.warmup):
        recs, tail, _ = run()
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        run()
        t.append((time.perf_counter() - t0) * 1e3)
    h = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        host_route(ctx, cur, nbs)
        h.append((time.perf_counter() - t0) * 1e3)
    out = {"case": "1 + 10 keyframes x 2000 features", "records": int(len(recs)), "tail": int(len(tail)),
           "fused_ms_median": round(float(np.median(t)), 4), "fused_ms_p99": round(float(np.percentile(t, 99)), 4),
           "reps": a.reps, "upload_bytes": upload_bytes(cur, nbs),
           "host_route_ms_median": round(float(np.median(h)), 2) if h else None, "host_reps": a.host_reps,
           "estimate_ms": 0.3}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
