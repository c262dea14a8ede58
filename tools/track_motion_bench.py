#!/usr/bin/env python3
"""Measures Tracking::trackMotionModel as one call over two frame slots (Context.track_motion_model_slots) against what it
replaces -- the unProject, the direction and the packing of the query arrays on the host (vectorised numpy standing for the drop-in's
per-feature loop), Context.track_motion_model (the array call), and the post-check and the isInMap count on the host -- in ONE process,
Python binding on both sides, and writes ONE JSON line (and --out).  Two frames of tests/track_motion_scenes.py: the full one (2000 x 2000
features, every last-frame feature a query) and the second-search one, where the array call synchronises twice.
The two routes' assignments, inlier flags, poses and verdicts are compared first; then median / p99 of --reps runs of each, alternating
(host to host); the bare C call of the one call; device milliseconds between events, the MATCH and BA stages of each route (separate
repetitions); the bytes each route uploads; the synchronising downloads of each route (the array call makes one per search it runs, its
`passes` output; the one call makes one by construction and reports the searches it ran).
Asserted: the one call uploads fewer bytes, and on the second-search frame it ran two searches behind its one download.
The case runs in a child process of its own under a time limit.
Usage: python tools/track_motion_bench.py [--reps 200] [--out profiles/track_motion_bench.json]"""
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

LIMIT_S = 400


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


def frame(ctx, store, orc, s, kw, reps, warmup):
    """one frame on both routes -> its part of the result"""
    import reloc_refine_restatement as rr
    import track_motion_restatement as tm
    NF, nl = s["nf"], 8
    p = dict(tm.DEFAULTS, **kw)
    n = len(s["store_ids"])
    if n:
        store.upsert(s["store_ids"], pos=s["store_pos"], view_dir=np.zeros((n, 3), np.float32), max_dist=np.ones(n, np.float32),
                     min_dist=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8))
    pose, last_pose = (s["Rcw"], s["tcw"]), (s["last_Rcw"], s["last_tcw"], s["last_Rwc"], s["last_twc"])
    args = (0, s["pair"], 2, s["last_pair"], s["last_flags"], pose, last_pose, s["cam"], s["bounds"], s["baseline"], s["sigma2"], s["inv_sigma2"])
    form = dict(store=store, last_ids=s["last_ids"], **kw)
    up = {}

    def one():
        return ctx.track_motion_model_slots(*args, **form)

    def old():
        temp, tpos = tm.unproject(s)
        q = tm.queries(s, temp, tpos)
        ai = tm.array_call_inputs(s, q)
        r = ctx.track_motion_model(0, ai["qxy"], ai["q_octave"], ai["q_min_level"], ai["q_max_level"], ai["desc"], ai["pos"], s["cam"], s["bounds"],
                                   rr.tcw_to_se3(s["Rcw"], s["tcw"]), s["sigma2"], s["inv_sigma2"], right_u=s["right_u"], th=p["th"],
                                   th_second=p["th_second"], min_matches=p["min_matches"])
        nq = len(q["who"])
        up["old"] = nq * 55 + NF * 8 + 2 * nl * 4 + 56 + r["passes"] * (nq * 4 + NF * 5)
        a = np.where(r["assigned"] >= 0, q["who"][np.maximum(r["assigned"], 0)], -1).astype(np.int32)
        if r["n_edges"] < 0:
            return dict(verdict=tm.REJECT_MATCHES, assigned=a, final_assigned=a, passes=r["passes"], n_matches=r["n_matches"])
        e_in = np.flatnonzero(r["inlier"])
        c = tm.post_check(s, q, a, e_in, np.ones(len(e_in), bool), r["pose"])
        n_map = tm.count_in_map(s, c["cur"])
        return dict(verdict=tm.ACCEPT if n_map >= p["min_inliers"] else tm.REJECT_INLIERS, assigned=a, final_assigned=c["cur"], inlier=c["inlier"],
                    pose_se3=r["pose"], passes=r["passes"], n_matches=r["n_matches"], n_in_map=n_map)

    a, b = old(), one()
    assert a["verdict"] == b["verdict"] and a["passes"] == b["passes"] and a["n_matches"] == b["n_matches"]
    assert np.array_equal(a["assigned"], b["assigned"]) and np.array_equal(a["final_assigned"], b["final_assigned"])
    if b["verdict"] != tm.REJECT_MATCHES:
        assert np.array_equal(a["inlier"], b["inlier"]) and np.array_equal(a["pose_se3"].view(np.uint64), b["pose_se3"].view(np.uint64))
        assert a["n_in_map"] == b["n_in_map"]
    t_old, t_one = alternate(old, one, reps, warmup)
    c_args, c_keep = ctx.track_motion_slots_call(*args, **form)
    bare = lambda: ctx.lib.orbfe_track_motion_model_slots(*c_args)  # noqa: E731
    t_bare, _ = alternate(bare, lambda: None, reps, warmup)
    device = {"one_call": {}, "array_call": {}}
    for stage, key in ((6, "match"), (7, "ba")):
        ctx.profile_enable(2 + stage)
        ctx.profile_read(reset=True)
        for _ in range(reps):
            bare()
        device["one_call"][key] = round(ctx.profile_read(reset=True)[key][0] / reps, 4)
        for _ in range(reps):
            old()
        device["array_call"][key] = round(ctx.profile_read(reset=True)[key][0] / reps, 4)
        ctx.profile_enable(0)
    bytes_up = {"one_call": NF * 9 + 2 * nl * 4, "array_call": int(up["old"])}
    assert bytes_up["one_call"] < bytes_up["array_call"], bytes_up
    return {"queries": len(tm.queries(s, b["temp"], b["temp_pos"])["who"]), "n_matches": b["n_matches"], "n_edges": b["n_edges"], "n_in_map": b["n_in_map"], "verdict": b["verdict_name"], "searches": b["passes"],
            "equal": True, "array_path_ms": stats(t_old), "one_call_ms": stats(t_one), "one_call_bare_c_ms": stats(t_bare), "device_ms": device,
            "bytes_up": bytes_up, "synchronising_downloads": {"one_call": 1, "array_call": int(a["passes"])},
            "one_call_faster": bool(np.median(t_one) < np.median(t_old))}


def case(reps, warmup):
    import track_motion_scenes as sc
    from oracle.pyoracle import Oracle
    from orb_slam2_ros2_amd._lib import Context, MapPointStore
    orc = Oracle()
    g = sc.GEOM["kitti"]
    ctx = Context(g["W"], g["H"], n_features=g["NF"], max_images=4)
    store = MapPointStore()
    for pair, ref, slot in zip(sc.images("kitti"), sc.frames(orc, "kitti"), (2, 0)):
        (lk, ld), _, _, _, _ = ctx.frame_stereo(pair[0], pair[1], g["cam"][0], g["cam"][4], slot_left=slot)
        assert np.array_equal(lk, ref["lk"]) and np.array_equal(ld, ref["ld"])
    n_l = len(sc.frames(orc, "kitti")[0]["lk"])
    full = sc.build(orc, in_map=np.arange(n_l))
    second, kw = sc.second_search(orc)
    res = {"case": f"{g['NF']} x {g['NF']} features", "reps": reps, "full_frame": frame(ctx, store, orc, full, {}, reps, warmup),
           "second_search_frame": frame(ctx, store, orc, second, kw, reps, warmup)}
    assert res["second_search_frame"]["searches"] == 2 and res["second_search_frame"]["synchronising_downloads"] == {"one_call": 1, "array_call": 2}
    store.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", action="store_true", help="(internal) run the case in this process and print its JSON")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(case(a.reps, a.warmup)))
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", "--reps", str(a.reps), "--warmup", str(a.warmup)],
                       capture_output=True, text=True, timeout=LIMIT_S)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.exit(f"the case failed with status {r.returncode}\n" + (r.stdout + r.stderr)[-2000:])
    line = line[0][len("RESULT "):]
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
