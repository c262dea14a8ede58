#!/usr/bin/env python3
"""Measures searchBySim3 over stored keyframes (Context.search_by_sim3_stored / search_by_sim3_points_stored) against the
path it replaces in ONE process on one box, and writes ONE JSON line (and the file given by --out).
  workload      pair: two stored keyframes x 2000 features, about 1500 good points each, 100 input matches, th 7.5, ratio 0.75
                (tests/sim3_search_scenes.seeded); points: 4000 loop-group points into one of them, th 10.
  equal         the two paths' results are compared first, element for element.
  replaced      the two (pair) / one (points) Context.search_in_area_features calls of ORBMatcher.searchBySim3Frames / searchBySim3MapPoints:
                the whole target keyframe uploaded and its grid rebuilt per call.  The projection of every point, the window sizes and the
                exclusion flags are computed BEFORE the clock starts, and the acceptance test and the merge after it stops: the figure is
                the bare device searches and FLATTERS the old path, whose callers run a scalar host loop per point on top of it.  The
                stored call has everything inside its clock.
  *_ms          median / p99 of --reps runs of each, alternating, host clock around the synchronous Python calls; stored_bare_c_call_ms:
                the C call of the pair alone, without the binding's argument conversion.
  device_ms     between HIP events around the launches (the MATCH stage timer, separate repetitions), per call of the path.
  upload_bytes  what each path copies host -> device per call of the path, counted from the arrays handed over, every array padded to
                256 bytes as the scratch layout pads it.
No threshold: the numbers are reported as measured.
Usage: python tools/sim3_search_bench.py [--reps 100] [--out profiles/sim3_search_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sim3_search_scenes as sc  # noqa: E402
from orb_slam2_ros2_amd._lib import Context, KeyframeStore  # noqa: E402
from orb_slam2_ros2_amd.matcher_ext import _affine, _matvec, sim3_project  # noqa: E402

F32 = np.float32
C_ID, M_ID = 1, 2


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


def device_ms(ctx, call, reps):
    ctx.profile_enable(2 + 6)                                  # the MATCH stage only, in the production schedule
    ctx.profile_read(reset=True)
    for _ in range(reps):
        call()
    ms, launches = ctx.profile_read(reset=True)["match"]
    ctx.profile_enable(0)
    return ms / reps, launches / reps


def pad(nbytes):
    return (max(int(nbytes), 8) + 255) // 256 * 256


def area_query(T, rows, uv, octave, desc, th, exclude):
    """the arguments of one search_in_area_features call and the bytes it uploads"""
    sf2 = np.asarray(sc.SF, F32) ** 2
    q = dict(t_kps=T["kps"], t_desc=T["desc"], qxy=np.asarray(uv, F32).reshape(-1, 2), radius=(F32(th) * sf2[octave]).astype(F32),
             min_level=(octave - 1).astype(np.int8), max_level=(octave + 1).astype(np.int8), q_desc=np.ascontiguousarray(desc), exclude=exclude)
    n, k = len(T["kps"]), len(rows)
    up = pad(T["kps"].nbytes) + pad(32 * n) + pad(8 * k) + pad(4 * k) + 2 * pad(k) + pad(32 * k) + (pad(n) if exclude is not None else 0)
    return q, up


def accept(res, ratio):
    bi, bd, sd, nc = res
    with np.errstate(all="ignore"):
        keep = (nc > 0) & (bd <= 50) & (bd.astype(F32) / sd.astype(F32) <= F32(ratio))
    return np.where(keep, bi, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--loop-points", type=int, default=4000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, ratio = a.features, 0.75
    S = sc.seeded(11, 1.1, n=n, n_pts=n * 13 // 10, bounds_c=sc.IMAGE, bounds_m=sc.IMAGE, m_loop=a.loop_points, n_matches=100)
    C, M, loop = S["C"], S["M"], S["loop"]
    ctx = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
    st = KeyframeStore(sc.W, sc.H, 8)
    sc.add_to_store(st, C, C_ID), sc.add_to_store(st, M, M_ID)
    log_sf = F32(np.log(sc.SF[1]))
    s, R, t = S["Scm"]

    # ---- the pair ----
    def stored_pair():
        return ctx.search_by_sim3_stored(st, sc.side(C, C_ID), sc.side(M, M_ID), (R, t), s, S["matches"], sc.CAM, sc.SF, 7.5, ratio, 50)

    s_inv = F32(F32(1) / s)
    Smc = (s_inv, R.T.copy(), (-s_inv * _matvec(R.T.copy(), t)).astype(F32))
    named = [np.zeros(len(C["kps"]), bool), np.zeros(len(M["kps"]), bool)]
    for q, tr in S["matches"]:
        named[0][q], named[1][tr] = True, True
    calls, up_old = [], 0
    for src, dst, sim, need, nm in ((C, M, Smc, 3, named[0]), (M, C, (s, R, t), 1, named[1])):
        rows = np.flatnonzero(~nm & ((src["flags"] & need) == need))
        ok, uv, octave = sim3_project(src["pos"][rows], src["max_dist"][rows], src["min_dist"][rows], src["Rcw"], src["tcw"], sim, sc.CAM, src["bounds"], log_sf)
        rows = rows[ok]
        q, up = area_query(dst, rows, uv[ok], octave[ok], src["desc"][rows], 7.5, ((dst["flags"] & 3) != 3).astype(np.uint8))
        calls.append((rows, q))
        up_old += up

    def plain_pair():
        return [ctx.search_in_area_features(**q) for _, q in calls]

    res = plain_pair()
    new = {}
    for ic, b in zip(calls[0][0], accept(res[0], ratio)):
        if b >= 0:
            new[int(ic)] = int(b)
    for im, b in zip(calls[1][0], accept(res[1], ratio)):
        if b >= 0:
            new.setdefault(int(b), int(im))
    got = stored_pair()
    assert got == sorted(new.items()), "the stored pair call and the two searches disagree"
    up_stored = pad(4 * len(sc.SF)) + sum(pad(k) + pad(12 * k) + 2 * pad(4 * k) for k in (len(C["kps"]), len(M["kps"])))
    t_s, t_p = alternate(stored_pair, plain_pair, a.reps, a.warmup)
    stored_pair()
    t_c, _ = alternate(lambda: ctx.lib.orbfe_search_by_sim3_stored(*ctx._sim3_search_args), lambda: None, a.reps, a.warmup)
    d_s, l_s = device_ms(ctx, stored_pair, max(a.reps // 2, 5))
    d_p, l_p = device_ms(ctx, plain_pair, max(a.reps // 2, 5))
    pair = {"case": f"2 stored keyframes x {n} features, {int((C['flags'] & 1).sum())} / {int((M['flags'] & 1).sum())} good points, "
                    f"{len(S['matches'])} input matches, th 7.5", "new_pairs": len(got), "stored_ms": stats(t_s), "stored_bare_c_call_ms": stats(t_c),
            "two_searches_ms": stats(t_p),
            "device_ms": {"stored": round(d_s, 4), "two_searches": round(d_p, 4)}, "launch_groups": {"stored": l_s, "two_searches": l_p},
            "upload_bytes": {"stored": int(up_stored), "two_searches": int(up_old)}}

    # ---- the points ----
    sw, Rw, tw = S["Scw"]

    def stored_points():
        return ctx.search_by_sim3_points_stored(st, C_ID, loop, (Rw, tw), sw, sc.CAM, sc.SF, 10.0, ratio, 50)

    rows = np.flatnonzero(loop["usable"])
    ok, uv, octave = sim3_project(loop["pos"][rows], loop["max_dist"][rows], loop["min_dist"][rows], None, None, (sw, Rw, tw), sc.CAM, C["bounds"], log_sf)
    for k in np.flatnonzero(ok):                                   # the viewing-angle test (src/ORBMatcher.cc:534-536)
        pc = _affine(sw, Rw, loop["pos"][rows[k]], tw)
        dws = F32(np.sqrt(np.float64(pc[0]) ** 2 + np.float64(pc[1]) ** 2 + np.float64(pc[2]) ** 2))
        rv = _matvec(Rw, loop["view_dir"][rows[k]])
        ok[k] = not (np.float64(rv[0]) * np.float64(pc[0]) + np.float64(rv[1]) * np.float64(pc[1]) + np.float64(rv[2]) * np.float64(pc[2]) < 0.5 * np.float64(dws))
    rows = rows[ok]
    pq, up_old_p = area_query(C, rows, uv[ok], octave[ok], loop["desc"][rows], 10.0, None)

    def plain_points():
        return ctx.search_in_area_features(**pq)

    want = np.full(len(loop["usable"]), -1, np.int64)
    want[rows] = accept(plain_points(), ratio)
    bi, _ = stored_points()
    assert np.array_equal(bi, want), "the stored points call and the one search disagree"
    m = len(loop["usable"])
    up_stored_p = pad(4 * len(sc.SF)) + pad(m) + 2 * pad(12 * m) + 2 * pad(4 * m) + pad(32 * m)
    t_s, t_p = alternate(stored_points, plain_points, a.reps, a.warmup)
    d_s, l_s = device_ms(ctx, stored_points, max(a.reps // 2, 5))
    d_p, l_p = device_ms(ctx, plain_points, max(a.reps // 2, 5))
    points = {"case": f"{m} loop points ({int(loop['usable'].sum())} usable, {len(rows)} searched) into a stored keyframe x {n} features, th 10",
              "matched": int((bi >= 0).sum()), "stored_ms": stats(t_s), "one_search_ms": stats(t_p),
              "device_ms": {"stored": round(d_s, 4), "one_search": round(d_p, 4)}, "launch_groups": {"stored": l_s, "one_search": l_p},
              "upload_bytes": {"stored": int(up_stored_p), "one_search": int(up_old_p)}}
    out = {"equal": True, "reps": a.reps, "note": "the replaced path is timed without its host projection loop, acceptance and merge", "pair": pair,
           "points": points}
    st.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
