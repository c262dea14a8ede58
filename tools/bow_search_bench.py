#!/usr/bin/env python3
"""Measures searchByBow over stored keyframes (Context.search_by_bow_stored) against the path it replaces -- a loop of
ORBMatcher.searchByBow, one orbfe_match_bruteforce call per candidate -- in ONE process on one box, and writes ONE JSON line (and the file
given by --out).
  workload      one frame against 20 candidate keyframes x 2000 features (tests/bow_search_scenes.scene(3, K=20, n=2000)), tracking mode
                (Tracking::filterKFByBow: ratio 0.75, orientation check), the candidates resident in a KeyframeStore.
  equal         the two results are compared first, element for element and in order.
  *_ms          median / p99 of --reps runs of each, alternating, host clock around the synchronous call.  The loop's FeatureVector
                dictionaries are built before the clock starts (a caller holds them as DBoW3 maps); its host walk, list flattening, ratio
                test and verifyAngle are inside, as they are for its callers.
  upload_bytes  what each path copies host -> device per frame: counted from the arrays handed to orbfe_match_bruteforce / from the stored
                call's layout (records, flags, the query's arrays; every array padded to 256 bytes as the scratch layout pads it).
  device_ms     between HIP events around the launches (the MATCH stage timer, separate repetitions), per frame.
Exit code 1 (after the line is written) when the stored call is slower than the loop of the same run.
Usage: python tools/bow_search_bench.py [--reps 100] [--out profiles/bow_search_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bow_search_scenes as bs  # noqa: E402
import tri_scenes as ts  # noqa: E402
import triangulation_restatement as tr  # noqa: E402
from orb_slam2_ros2_amd._lib import Context, KeyframeStore  # noqa: E402
from orb_slam2_ros2_amd.frontend import ORBMatcher  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=20)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    K, n = a.candidates, a.features
    query, cands = bs.scene(3, K=K, n=n, n_pts=n * 3 // 2, skewed=False)
    ctx = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
    st = KeyframeStore(ts.W, ts.H, 8)
    ids = bs.fill_store(st, cands)
    flags = [kf["flags"] for kf in cands]
    hq = bs.host_query(query)
    m = ORBMatcher(0.75, True)

    def stored():
        return ctx.search_by_bow_stored(st, hq, ids, flags, bs.TRACK, m.mfRatio, m.mnMinThreshold, m.mbCheckOri)

    fq = query["flags"]
    fv_q = tr.featvec_dict(query["fv"])
    per_kf = [dict(desc_f=query["desc"], desc_kf=kf["desc"], featvec_f=fv_q, featvec_kf=tr.featvec_dict(kf["fv"]), good_f=(fq & 1) != 0,
                   inmap_f=(fq & 2) != 0, good_kf=(kf["flags"] & 1) != 0, inmap_kf=(kf["flags"] & 2) != 0, angles_f=query["kps"]["angle"],
                   angles_kf=kf["kps"]["angle"]) for kf in cands]
    up_loop = [0]

    def counting(q, t, off, cand):
        up_loop[0] += pad(np.asarray(q).nbytes) + pad(np.asarray(t).nbytes) + pad(np.asarray(off).nbytes) + pad(np.asarray(cand).nbytes)
        return ctx.match_bruteforce(q, t, off, cand)

    def loop(best_match=None):
        return [m.searchByBow(ctx, best_match=best_match, **kw) for kw in per_kf]

    a_res, b_res = [bs.as_tuples(x) for x in stored()], loop(counting)
    assert a_res == b_res, "the stored call and the per-candidate loop disagree"
    assert a_res == [bs.oracle(query, kf, bs.TRACK, 0.75, True) for kf in cands], "the stored call and the CPU oracle disagree"
    nodes, offs, feats = query["fv"]
    up_stored = pad(K * 56) + sum(pad(len(f)) for f in flags) + pad(len(fq)) + pad(query["desc"].nbytes) + pad(4 * len(fq)) + pad(nodes.nbytes) + \
        pad(offs.nbytes) + pad(feats.nbytes)
    ts_, tl = alternate(stored, loop, a.reps, a.warmup)
    c_stored = lambda: ctx.lib.orbfe_search_by_bow_stored(*ctx._bow_search_args)  # noqa: E731
    tb, _ = alternate(c_stored, lambda: None, a.reps, a.warmup)
    ds, ls = device_ms(ctx, stored, max(a.reps // 2, 5))
    dl, ll = device_ms(ctx, loop, max(a.reps // 2, 5))
    out = {"case": f"{K} candidate keyframes x {n} features, tracking mode, ratio 0.75, orientation check", "equal": True,
           "matches": int(sum(len(x) for x in a_res)), "reps": a.reps, "stored_ms": stats(ts_), "loop_ms": stats(tl), "stored_bare_c_call_ms": stats(tb),
           "upload_bytes": {"stored": int(up_stored), "loop": int(up_loop[0])},
           "device_ms": {"stored": round(ds, 4), "loop": round(dl, 4)}, "launch_groups": {"stored": ls, "loop": ll},
           "stored_not_slower": bool(np.median(ts_) <= np.median(tl))}
    st.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    # the one condition: the stored call is not slower than the per-candidate loop of the same run (medians of alternating repetitions)
    if not out["stored_not_slower"]:
        sys.exit("the stored call is slower than the per-candidate loop of the same run")


if __name__ == "__main__":
    main()
