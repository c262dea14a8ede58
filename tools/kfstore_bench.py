#!/usr/bin/env python3
"""Measures the calls over the device-resident keyframe store against their plain counterparts, in ONE process on one box, and writes
ONE JSON line (and the file given by --out).
  fuse          61 target keyframes x 2000 features (tests/fuse_scenes.gpu_scene("full")): Context.fuse_into_keyframes_stored against
                Context.fuse_into_keyframes.  The two results are compared first; then median / p99 of --reps runs of each, alternating.
                split_ms per form: binding = the Python argument preparation (the call minus the bare C call with prepared arguments),
                c_call = the bare C call, kernels = between HIP events (MATCH stage, separate repetitions), download = the three result
                tables copied device -> host with torch (a replay, not a probe inside the call), rest = c_call - kernels - download
                (upload, launches, synchronisation).
  triangulation 1 + 10 keyframes x 2000 features (tests/tri_scenes.scene(0)): create_new_map_points_stored against
                create_new_map_points, the same way (no stage timer covers these kernels: binding / c_call only).
  add_from_slot one keyframe of 2000 features out of an extraction slot, against the route it replaces: fetch_features + fetch_stereo +
                the host add.
  memory        bytes of one 2000-feature keyframe (info: features + grid + FeatureVector) and of 1500 of them by that figure.
Exit code 1 (after the line is written) when a stored call is slower than the plain call of the same run.
Usage: python tools/kfstore_bench.py [--reps 100] [--out profiles/kfstore_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fuse_scenes as fs  # noqa: E402
import tri_scenes as ts  # noqa: E402
from orb_slam2_ros2_amd._lib import Context, KeyframeStore  # noqa: E402


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


def kernels_ms(ctx, call, reps):
    ctx.profile_enable(2 + 6)                                  # the MATCH stage only, in the production schedule
    ctx.profile_read(reset=True)
    for _ in range(reps):
        call()
    ms, _ = ctx.profile_read(reset=True)["match"]
    ctx.profile_enable(0)
    return ms / reps


def download_ms(K, n, reps):
    import torch
    d_out = [torch.empty(K * n * b, dtype=torch.uint8, device="cuda") for b in (4, 4, 1)]
    h_out = [torch.empty(K * n * b, dtype=torch.uint8) for b in (4, 4, 1)]

    def down():
        for d, h in zip(d_out, h_out):
            h.copy_(d)
        torch.cuda.synchronize()
    down()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        down()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def fuse_case(ctx, reps, warmup):
    sc = fs.gpu_scene("full")
    K, n = len(sc["targets"]), len(sc["cur"]["kps"])
    st = KeyframeStore(fs.W, fs.H, 8)
    cur_id = 1 << 40
    st.add(cur_id, sc["cur"]["kps"], sc["cur"]["desc"], bounds=sc["cur"]["bounds"])
    ids = []
    for k, t in enumerate(sc["targets"]):
        if t is sc["cur"]:
            ids.append(cur_id)
            continue
        st.add(1 + k, t["kps"], t["desc"], bounds=t["bounds"])
        ids.append(1 + k)
    plain = lambda: ctx.fuse_into_keyframes(sc["cur"], sc["pts"], sc["targets"], sc["z"], fs.CAM, fs.BL, fs.SF)  # noqa: E731
    stored = lambda: ctx.fuse_into_keyframes_stored(st, cur_id, sc["pts"], ids, sc["targets"], sc["z"], fs.CAM, fs.BL, fs.SF)  # noqa: E731
    a, b = plain(), stored()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "the stored and the plain fuse disagree"
    tp, tsd = alternate(plain, stored, reps, warmup)
    c_plain = lambda: ctx.lib.orbfe_fuse_into_keyframes(*ctx._fuse_args)  # noqa: E731
    c_stored = lambda: ctx.lib.orbfe_fuse_into_keyframes_stored(*ctx._fuse_stored_args)  # noqa: E731
    bp, bs = alternate(c_plain, c_stored, reps, warmup)
    kp, ks = kernels_ms(ctx, c_plain, reps), kernels_ms(ctx, c_stored, reps)
    down = download_ms(K, n, max(reps // 4, 5))
    up_plain = sum(t["kps"].nbytes + t["desc"].nbytes for t in sc["targets"]) + sc["cur"]["kps"].nbytes + sc["cur"]["desc"].nbytes
    up_common = K * 128 + n * (1 + 12 + 12 + 4 + 4) + 32        # target records, cur's slot points, scale factors

    def split(call, bare, kern):
        c = float(np.median(bare))
        return {"binding": round(float(np.median(call)) - c, 4), "c_call": round(c, 4), "kernels": round(kern, 4), "download": round(down, 4),
                "rest": round(c - kern - down, 4)}
    st.close()
    return {"case": f"{K} target keyframes x 2000 features, {n} current features", "equal": True, "matches": int((a[0] >= 0).sum()), "reps": reps,
            "plain_ms": stats(tp), "stored_ms": stats(tsd), "plain_bare_ms": stats(bp), "stored_bare_ms": stats(bs),
            "upload_bytes": {"plain": up_plain + up_common, "stored": up_common},
            "split_ms": {"plain": split(tp, bp, kp), "stored": split(tsd, bs, ks)},
            "stored_not_slower": bool(np.median(tsd) <= np.median(tp))}


def tri_case(ctx, reps, warmup):
    cur, nbs, _ = ts.scene(0, n_nb=10, n=2000)
    st = KeyframeStore(ts.W, ts.H, 8)
    cur_id, ids = 1 << 40, list(range(1, 1 + len(nbs)))
    for kid, kf in [(cur_id, cur)] + list(zip(ids, nbs)):
        st.add(kid, kf["kps"], kf["desc"], kf["depth"], kf["right_u"])
        st.set_bow(kid, *kf["fv"])
    args = (ts.CAM, ts.k_inv(), ts.BL, ts.SF)
    plain = lambda: ctx.create_new_map_points(cur, nbs, *args)  # noqa: E731
    stored = lambda: ctx.create_new_map_points_stored(st, cur_id, cur, ids, nbs, *args)  # noqa: E731
    a, b = plain(), stored()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "the stored and the plain triangulation disagree"
    tp, tsd = alternate(plain, stored, reps, warmup)
    c_stored = lambda: ctx.lib.orbfe_create_new_map_points_stored(*ctx._tri_stored_args)  # noqa: E731
    for _ in range(warmup):
        c_stored()
    bs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        c_stored()
        bs.append((time.perf_counter() - t0) * 1e3)
    info = st.info(1)
    st.close()
    return {"case": f"1 + {len(nbs)} keyframes x 2000 features", "equal": True, "records": int(len(a[0])), "reps": reps, "plain_ms": stats(tp),
            "stored_ms": stats(tsd), "stored_bare_ms": stats(bs), "stored_binding_ms": round(float(np.median(tsd) - np.median(bs)), 4),
            "stored_not_slower": bool(np.median(tsd) <= np.median(tp)), "keyframe_bytes_with_bow": info["bytes"]}


def slot_case(reps, warmup):
    from orb_slam2_ros2_amd import synth
    L, R = synth.stereo_pair(0, 1241, 376)
    c = Context(1241, 376, n_features=2000, n_levels=8, device_id=0, max_images=2)
    c.frame_stereo(L, R, 718.856, 386.1448)
    st = KeyframeStore(1241, 376, 8)
    n = st.add_from_slot(c, 0, 0, 0)
    nxt = [1]

    def from_slot():
        st.add_from_slot(c, nxt[0], 0, 0)
        nxt[0] += 1

    def round_trip():
        kps, desc = c.fetch_features(0)
        _, ru, dp, _, _ = c.fetch_stereo(0)
        st.add(nxt[0], kps, desc, dp[:len(kps)], ru[:len(kps)])
        nxt[0] += 1
    a, b = alternate(from_slot, round_trip, reps, warmup)
    g0, g1 = st.fetch(1), st.fetch(2)
    assert all(g0[k].tobytes() == g1[k].tobytes() for k in ("kps", "desc", "depth", "right_u", "cell_off", "cell_feat"))
    out = {"features": n, "add_from_slot_ms": stats(a), "fetch_and_add_ms": stats(b), "keyframe_bytes": st.info(0)["bytes"], "reps": reps}
    st.close()
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
    out = {"fuse": fuse_case(ctx, a.reps, a.warmup), "triangulation": tri_case(ctx, a.reps, a.warmup), "add_from_slot": slot_case(a.reps, a.warmup)}
    per = out["triangulation"]["keyframe_bytes_with_bow"]
    out["memory"] = {"bytes_per_keyframe_2000": per, "bytes_1500_keyframes": 1500 * per}
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    # the one condition: a stored call is not slower than the plain call of the same run (medians of alternating repetitions)
    slow = [k for k in ("fuse", "triangulation") if not out[k]["stored_not_slower"]]
    if slow:
        sys.exit("stored call slower than the plain call of the same run: " + ", ".join(slow))


if __name__ == "__main__":
    main()
