#!/usr/bin/env python3
"""Measures orbfe_fuse_into_keyframes (Context.fuse_into_keyframes) and writes ONE JSON line (and the file given by --out).
Case: 61 target keyframes x 2000 features against a current keyframe of 2000 features (tests/fuse_scenes.gpu_scene("full")).
  one_call_ms      host to host of Context.fuse_into_keyframes, median / p99 over --reps after --warmup
  chain_ms         in the same process, what the parent's entry points need for the same tables: per target one
                   Context.project_map_points and one Context.search_in_area_features (2 x 61 calls, each with its own upload, launches,
                   synchronisation and download), median / p99 over --chain-reps
  split_ms         of the one call: flatten = the binding's argument preparation (one_call - the bare C call with prepared arguments),
                   device = the three kernels between HIP events (orbfe_profile_enable, MATCH stage, measured in separate repetitions),
                   upload / download = the same arrays (count and sizes) copied host -> device / device -> host with torch in this process
                   (a replay of the copies, not a probe inside the call), other = the bare C call minus those three
The two routes are checked to give the same tables before anything is timed.
Usage: python tools/fuse_bench.py [--reps 100] [--chain-reps 10] [--out profiles/fuse_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fuse_restatement as fr  # noqa: E402
import fuse_scenes as fs  # noqa: E402
from orb_slam2_ros2_amd._lib import Context  # noqa: E402

F32 = np.float32


def chain(ctx, sc):
    cur, pts = sc["cur"], sc["pts"]
    n, K = len(cur["kps"]), len(sc["targets"])
    octave = cur["kps"]["octave"].astype(np.int32)
    radius = (F32(3.0) * (fs.SF[octave] * fs.SF[octave])).astype(F32)
    qxy = np.stack([cur["kps"]["x"], cur["kps"]["y"]], 1)
    bi, bd, vis = np.empty((K, n), np.int32), np.empty((K, n), np.int32), np.empty((K, n), np.uint8)
    for k, t in enumerate(sc["targets"]):
        lo, hi = fr.octave_window(octave, sc["z"][k], fs.BL)
        b, d, s, nc = ctx.search_in_area_features(t["kps"], t["desc"], qxy, radius, lo, hi, cur["desc"], bounds=t["bounds"])
        ok = (nc > 0) & (d.astype(F32) / s.astype(F32) < F32(0.6)) & (d < 50)
        bi[k], bd[k] = np.where(ok, b, -1), np.where(ok, d, 0)
        p = ctx.project_map_points(pts["pos"], pts["view_dir"], pts["max_dist"], pts["min_dist"], t["Rcw"], t["tcw"], fs.CAM, t["bounds"])
        vis[k] = np.where(pts["has_point"] > 0, p["visible"], 0)
    return bi, bd, vis


def timed(f, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def stats(t):
    return {"median": round(float(np.median(t)), 4), "p99": round(float(np.percentile(t, 99)), 4)}


def copy_replay(sc, reps):
    """the call's copies replayed with torch: every uploaded array from pageable memory, the three result tables back"""
    import torch
    cur, pts = sc["cur"], sc["pts"]
    ups = [cur["kps"], cur["desc"]] + [np.ascontiguousarray(v) for v in pts.values()]
    for t in sc["targets"]:
        ups += [t["kps"], t["desc"]]
    ups = [torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()) for a in ups if a.size]
    dev = [torch.empty(len(a), dtype=torch.uint8, device="cuda") for a in ups]
    K, n = len(sc["targets"]), len(cur["kps"])
    d_out = [torch.empty(K * n * b, dtype=torch.uint8, device="cuda") for b in (4, 4, 1)]
    h_out = [torch.empty(K * n * b, dtype=torch.uint8) for b in (4, 4, 1)]

    def up():
        for a, d in zip(ups, dev):
            d.copy_(a, non_blocking=True)
        torch.cuda.synchronize()

    def down():
        for d, h in zip(d_out, h_out):
            h.copy_(d)
        torch.cuda.synchronize()
    up(), down()
    return float(np.median(timed(up, reps))), float(np.median(timed(down, reps))), int(sum(len(a) for a in ups)), len(ups)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--chain-reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sc = fs.gpu_scene("full")
    ctx = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
    run = lambda: ctx.fuse_into_keyframes(sc["cur"], sc["pts"], sc["targets"], sc["z"], fs.CAM, fs.BL, fs.SF)  # noqa: E731
    got, want = run(), chain(ctx, sc)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), "the one call and the chain disagree"
    for _ in range(a.warmup):
        run()
    one = timed(run, a.reps)
    ch = timed(lambda: chain(ctx, sc), a.chain_reps)
    # the bare C call: the binding's last prepared arguments again (Context keeps them in _fuse_args)
    bare = timed(lambda: ctx.lib.orbfe_fuse_into_keyframes(*ctx._fuse_args), a.reps)
    ctx.profile_enable(2 + 6)                                  # the MATCH stage only, in the production schedule
    ctx.profile_read(reset=True)
    for _ in range(a.reps):
        ctx.lib.orbfe_fuse_into_keyframes(*ctx._fuse_args)
    dev_ms, _ = ctx.profile_read(reset=True)["match"]
    ctx.profile_enable(0)
    up_ms, down_ms, up_bytes, up_copies = copy_replay(sc, max(a.reps // 4, 5))
    device = dev_ms / a.reps                                   # (one timed interval per call)
    bare_med = float(np.median(bare))
    out = {"case": "61 target keyframes x 2000 features, 2000 current features", "matches": int((got[0] >= 0).sum()), "visible": int(got[2].sum()),
           "one_call_ms": stats(one), "chain_ms": stats(ch), "chain_calls": 2 * len(sc["targets"]), "reps": a.reps, "chain_reps": a.chain_reps,
           "bare_call_ms": stats(bare), "upload_bytes": up_bytes, "upload_copies": up_copies,
           "split_ms": {"flatten": round(float(np.median(one)) - bare_med, 4), "upload": round(up_ms, 4), "device": round(device, 4),
                        "download": round(down_ms, 4), "other": round(bare_med - up_ms - device - down_ms, 4)}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
