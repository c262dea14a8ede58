#!/usr/bin/env python3
"""Measures Context.track_local_map_stored (the local map points named by id in a device-resident MapPointStore) against
Context.track_local_map (their arrays uploaded with the call), in ONE process on one box, and writes ONE JSON line (and --out).

Per size (2000 and 5000 map points: the range of a KITTI local map; tests/test_track_chain.py's scene, its points repeated with a few
centimetres of jitter up to the size): the two results are compared first (every output, as integers); then host-to-host times of
--reps calls of each through the Python bindings, INTERLEAVED -- arrays, stored, arrays again -- after --warmup rounds.  Every call ends
in its own device synchronisation, so a host clock around it is the call's time.  `arrays_again` is the same call as `arrays` a moment
later: the difference of their medians is the spread the stored call's difference has to be read against.  bytes_uploaded: what each
form copies to the device per call (the map points' share and the whole upload).
--lib PATH: a liborbfe_hip.so of another commit (one without the store): only the array call is measured, as `arrays`, for the
comparison with that commit on the same box.
Usage: python tools/mpstore_bench.py [--reps 300] [--warmup 30] [--out profiles/mpstore_bench.json] [--lib PATH]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class OlderLibrary(ctypes.CDLL):
    """A library of an earlier commit for --lib: an entry point it does not export reads as an inert object that takes the argtypes
    _lib.load() assigns and cannot be called.  Only the array call is measured on such a library."""

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if not name.startswith("orbfe_"):
                raise
            missing = type("MissingEntryPoint", (), {})()
            setattr(self, name, missing)
            return missing


def stats(t):
    return {"median": round(float(np.median(t)), 4), "p10": round(float(np.percentile(t, 10)), 4), "p90": round(float(np.percentile(t, 90)), 4)}


def sized(s, n, rng):
    """the scene's map points repeated up to n, every repetition a few centimetres off the original"""
    N = len(s["pos"])
    idx = np.arange(n) % N
    pos = s["pos"][idx].copy()
    pos[N:] += rng.normal(0, 0.03, (max(n - N, 0), 3)).astype(np.float32)
    held = s["held"].copy()
    held[held >= n] = -1
    return dict(pos=pos[:n], view_dir=s["view_dir"][idx], max_dist=s["max_dist"][idx], min_dist=s["min_dist"][idx], desc=s["mp_desc"][idx],
                flags=s["flags"][idx], held=held)


def same(a, b):
    return (all(np.array_equal(a[k], b[k]) for k in ("assigned", "edge_of", "inlier")) and np.array_equal(a["pose"].view(np.uint64), b["pose"].view(np.uint64))
            and all(a[k] == b[k] for k in ("n_matches", "n_edges", "n_good")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 5000])
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    from orb_slam2_ros2_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
        ctypes.CDLL = OlderLibrary            # (this process only: _lib.load() declares entry points such a library may lack)
    import test_track_chain as T
    ctx = _lib.Context(T.W, T.H, n_features=T.NF, max_images=2)
    scene = T._scene(ctx, 3)
    sig2 = (T.SF * T.SF).astype(np.float32)
    tail = (scene["Rcw"], scene["tcw"], (T.FX, T.FY, T.CX, T.CY, T.BF), (0.0, float(T.W), 0.0, float(T.H)), scene["pose_se3"], sig2,
            (np.float32(1.0) / sig2).astype(np.float32))
    frame_bytes = T.NF * (4 + 8) + 2 * 4 * len(sig2) + 56
    res = {"tool": "mpstore_bench", "library": os.path.basename(args.lib) if args.lib else "this tree", "reps": args.reps, "warmup": args.warmup, "n_features": T.NF, "sizes": {}}
    ok = True
    rng = np.random.default_rng(5)
    for n in args.sizes:
        m = sized(scene, n, rng)
        kw = dict(held=m["held"], right_u=scene["right_u"])
        arrays = lambda: ctx.track_local_map(0, m["pos"], m["view_dir"], m["max_dist"], m["min_dist"], m["desc"], m["flags"], *tail, **kw)  # noqa: E731
        entry = {"n_map_points": n, "bytes_uploaded": {"arrays": {"map_points": 73 * n, "call": 73 * n + frame_bytes}}}
        if args.lib:
            for _ in range(args.warmup):
                arrays()
            t = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                arrays()
                t.append((time.perf_counter() - t0) * 1e3)
            entry["ms"] = {"arrays": stats(t)}
        else:
            store = _lib.MapPointStore()
            ids = (rng.permutation(3 * n)[:n] + 11).astype(np.uint64)           # gapped, in no order
            store.upsert(ids, m["pos"], m["view_dir"], m["max_dist"], m["min_dist"], m["desc"])
            stored = lambda: ctx.track_local_map_stored(0, store, ids, m["flags"], *tail, **kw)  # noqa: E731
            a, g = arrays(), stored()
            entry["results_equal"] = bool(same(a, g))
            entry["n_matches"], entry["n_edges"] = int(a["n_matches"]), int(a["n_edges"])
            ok = ok and entry["results_equal"]
            entry["bytes_uploaded"]["stored"] = {"map_points": 9 * n, "call": 9 * n + 8 + frame_bytes}
            for _ in range(args.warmup):
                arrays(), stored()
            ta, ts, ta2 = [], [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                arrays()
                t1 = time.perf_counter()
                stored()
                t2 = time.perf_counter()
                arrays()
                t3 = time.perf_counter()
                ta.append((t1 - t0) * 1e3), ts.append((t2 - t1) * 1e3), ta2.append((t3 - t2) * 1e3)
            entry["ms"] = {"arrays": stats(ta), "stored": stats(ts), "arrays_again": stats(ta2)}
            entry["stored_minus_arrays_ms"] = round(float(np.median(ts) - np.median(ta)), 4)
            entry["spread_of_arrays_ms"] = round(float(abs(np.median(ta2) - np.median(ta))), 4)
            store.close()
        res["sizes"][str(n)] = entry
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
