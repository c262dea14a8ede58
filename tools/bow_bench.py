#!/usr/bin/env python3
"""Measures the bag-of-words path and prints ONE JSON line:
  parse_s              orbfe_vocab_load_txt of the full-size text vocabulary (k = 10, L = 6, 1 111 111 nodes; generated into a temporary
                       directory by orb_slam2_ros2_amd.synth_vocab.full)
  one_image_us         orbfe_bow_transform host -> host of the 2000 product descriptors of one KITTI-sized synth frame on that vocabulary
                       (Context.bow_transform, Python call included): median / p99 over --calls calls
  slots_ms             orbfe_bow_slots over --slots extracted left images (host -> host wall of the call, the download of the whole
                       result block included), median over --reps calls, and us per image
Usage: python tools/bow_bench.py [--calls 2000] [--slots 512] [--reps 20] [--only one|slots]
The device time of the two kernels comes from a kernel trace of the same tool, one run per call shape:
  rocprofv3 --kernel-trace --memory-copy-trace --stats -d DIR -- python tools/bow_bench.py --only one --calls 500
  rocprofv3 --kernel-trace --memory-copy-trace --stats -d DIR -- python tools/bow_bench.py --only slots --reps 10"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orb_slam2_ros2_amd import synth, synth_vocab  # noqa: E402
from orb_slam2_ros2_amd._lib import Context, Vocabulary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=("one", "slots"), default=None, help="time one call shape only (for a kernel trace of it)")
    a = ap.parse_args()
    out = {"tool": "bow_bench"}
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "voc.txt")
        t0 = time.perf_counter()
        voc = synth_vocab.full(0, 10, 6)
        synth_vocab.write_txt(p, voc)
        out["generate_s"] = round(time.perf_counter() - t0, 3)
        out["vocab_mb"] = round(os.path.getsize(p) / 1e6, 1)
        t0 = time.perf_counter()
        v = Vocabulary.load_txt(p)
        out["parse_s"] = round(time.perf_counter() - t0, 3)
    out["vocab"] = v.info()
    ctx = Context(1241, 376, n_features=2000, n_levels=8, device_id=0, max_images=a.slots)
    imgs = [synth.stereo_pair_content(f, synth.CONTENT_CLASSES[f % 4])[0] for f in range(a.slots)]
    t0 = time.perf_counter()
    feats = []
    for s in range(0, a.slots, 64):
        feats += ctx.extract_slots(s, imgs[s:s + 64])
    out["extract_s"] = round(time.perf_counter() - t0, 3)
    d = feats[0][1]
    out["one_image_features"] = int(len(d))
    t0 = time.perf_counter()
    ctx.bow_transform(v, d, 4)   # the first call uploads the vocabulary
    out["first_call_upload_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    ts = []
    for _ in range(0 if a.only == "slots" else a.calls):
        t0 = time.perf_counter()
        ctx.bow_transform(v, d, 4)
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts if ts else [0.0]) * 1e6
    out["one_image_us"] = {"median": round(float(np.median(ts)), 1), "p99": round(float(np.percentile(ts, 99)), 1), "calls": a.calls}
    ts = []
    for _ in range(0 if a.only == "one" else a.reps + 1):
        t0 = time.perf_counter()
        ctx.bow_slots(v, 0, a.slots, 4)
        ts.append(time.perf_counter() - t0)
    ms = float(np.median(ts[1:])) * 1e3 if len(ts) > 1 else 0.0
    out["slots_ms"] = {"images": a.slots, "median": round(ms, 3), "us_per_image": round(ms * 1e3 / a.slots, 2), "reps": a.reps,
                       "mean_features": round(float(np.mean([len(f[1]) for f in feats])), 1)}
    print(json.dumps(out))
    ctx.close()
    v.close()


if __name__ == "__main__":
    main()
