#!/usr/bin/env python3
"""Measures Tracking::trackReference as one call (Context.track_reference_stored) against the three-call chain it replaces
-- Context.bow_slots, Context.search_by_bow_stored with the frame as a host query, Context.pose_only_optimize, with setMapPoints, the
edge list and the post-check in vectorised numpy in between -- in ONE process, Python binding on both sides, and writes ONE JSON line
(and --out).  The scene is tests/track_reference_scenes.py's ACCEPT scene grown to 2000 frame features x 2000 keyframe features.
The two routes' matches, inlier flags, final assignments and poses are compared first; then median / p99 of --reps runs of each,
alternating (host to host); the bare C call of the one call; device milliseconds between events, the MATCH and BA stages of each route
(separate repetitions; the chain's bow_slots launches are outside any timed stage); the bytes each route uploads.
The case runs in a child process of its own under a time limit.
Usage: python tools/track_reference_bench.py [--reps 200] [--out profiles/track_reference_bench.json]"""
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

LIMIT_S = 300


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


def case(reps, warmup, tmp):
    import reloc_refine_restatement as rr
    import track_reference_restatement as tr
    import track_reference_scenes as sc
    from oracle.pyoracle import Oracle
    from orb_slam2_ros2_amd import synth, synth_vocab
    from orb_slam2_ros2_amd._lib import BOW_TRACK, Context, KeyframeStore, Vocabulary
    orc = Oracle()
    n = len(sc.frame(orc, 11)["lk"])
    s = sc.build(orc, image_seed=11, n_match=1500, n_bad=100, n_dup=60, n_fill=n - 1660, rng_seed=9001)
    ctx = Context(sc.W, sc.H, n_features=sc.NF, max_images=2)
    (kps, desc), _ = ctx.extract_batch(list(synth.stereo_pair(11)))
    assert np.array_equal(kps, s["kps"]) and np.array_equal(desc, s["desc"])
    path = os.path.join(tmp, "trained.txt")
    synth_vocab.write_txt(path, sc.vocabulary()[0])
    vocab = Vocabulary.load_txt(path)
    st = KeyframeStore(sc.W, sc.H)
    KF = 77
    st.add(KF, s["kf_kps"], s["kf_desc"], bounds=sc.BOUNDS)
    st.set_bow(KF, *s["kf_fv"])
    n_kp, NF, N, nl = s["n_kp"], sc.NF, len(s["good"]), 8
    fx, fy, cx, cy, bf = (float(np.float32(v)) for v in s["cam"])
    p_init = rr.tcw_to_se3(s["Rcw"], s["tcw"])
    angle = np.ascontiguousarray(s["kps"]["angle"][:n_kp])
    up = {"chain": 0}

    def one():
        return ctx.track_reference_stored(0, vocab, st, KF, s["good"], s["pos"], s["Rcw"], s["tcw"], s["cam"], s["bounds"], s["sigma2"],
                                          s["inv_sigma2"], right_u=s["right_u"], levelsup=s["levelsup"], want_bow=True)

    def chain():
        bow = ctx.bow_slots(vocab, 0, 1, levelsup=s["levelsup"])[0]
        q = dict(desc=s["desc"][:n_kp], fv=bow[2:], angle=angle, flags=None)
        m = ctx.search_by_bow_stored(st, q, [KF], [s["good"]], BOW_TRACK, 0.7, 50, True)[0]
        a = np.full(NF, -1, np.int32)
        a[m["query"]] = m["train"]                                    # setMapPoints: of repeated indices the last assignment stays
        if len(m) < 10:
            return dict(matches=m, verdict=tr.REJECT_MATCHES, final_assigned=a)
        ef, Xw, meas, info, sig = tr.edge_arrays(s, a)
        _, pose, inl = ctx.pose_only_optimize(Xw, meas, info, sig, p_init, fx, fy, cx, cy, bf)
        c = tr.post_check(s, a, ef, inl, pose)
        up["chain"] = n_kp * 36 + (2 * len(bow[2]) + 1 + len(bow[4])) * 4 + N + 56 + len(ef) * 60 + 56
        return dict(matches=m, verdict=tr.ACCEPT if c["n_inliers"] >= 10 else tr.REJECT_INLIERS, final_assigned=c["final"], pose_se3=pose,
                    inlier=c["inlier"], n_inliers=c["n_inliers"], n_edges=len(ef))

    a, b = chain(), one()
    assert np.array_equal(a["matches"], b["matches"]) and a["verdict"] == b["verdict"] and np.array_equal(a["final_assigned"], b["final_assigned"])
    assert np.array_equal(a["inlier"], b["inlier"]) and np.array_equal(a["pose_se3"].view(np.uint64), b["pose_se3"].view(np.uint64))
    t_chain, t_one = alternate(chain, one, reps, warmup)
    c_args, c_keep = ctx.track_reference_call(0, vocab, st, KF, s["good"], s["pos"], s["Rcw"], s["tcw"], s["cam"], s["bounds"], s["sigma2"],
                                              s["inv_sigma2"], right_u=s["right_u"], levelsup=s["levelsup"], want_bow=True)
    bare = lambda: ctx.lib.orbfe_track_reference_stored(*c_args)  # noqa: E731
    t_bare, _ = alternate(bare, lambda: None, reps, warmup)
    device = {"one_call": {}, "chain": {}}
    for stage, key in ((6, "match"), (7, "ba")):
        ctx.profile_enable(2 + stage)
        ctx.profile_read(reset=True)
        for _ in range(reps):
            bare()
        device["one_call"][key] = round(ctx.profile_read(reset=True)[key][0] / reps, 4)
        for _ in range(reps):
            chain()
        device["chain"][key] = round(ctx.profile_read(reset=True)[key][0] / reps, 4)
        ctx.profile_enable(0)
    res = {"case": f"{n_kp} frame features x {N} keyframe features, {b['n_matches']} matches, {b['n_edges']} edges", "equal": True,
           "verdict": b["verdict_name"], "n_inliers": b["n_inliers"], "reps": reps, "chain_ms": stats(t_chain), "one_call_ms": stats(t_one),
           "one_call_bare_c_ms": stats(t_bare), "device_ms": device,
           "bytes_up": {"one_call": N * 13 + NF * 9 + 2 * nl * 4 + 56, "chain": up["chain"]}, "device_calls": {"one_call": 1, "chain": 3},
           "one_call_faster": bool(np.median(t_one) < np.median(t_chain))}
    st.close()
    vocab.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="(internal) run the case in this process, with this scratch directory, and print its JSON")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(case(a.reps, a.warmup, a.case)))
        return
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", tmp, "--reps", str(a.reps), "--warmup", str(a.warmup)],
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
