#!/usr/bin/env python3
"""Measures the Sim3 RANSAC sets (orbfe_sim3, _lib.Sim3Set) against the EPnP RANSAC sets of the same run and writes ONE JSON line (and
profiles/sim3_bench.json with --out).  Each case times the RANSAC loop host to host (every iterate call from Python, n = 5 per call,
round-robin over the candidates that are not exhausted) over --reps fresh sets after --warmup; set creation is reported apart.
Device time comes from a second series with the library's events on (orbfe_sim3_profile), bytes uploaded from the library's own count.
  sim3_fail_20x300     20 candidates x 300 correspondences of pure outliers: every budget spent -- a false loop candidate set
  sim3_success_round1  20 x 300 with candidate 0 at 10 % outliers: its first call succeeds (a refine passes, the loop stops)
  pnp_fail_20x300      the failing orbfe_pnp loop of the same shape, in the same process: the yardstick
Before timing, the Sim3 failing and success loops and the PnP failing loop are compared call by call with their restatements
(tests/sim3_restatement.py, tests/pnp_restatement.py).  A Sim3 hypothesis is a strict subset of an EPnP hypothesis's work, so the
expectation is that the failing Sim3 loop is not slower than the failing PnP loop of the same run: the tool exits 1 otherwise (the
figures are written either way).
Usage: python tools/sim3_bench.py [--reps 200] [--out profiles/sim3_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pnp_restatement as P  # noqa: E402
import sim3_restatement as S  # noqa: E402
from orb_slam2_ros2_amd._lib import PnPSet, Sim3Set, pnp_engine, sim3_engine  # noqa: E402

N_ITER = 5


def sim3_data(seed, K, N, outliers):
    scenes = [S.scene(np.random.default_rng(seed * 1000 + k), N, outlier=outliers[k]) for k in range(K)]
    off = np.arange(K + 1, dtype=np.int64) * N
    arrays = (off, *(np.concatenate([np.asarray(sc[i]).reshape(-1, w) if w else np.asarray(sc[i]) for sc in scenes])
                     for i, w in ((0, 3), (1, 3), (2, 0), (3, 0), (4, 12), (5, 12))))
    return arrays, scenes


def accept_half(N):
    return lambda p, model, inl: len(set(inl)) * 2 >= N


def sim3_loop(arrays, K, N, profile=False):
    sim3_engine(1)
    t0 = time.perf_counter()
    s = Sim3Set(*arrays, S.SIGMA2, S.CAM)
    t1 = time.perf_counter()
    if profile:
        s.profile(True)
    log = S.loop_closing_loop(s.iterate, K, N_ITER, accept_half(N))
    t2 = time.perf_counter()
    stats, dev = s.stats(), s.profile()
    s.close()
    return log, t1 - t0, t2 - t1, stats, dev


def check_sim3(arrays, scenes, K, N):
    ref = [S.Solver(*sc) for sc in scenes]
    e = S.Engine(1)
    want = S.loop_closing_loop(lambda p, n: ref[p].iterate(e, n), K, N_ITER, accept_half(N))
    got = sim3_loop(arrays, K, N)[0]
    assert len(want) == len(got), (len(want), len(got))
    for (pw, w), (pg, g) in zip(want, got):
        assert pw == pg and w[0] == g[0] and w[1] == g[1] and list(w[3]) == g[3].tolist()
        assert (w[2] is None) == (g[2] is None) and (w[2] is None or np.array_equal(w[2].view(np.uint32), g[2].view(np.uint32)))
    assert sim3_engine() == e.state
    return len(got)


def pnp_data(seed, K, N):
    sc = [P.scene(np.random.default_rng(seed * 1000 + k), N, outlier=1.0) for k in range(K)]
    return (np.arange(K + 1, dtype=np.int64) * N, np.concatenate([s[0] for s in sc]), np.concatenate([s[1] for s in sc]),
            np.concatenate([s[2] for s in sc]))


def pnp_loop(data, K, N):
    pnp_engine(1)
    s = PnPSet(*data, P.SIGMA2, P.CAM)
    t1 = time.perf_counter()

    def it(p, n):
        d = s.iterate(p, n)
        return d[0], d[1], (None if d[2] is None else (d[2], d[3])), d[4]
    log = P.tracking_loop(it, K, N_ITER, lambda p, pose, inl: len(set(inl)) * 2 >= N)
    t2 = time.perf_counter()
    stats = s.stats()
    s.close()
    return log, t2 - t1, stats


def check_pnp(data, K, N):
    off, xyz, uv, oc = data
    ref = [P.Solver(xyz[a:b], uv[a:b], oc[a:b], P.SIGMA2, P.CAM) for a, b in zip(off[:-1], off[1:])]
    e = P.Engine(1)
    want = P.tracking_loop(lambda p, n: ref[p].iterate(e, n), K, N_ITER, lambda p, pose, inl: len(set(inl)) * 2 >= N)
    got = pnp_loop(data, K, N)[0]
    assert len(want) == len(got)
    for (pw, w), (pg, g) in zip(want, got):
        assert pw == pg and w[0] == g[0] and w[1] == g[1] and list(w[3]) == g[3].tolist()
        assert (w[2] is None) == (g[2] is None)
        if w[2] is not None:
            assert np.array_equal(w[2][0].view(np.uint32), g[2][0].reshape(9).view(np.uint32))
            assert np.array_equal(w[2][1].view(np.uint32), g[2][1].view(np.uint32))
    assert pnp_engine() == e.state


def summary(us):
    us = np.asarray(us) * 1e6
    return {"median": round(float(np.median(us)), 1), "p99": round(float(np.percentile(us, 99)), 1), "n": len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    K, N = 20, 300
    fail, fail_sc = sim3_data(1, K, N, [1.0] * K)
    succ, succ_sc = sim3_data(2, K, N, [0.1] + [1.0] * (K - 1))
    pnp = pnp_data(3, K, N)
    calls_fail = check_sim3(fail, fail_sc, K, N)
    calls_succ = check_sim3(succ, succ_sc, K, N)
    check_pnp(pnp, K, N)
    res = {"tool": "sim3_bench", "candidates": K, "correspondences": N, "n": N_ITER, "checked_against_restatements": True}
    for name, arrays, calls in (("sim3_fail_20x300", fail, calls_fail), ("sim3_success_round1", succ, calls_succ)):
        runs = [sim3_loop(arrays, K, N) for _ in range(a.reps + a.warmup)][a.warmup:]      # timed without the events
        prof = [sim3_loop(arrays, K, N, profile=True) for _ in range(a.reps + a.warmup)][a.warmup:]
        log, _, _, stats, (_, nbytes) = runs[-1]
        assert len(log) == calls and all(r[4][1] == nbytes for r in runs + prof)
        res[name] = {"loop_us": summary([r[2] for r in runs]), "create_us_median": round(float(np.median([r[1] for r in runs])) * 1e6, 1),
                     "device_us_between_events": summary([r[4][0] * 1e-6 for r in prof]), "launch_sequences": stats[0],
                     "hypotheses": stats[1], "iterate_calls": calls, "bytes_uploaded": nbytes}
    runs = [pnp_loop(pnp, K, N) for _ in range(a.reps + a.warmup)][a.warmup:]
    res["pnp_fail_20x300"] = {"loop_us": summary([r[1] for r in runs]), "launch_sequences": runs[-1][2][0], "hypotheses": runs[-1][2][1],
                              "iterate_calls": len(runs[-1][0])}
    met = res["sim3_fail_20x300"]["loop_us"]["median"] <= res["pnp_fail_20x300"]["loop_us"]["median"]
    res["expectation"] = {"what": "failing Sim3 loop not slower than the failing PnP loop of the same run (medians)", "met": bool(met)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
