#!/usr/bin/env python3
"""Measures orbfe_pose_graph_optimize_ex (Optimizer::optimizeEssentialGraph on the device) with both linear solvers -- 1 dense
(launch_lba_chol), 2 the block-sparse Cholesky (k_pgsparse.hip) -- in ONE run on one box, optimize(20) as the reference calls it, and
writes ONE JSON line (and profiles/essential_graph_bench.json with --out; the rows that file already holds under essential_graph_100 /
_500 / _1000, the parent commit's dense figures, are kept under "parent_commit").
Graphs: loop-closure graphs with about 4 edges per vertex (tests/essential_graph_sparse_cases.py: chain, covisibility to the 2nd, 3rd
and 4th neighbour, a corrected group, loop edges into the fixed vertex, and far edges between non-fixed vertices so that the factor has
fill) of 25, 50, 100, 500 and 1000 keyframes with both solvers, 1500 and 2500 sparse only (the dense solver stops at 1024 non-fixed
vertices); and one dense-ish graph of 500 keyframes, every vertex joined to 32 random others, whose factor fills almost completely:
solver 0 must send it to the dense solver; and bands of half-width 8 .. 48 (every vertex joined to its next w neighbours) at 100, 500 and
1000 keyframes, which locate the guard of solver 0 in blocks per column of the factor.  The dense-ish and band rows run ONE iteration (a
trial of the sparse solver on a full factor takes seconds, and in the first iteration both solvers see identical Jacobians, so their
results must agree to rounding): their per-trial figures are what compares.
Each row: host -> host time of the C call through the Python binding (median, p99), a series with the context's stage events on for the
device time between the events around the loop, and one call with ORBFE_PG_PHASES set for the split into build / assemble / solve /
evaluate (wall time with the stream synchronised after every phase), from which the per-trial time of the linear solve (assemble + the
factor-and-solve phase, divided by the trials).  Before timing, every result is checked: chi2 must have fallen by more than 1e6 (the
graphs are consistent, the minimum is 0); the sparse result must agree with the dense one within 1e-6 wherever both run; the
100-keyframe results are compared with the restatement (tests/essential_graph_restatement.py) within 1e-6.
The expectations this tool tests are in DESIGN 4.24 and 4.26, written before anything was measured.  There is no CPU figure for g2o:
g2o is not available where this runs, and none is invented.
Usage: python tools/essential_graph_bench.py [--out profiles/essential_graph_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import essential_graph_cases as K  # noqa: E402
import essential_graph_restatement as R  # noqa: E402
import essential_graph_sparse_cases as S  # noqa: E402
import sim3_opt_restatement as s3  # noqa: E402
from orb_slam2_ros2_amd._lib import Context  # noqa: E402

SOLVER = {"dense": 1, "sparse": 2}


def summary(s):
    ms = np.asarray(s) * 1e3
    return {"median": round(float(np.median(ms)), 3), "p99": round(float(np.percentile(ms, 99)), 3), "n": len(ms)}


def denseish_graph(n_free, degree, seed=1):
    """the far-edge graph of n_free non-fixed vertices with every vertex joined to `degree` random others, consistent measurements"""
    g = S.make_graph(n_free, hops=(2, 3, 4))
    rng = np.random.default_rng(seed)
    verts = [v for v in range(n_free + 1) if v != g["isolated"]]
    edges, meas = [tuple(e) for e in g["edges"]], [tuple(m) for m in g["meas"]]
    for a in verts:
        for b in rng.choice([v for v in verts if v != a], size=degree, replace=False):
            C = s3.sim3_mul(tuple(g["true"][int(b)]), s3.sim3_inverse(tuple(g["true"][a])))
            edges.append((a, int(b)))
            meas.append(C[:7] + (1.0,))
    g["edges"], g["meas"] = np.array(edges, np.int32), np.array(meas, np.float64)
    return g


def measure(ctx, g, solver, iterations, reps, warmup, check_against=None):
    args = K.args(g)
    chi0 = float(R.edge_chi2(R.errors(R.Graph(*args), g["estimates"])).sum())
    est, chi2, stats = ctx.pose_graph_optimize(*args, iterations=iterations, solver=solver)
    assert stats[2] == solver
    if iterations >= 20:
        assert chi2.sum() * 1e6 < chi0, (solver, chi0, chi2.sum())
    r = {"non_fixed": int((g["fixed"] == 0).sum()), "edges": int(len(g["edges"])), "solver": solver, "iterations_asked": iterations,
         "iterations": stats[0], "trials": stats[1], "l_blocks": stats[3], "chi2_initial": chi0, "chi2_final": float(chi2.sum())}
    nf = r["non_fixed"]
    r["fill_percent_of_dense_triangle"] = round(100.0 * stats[3] / (nf * (nf + 1) / 2), 2) if stats[3] else None
    if check_against is not None:
        r["max_abs_diff_to_dense"] = float(np.abs(est - check_against).max())
        assert r["max_abs_diff_to_dense"] < 1e-6
    host = []
    for i in range(reps + warmup):
        t0 = time.perf_counter()
        ctx.pose_graph_optimize(*args, iterations=iterations, solver=solver)
        host.append(time.perf_counter() - t0)
    r["host_ms"] = summary(host[warmup:])
    ctx.profile_enable(2 + 7)           # the "ba" stage only
    ctx.profile_read(True)
    dev = []
    for i in range(reps + warmup):
        ctx.pose_graph_optimize(*args, iterations=iterations, solver=solver)
        ms, k = ctx.profile_read(True)["ba"]
        dev.append(ms * 1e-3 / max(k, 1))
    ctx.profile_enable(False)
    r["device_ms_between_events"] = summary(dev[warmup:])
    os.environ["ORBFE_PG_PHASES"] = "1"
    t0 = time.perf_counter()
    _, _, st = ctx.pose_graph_optimize(*args, iterations=iterations, solver=solver)
    r["synchronised_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    del os.environ["ORBFE_PG_PHASES"]
    ph = ctx.debug_pose_graph_phases()
    r["split_ms_synchronised"] = dict(zip(("build", "assemble", "solve", "evaluate"), (round(v, 3) for v in ph)))
    r["solve_share"] = round(ph[2] / max(sum(ph), 1e-9), 3)
    r["linear_solve_ms_per_trial"] = round((ph[1] + ph[2]) / max(st[1], 1), 4)
    r["factor_and_solve_ms_per_trial"] = round(ph[2] / max(st[1], 1), 4)
    return r, est


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="25,50,100,500,1000,1500,2500")
    ap.add_argument("--denseish", default="500,32", help="keyframes,degree of the dense-ish graph; empty: none")
    ap.add_argument("--band-sizes", default="100,500,1000")
    ap.add_argument("--band-widths", default="8,12,16,24,32,48")
    a = ap.parse_args()
    ctx = Context(640, 480, n_features=500, max_images=1)
    res = {"tool": "essential_graph_bench", "unit": "ms", "iterations_asked": 20, "g2o_cpu_ms": None,
           "g2o_cpu_note": "not measured: g2o is not available where this tool runs"}
    if a.out and os.path.exists(a.out):
        old = json.loads(open(a.out).read())
        res["parent_commit"] = old.get("parent_commit") or {k: v for k, v in old.items() if k.startswith("essential_graph_")}
    for n in (int(v) for v in a.sizes.split(",") if v):
        reps, warmup = (30, 3) if n <= 100 else ((10, 2) if n <= 500 else (5, 1))
        g = S.make_graph(n - 1, hops=(2, 3, 4))
        dense_est = None
        for name in ("dense", "sparse"):
            if name == "dense" and n - 1 > 1024:
                continue
            r, est = measure(ctx, g, SOLVER[name], 20, reps, warmup, dense_est if name == "sparse" else None)
            r["keyframes"] = n
            if name == "dense":
                dense_est = est
            if n <= 100:
                want = R.optimize(*K.args(g), iterations=6)
                got = ctx.pose_graph_optimize(*K.args(g), iterations=6, solver=SOLVER[name])
                r["max_abs_diff_to_restatement_6_iterations"] = float(np.abs(got[0] - want["est"]).max())
                assert r["max_abs_diff_to_restatement_6_iterations"] < 1e-6 and got[2][:2] == (want["iterations"], want["trials"])
            res[f"pg_{n}_{name}"] = r
            print(f"{n} keyframes, {name}: host {r['host_ms']}, per trial {r['linear_solve_ms_per_trial']} ms, l_blocks {r['l_blocks']}", file=sys.stderr)
        if dense_est is not None:
            d, s = res[f"pg_{n}_dense"]["host_ms"], res[f"pg_{n}_sparse"]["host_ms"]
            res[f"pg_{n}_dense_over_sparse"] = round(d["median"] / s["median"], 3)
    if a.denseish:
        n, degree = (int(v) for v in a.denseish.split(","))
        g = denseish_graph(n - 1, degree)
        dense_est = None
        for name in ("dense", "sparse"):
            r, est = measure(ctx, g, SOLVER[name], 1, 2, 0, dense_est if name == "sparse" else None)
            r["keyframes"], r["degree"] = n, degree
            dense_est = est
            res[f"pg_denseish_{n}_{name}"] = r
            print(f"dense-ish {n}, {name}: host {r['host_ms']}, per trial {r['linear_solve_ms_per_trial']} ms, l_blocks {r['l_blocks']}", file=sys.stderr)
    # bands of growing half-width: where the sparse solver stops paying, in blocks per column of the factor (the guard of solver 0)
    for n in (int(v) for v in a.band_sizes.split(",") if v):
        for w in (int(v) for v in a.band_widths.split(",") if v):
            g = S.make_graph(n - 1, hops=tuple(range(2, w + 1)))
            dense_est = None
            for name in ("dense", "sparse"):
                r, est = measure(ctx, g, SOLVER[name], 1, 3, 1, dense_est if name == "sparse" else None)
                r["keyframes"], r["half_bandwidth"] = n, w
                dense_est = est
                res[f"pg_band_{n}_w{w}_{name}"] = r
            d, sp = res[f"pg_band_{n}_w{w}_dense"], res[f"pg_band_{n}_w{w}_sparse"]
            print(f"band {n} w {w}: {sp['l_blocks'] / (n - 1):.1f} blocks a column; per trial dense {d['linear_solve_ms_per_trial']} ms, sparse "
                  f"{sp['linear_solve_ms_per_trial']} ms", file=sys.stderr)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
