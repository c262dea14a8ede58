"""The graphs the pose-graph optimiser's tests share (orbfe_pose_graph_optimize against tests/essential_graph_restatement.py), and the
restatement's results on them, computed once per process.

A graph (make_graph) is what Optimizer::optimizeEssentialGraph builds after a loop closure, seeded:
  * a keyframe chain with general rotations (0.3 rad, 0.2 m a step) whose estimates carry accumulated odometry drift, joined by
    spanning-tree edges (i, i + 1) and covisibility edges to the 2nd and 3rd neighbour, in both orientations;
  * a corrected group at the end of the chain whose estimates were moved by the loop Sim3 (0.25 rad, 0.3 m): the edges across its
    boundary start with relative angles far on the acos side of Sim3::log's d > 1 - 1e-5 switch (4.5e-3 rad), the edges inside it and
    the drifted ones (2e-3 rad a step) on the small-angle side, and every edge crosses to that side as the optimisation converges;
  * loop edges from the group's last vertices into the early, FIXED vertex (index 2, never 0);
  * one isolated non-fixed vertex (n_free >= 3) and one chain pair joined twice, (a, b) and (b, a).
n_free counts the non-fixed vertices: the block rows of the system.

Two families.  consistent=True (the default, the GPU cases): every measurement is the relative pose of ONE configuration the estimates
have drifted away from, so the minimum has chi2 = 0.  consistent=False (realistic()): the measurements come from the uncorrected
estimates, times exp(noise) (1e-4 or 1e-2 rad, either side of the switch), and the loop edges from the corrected ones, as
Optimizer.cc:804-877 takes them; the minimum keeps a residual.

Qualification.  The device is compared with the restatement at 1e-6 per estimate entry, the project's bound for its
optimisers; that bound may stand only where the restatement alone stays well inside it.  qualify() runs the restatement twice, as
specified and with every per-block edge sum reversed and the system solved by numpy.linalg.solve.  What it found, and why the cases
are what they are:
  * The numeric Jacobians carry rounding noise of ~1e-7 relative, and that noise is a different draw at estimates that differ in the
    last bit.  Two runs agree to 1e-13 after the first iteration (same estimates, same Jacobians) and to cond * 1e-7 * |step| after the
    second.  Where the minimum keeps a residual the difference stays: 1e-6 .. 1e-4 at 99 to 257 vertices in the realistic family, so
    no realistic case of those sizes is inside 1e-8 beyond one iteration.  In the consistent family the steps shrink to nothing and so
    does the difference: <= 3e-14 once converged.  Hence the GPU cases are the consistent ones.
  * g2o's Levenberg-Marquardt has no convergence test.  optimize(20) keeps iterating at the minimum, where the gain ratio is (chi2
    noise) / (scale + 1e-3): 0 to within rounding, with a sign that is noise.  More: the ratio's denominator carries that 1e-3, so
    EVERY step that lowers chi2 by less than 1e-6 has a ratio within 1e-3 of 0, however clear the decrease.  No graph that converges
    within 20 iterations -- every graph here does, in 3 to 7 -- passes the gain-ratio condition for the whole run.
  So each size has three comparisons, at three iteration counts (the count is an argument of the call):
  ADM[n]   = (iterations, difference, bound): the longest prefix over which both conditions on the sequences hold as the issue states
             them (same accept / reject sequence, no gain ratio within 1e-3 of 0).  Bound 1e-6 where the difference is <= 1e-8, else
             100 x the difference (sizes 100, 101, 257: the second iteration's Jacobian noise).  Estimates, chi2, iteration and trial
             counts are compared.
  CONV[n]  = (iterations, difference): the longest prefix over which the sequences are equal and every trial is either that far from
             0 or ROBUSTLY accepted (chi2 at most a tenth of the chi2 before: a decision no rounding turns), with a difference <= 1e-8
             at its end.  This is the run to convergence (chi2 falls by > 1e25).  Bound 1e-6; estimates, chi2 and counts compared.
  20 iterations: the two restatement runs agree to 3e-14 in the estimates but not in their trial counts (noise decides at the
             minimum), so estimates (1e-6) and chi2 are compared and the counts are not.
test_essential_graph_host.py recomputes both tables (CONV[101] is one short of what qualify() finds: the seventh step there ends at the
rounding floor, a hundredth of the chi2 before it, and the tables are meant to hold under another BLAS).
"""
from __future__ import annotations

import functools
import math

import numpy as np

import essential_graph_restatement as R
import sim3_opt_restatement as s3

SIZES = (1, 2, 7, 99, 100, 101, 257)
BOUND = 1e-6
QUAL_DIFF = 1e-8
QUAL_RHO = 1e-3
# measured by qualify(); see the module text
ADM = {1: (1, 2.3e-16, 1e-6), 2: (2, 9.2e-11, 1e-6), 7: (2, 3.4e-11, 1e-6), 99: (2, 6.6e-9, 1e-6), 100: (2, 1.47e-8, 1.47e-6),
       101: (2, 3.35e-8, 3.35e-6), 257: (2, 3.60e-8, 3.60e-6)}
CONV = {1: (3, 8.9e-16), 2: (4, 1.2e-16), 7: (4, 1.0e-15), 99: (6, 3.5e-15), 100: (6, 8.0e-15), 101: (6, 8.0e-15), 257: (7, 2.8e-14)}
MIN_REDUCTION = 1e20           # consistent family at CONV: the minimum is 0, chi2 ends at rounding level (measured: > 8e25)
MIN_REDUCTION_REALISTIC = 4.0  # realistic family after 20 iterations (measured: 6.2 at 7 vertices, 466 at 99)
REALISTIC = dict(consistent=False, noise=1.0, loop=(0.25, 1.5), step=(0.3, 1.0))


def _rand_sim3(rng, ang, tr):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    w = ax * ang
    return s3.sim3_exp([float(w[0]), float(w[1]), float(w[2])] + [float(v) for v in rng.normal(size=3) * tr])


def make_graph(n_free, seed=0, drift=(2e-3, 1e-2), noise=0.0, loop=(0.25, 0.3), step=(0.3, 0.2), consistent=True, hops=(2, 3)):
    """Returns dict(estimates (nv, 8), fixed (nv,), edges (ne, 2), meas (ne, 8), isolated (index or None), dup (the two edge indices of
    the pair joined twice)).  drift = (rad, m) per step, loop = (rad, m) of the loop correction; noise=False and loop=None: drift-free
    (every edge starts at zero error)."""
    rng = np.random.default_rng(1000 * n_free + seed)
    nv = n_free + 1
    fixed_v = min(2, nv - 1)
    isolated = 4 if n_free >= 7 else (1 if n_free >= 3 else None)
    chain = [v for v in range(nv) if v != isolated]
    nc = len(chain)
    # uncorrected estimates along the chain: general rotations, drift accumulated on the left
    unc, true = {}, {}
    S = T = _rand_sim3(rng, 1.0, 2.0)

    def unit(S):
        nq = math.sqrt(sum(c * c for c in S[:4]))
        return tuple(c / nq for c in S[:4]) + S[4:7] + (1.0,)

    for k, v in enumerate(chain):
        if k:
            D = _rand_sim3(rng, step[0], step[1])
            S, T = s3.sim3_mul(D, S), s3.sim3_mul(D, T)
            if drift:
                S = s3.sim3_mul(_rand_sim3(rng, drift[0], drift[1]), S)
        S, T = unit(S), unit(T)
        unc[v], true[v] = S, T
    est = dict(unc)
    cand = [v for v in chain if v != fixed_v]
    group = cand[len(cand) - max(1, len(cand) // 5):] if loop else []
    if loop:
        Gc = _rand_sim3(rng, loop[0], loop[1])
        for v in group:
            est[v] = s3.sim3_mul(unc[v], Gc)
    if isolated is not None:
        est[isolated] = _rand_sim3(rng, 0.7, 3.0)
    edges, meas = [], []

    def add(a, b, src):
        if consistent:
            src = true  # every measurement is the relative pose of ONE configuration: the minimum has chi2 = 0
        C = s3.sim3_mul(src[b], s3.sim3_inverse(src[a]))
        if noise:
            lvl = (1e-4, 1e-3) if rng.random() < 0.5 else (1e-2, 3e-2)
            C = s3.sim3_mul(_rand_sim3(rng, noise * lvl[0], noise * lvl[1]), C)
        edges.append((a, b))
        meas.append(C[:7] + (1.0,))

    for k in range(nc - 1):
        add(chain[k], chain[k + 1], unc)
    for hop in hops:
        for k in range(nc - hop):
            add(chain[k + hop], chain[k], unc)  # (either orientation occurs: pkf1 is the keyframe being visited)
    dup = None
    if nc >= 2:
        a, b = chain[nc // 2 - 1], chain[nc // 2]
        dup = (chain.index(a), len(edges))  # the spanning edge (a, b) and this one, (b, a)
        add(b, a, unc)
    for v in (group[-3:] if loop else chain[-1:]):
        if v != fixed_v and (fixed_v, v) not in edges and (v, fixed_v) not in edges:
            add(v, fixed_v, est)  # loop connections: measured between the corrected estimates
    fixed = np.zeros(nv, np.uint8)
    fixed[fixed_v] = 1
    return dict(estimates=np.array([est[v] for v in range(nv)], np.float64), fixed=fixed, edges=np.array(edges, np.int32).reshape(-1, 2),
                meas=np.array(meas, np.float64).reshape(-1, 8), isolated=isolated, dup=dup, fixed_v=fixed_v)


def args(g):
    return g["estimates"], g["fixed"], g["edges"], g["meas"]


@functools.lru_cache(maxsize=None)
def graph(n_free):
    return make_graph(n_free)


@functools.lru_cache(maxsize=None)
def realistic(n_free):
    return make_graph(n_free, **REALISTIC)


@functools.lru_cache(maxsize=None)
def reference(n_free, iterations=20):
    """the restatement on graph(n_free): ONE run of `iterations`; a shorter run is its prefix (prefix())"""
    return R.optimize(*args(graph(n_free)), iterations=iterations)


def prefix(ref, k):
    """what a run of k iterations returns, from a longer run of the restatement: (estimates, iterations, trials)"""
    k = min(k, ref["iterations"])
    return ref["est_after"][k - 1], k, sum(1 for it in ref["trial_iter"] if it < k)


def qualify(n_free, max_iterations=20, **kw):
    """The two restatement runs of the qualification on graph(n_free) (or make_graph(n_free, **kw)).  Returns (k_adm, diff_adm, k_conv,
    diff_conv, a, b): the longest prefix of iterations over which the two runs take the same accept / reject sequence and every trial's
    gain ratio is at least 1e-3 away from 0, with the runs' largest difference there; and the longest prefix (with a difference of at
    most 1e-8 at its end) over which every trial is either that far from 0 or ROBUSTLY accepted -- its chi2 at most a tenth of the chi2
    before it, a decision rounding cannot turn."""
    g = make_graph(n_free, **kw) if kw else graph(n_free)
    a = R.optimize(*args(g), iterations=max_iterations)
    b = R.optimize(*args(g), iterations=max_iterations, reverse=True, lu=True)

    def trials(r, k):
        return [(acc, rho, c) for acc, rho, c, it in zip(r["accepts"], r["rhos"], r["trial_chi"], r["trial_iter"]) if it < k]

    adm, conv = (0, 0.0), (0, 0.0)
    adm_open = conv_open = True
    for k in range(1, min(len(a["est_after"]), len(b["est_after"])) + 1):
        ta, tb = trials(a, k), trials(b, k)
        if [t[0] for t in ta] != [t[0] for t in tb]:
            break
        diff = float(np.max(np.abs(a["est_after"][k - 1] - b["est_after"][k - 1])))
        far = [abs(t[1]) >= QUAL_RHO for t in ta + tb]
        robust = [f or (t[0] and t[2][1] <= 0.1 * t[2][0]) for f, t in zip(far, ta + tb)]
        adm_open = adm_open and all(far)
        conv_open = conv_open and all(robust)
        if adm_open:
            adm = (k, diff)
        if conv_open and diff <= QUAL_DIFF:
            conv = (k, diff)
    return adm + conv + (a, b)


# ---- the scene of tests/cpp/test_essential_dropin.cpp -----------------------------------------------------------------------------
def dropin_scene():
    """A small map after a loop closure, for dropin::optimizeEssentialGraph over stand-in classes.  Keyframes 0 .. 8 without 6, 7 bad;
    current 8, loop 1 (fixed, not id 0), graphTh 50; corrected and uncorrected Sim3 for 8 and 5.  Returns (text of the input file,
    dict of what the test needs)."""
    rng = np.random.default_rng(17)
    ids = [0, 1, 2, 3, 4, 5, 7, 8]
    S = _rand_sim3(rng, 0.8, 1.0)
    model = {}
    for i in ids:
        S = s3.sim3_mul(_rand_sim3(rng, 0.2, 0.3), S)
        model[i] = s3.sim3_to_model(S)
    G = _rand_sim3(rng, 0.05, 0.2)
    corrected = {i: s3.sim3_to_model(s3.sim3_mul(s3.sim3_from_model(model[i]), G)) for i in (8, 5)}
    uncorrected = {i: model[i] for i in (8, 5)}
    parent = {0: -1, 1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 7: 5, 8: 7}
    loops = {5: [1]}
    cov = {0: [(1, 150), (2, 90)], 1: [(0, 150), (2, 120)], 2: [(1, 120), (3, 101)], 3: [(2, 101), (4, 99)], 4: [(5, 200)],
           5: [(4, 200), (1, 3)], 7: [], 8: [(5, 100)]}
    conn = {8: [1, 2, 7], 5: [1, 4]}
    mps = [(0, rng.normal(size=3), 2, -1, -1), (0, rng.normal(size=3), 3, 8, 5), (1, rng.normal(size=3), 2, -1, -1),
           (0, rng.normal(size=3), 7, -1, -1), (0, rng.normal(size=3), 2, 8, -1)]
    fl = lambda a: " ".join(repr(float(v)) for v in np.asarray(a, np.float32))
    lines = [f"{len(ids)} 8"]
    for i in ids:
        lines.append(f"{i} {1 if i == 7 else 0} {parent[i]} {fl(model[i])} {len(loops.get(i, []))} " + " ".join(map(str, loops.get(i, []))) +
                     f" {len(cov[i])} " + " ".join(f"{a} {w}" for a, w in cov[i]))
    for m in (corrected, uncorrected):
        lines.append(str(len(m)))
        lines += [f"{i} {fl(v)}" for i, v in m.items()]
    lines.append(str(len(conn)))
    lines += [f"{i} {len(v)} " + " ".join(map(str, v)) for i, v in conn.items()]
    lines.append("1 8 50")
    lines.append(str(len(mps)))
    lines += [f"{b} {fl(p)} {r} {lk} {lr}" for b, p, r, lk, lr in mps]
    return "\n".join(lines) + "\n", dict(ids=ids, model=model, corrected=corrected, uncorrected=uncorrected, parent=parent, loops=loops, cov=cov,
                                        conn=conn, mps=mps, loop=1, curr=8, th=50, bad={7})


def dropin_expected_graph(sc):
    """(vertices [(id, fixed, estimate)], loop-connection edges as a set, the other edges in order); an edge is (id1, id2, measurement)"""
    good = [i for i in sc["ids"] if i not in sc["bad"]]
    vS = {i: s3.sim3_from_model(sc["corrected"][i] if i in sc["corrected"] else sc["model"][i]) for i in good}
    verts = [(i, int(i == sc["loop"]), vS[i]) for i in good]
    weight = lambda a, b: dict(sc["cov"][a]).get(b, 0)
    first, done = [], set()
    for id1, lst in sc["conn"].items():
        for id2 in lst:
            if id2 in sc["bad"] or ((id1, id2) != (sc["curr"], sc["loop"]) and weight(id1, id2) < sc["th"]):
                continue
            first.append((id1, id2, s3.sim3_mul(vS[id2], s3.sim3_inverse(vS[id1]))))
            done.add((id1, id2))
    unc = lambda i: s3.sim3_from_model(sc["uncorrected"][i]) if i in sc["uncorrected"] else vS[i]
    rest = []
    for id1 in good:
        others = list(sc["loops"].get(id1, []))
        if sc["parent"][id1] >= 0 and sc["parent"][id1] not in sc["bad"]:
            others.append(sc["parent"][id1])
        others += [a for a, w in sc["cov"][id1] if w >= 100]
        for id2 in others:
            if (id1, id2) in done:
                continue
            done.add((id1, id2))
            rest.append((id1, id2, s3.sim3_mul(unc(id2), s3.sim3_inverse(unc(id1)))))
    return verts, first, rest


def dropin_parse_graph(stdout):
    """the 'v' and 'e' lines of the program -> (vertices, edges) with the doubles decoded from their bits"""
    dec = lambda words: tuple(float(np.array(int(w, 16), np.uint64).view(np.float64)) for w in words)
    verts, edges = [], []
    for ln in stdout.splitlines():
        w = ln.split()
        if w and w[0] == "v":
            verts.append((int(w[1]), int(w[2]), dec(w[3:11])))
        elif w and w[0] == "e":
            edges.append((int(w[1]), int(w[2]), dec(w[3:11])))
    return verts, edges


def dropin_build_command(root, exe):
    import os
    pkg = os.path.join(root, "orb_slam2_ros2_amd")
    return ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(root, "tests", "cpp", "stubs"), "-I" + os.path.join(pkg, "host"),
            "-I" + os.path.join(root, "include"), "-o", exe, os.path.join(root, "tests", "cpp", "test_essential_dropin.cpp"), "-L" + pkg,
            "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"]
