"""The graphs of the block-sparse pose-graph solver's tests (orbfe_pose_graph_optimize_ex, solver 2): make_graph of
tests/essential_graph_cases.py, consistent family only, plus FAR EDGES BETWEEN NON-FIXED VERTICES.

Why.  The loop edges of the existing family all end in the fixed vertex, which has no block row: its system is a band, the Cholesky
factor has exactly the blocks of the matrix (3064 in, 3064 out at 1025 block rows) and the fill path of a sparse factorisation would
never run.  Here the last vertices of the corrected group (up to four) are also joined to early non-fixed ones (the first non-fixed
vertices of the chain, as many), the first such pair in both orientations: rows that reach from the end of the band to its start and
fill every column between (1025 block rows: 3068 off-diagonal blocks in, 7132 out, at most 7 below a diagonal).  The measurements are
relative poses of the same ONE configuration `true` the estimates have drifted away from, so the minimum still has chi2 = 0 and is known
in closed form: every edge error is zero iff S_v = true_v * G for one G, and the fixed vertex f decides G = true_f^-1 * est_f.

make_graph returns the dict of essential_graph_cases.make_graph with two more keys: true (nv, 8) and far (the indices of the far
edges).  `true` is not something that generator returns, so its chain is replayed here from the same seed, draw for draw
(test_pg_sparse_host.py checks that the replay reproduces the generator's measurements bit for bit).

Qualification, by the convention of essential_graph_cases (its module text): qualify() here is that module's qualify() on this family.
ADM[n] = (iterations, the two restatement runs' spread there, bound): 1e-6 where the spread is <= 1e-8, 100 x the spread otherwise;
CONV[n] = (iterations, spread) of the run to convergence, bound 1e-6.  At 1025 only one iteration is admitted: the second iteration's
spread is already 3.9e-6 (the numeric Jacobians' noise times the chain's conditioning), so past one iteration the restatement is no
yardstick there -- the closed form is -- and it costs 6 s an iteration.  Measured by test_pg_sparse_host.py's recomputation.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import essential_graph_cases as K
import essential_graph_restatement as R
import sim3_opt_restatement as s3

SIZES = (1, 2, 7, 12, 99, 257)          # the optimiser against the restatement
BIG = 1025                              # one past the dense solver's bound
BOUND = K.BOUND
# measured by qualify(); see the module text
ADM = {1: (1, 2.3e-16, 1e-6), 2: (2, 9.2e-11, 1e-6), 7: (2, 3.3e-10, 1e-6), 12: (2, 1.4e-10, 1e-6), 99: (2, 9.2e-9, 1e-6),
       257: (2, 4.7e-8, 4.7e-6), 1025: (1, 2.1e-13, 1e-6)}
CONV = {1: (3, 8.9e-16), 2: (4, 1.2e-16), 7: (4, 1.4e-15), 12: (4, 5e-16), 99: (7, 3.6e-15), 257: (8, 1.8e-14)}
MIN_REDUCTION = 1e20


def _true_configuration(n_free, seed, step, drift):
    """the chain of essential_graph_cases.make_graph replayed: the same generator, the same draws in the same order"""
    rng = np.random.default_rng(1000 * n_free + seed)
    nv = n_free + 1
    isolated = 4 if n_free >= 7 else (1 if n_free >= 3 else None)
    chain = [v for v in range(nv) if v != isolated]

    def unit(S):
        nq = math.sqrt(sum(c * c for c in S[:4]))
        return tuple(c / nq for c in S[:4]) + S[4:7] + (1.0,)

    true = {}
    T = K._rand_sim3(rng, 1.0, 2.0)
    for k, v in enumerate(chain):
        if k:
            T = s3.sim3_mul(K._rand_sim3(rng, step[0], step[1]), T)
            K._rand_sim3(rng, drift[0], drift[1])
        T = unit(T)
        true[v] = T
    return chain, true


def make_graph(n_free, seed=0, hops=(2, 3)):
    g = dict(K.make_graph(n_free, seed=seed, hops=hops))
    chain, true = _true_configuration(n_free, seed, (0.3, 0.2), (2e-3, 1e-2))
    nv = n_free + 1
    cand = [v for v in chain if v != g["fixed_v"]]
    group = cand[len(cand) - max(1, len(cand) // 5):]
    late, early = group[-4:], cand[:4]
    edges, meas, far = [tuple(e) for e in g["edges"]], [tuple(m) for m in g["meas"]], []

    def add(a, b):
        C = s3.sim3_mul(true[b], s3.sim3_inverse(true[a]))
        far.append(len(edges))
        edges.append((a, b))
        meas.append(C[:7] + (1.0,))

    for a, b in zip(late, early):
        if abs(chain.index(a) - chain.index(b)) <= 3:
            continue                     # (a graph too short to have a far pair: the chain already joins the two)
        add(a, b)
        if len(far) == 1:
            add(b, a)                    # one pair in both orientations
    g["edges"] = np.array(edges, np.int32).reshape(-1, 2)
    g["meas"] = np.array(meas, np.float64).reshape(-1, 8)
    g["true"] = np.array([true.get(v, (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)) for v in range(nv)], np.float64)
    g["far"] = far
    return g


@functools.lru_cache(maxsize=None)
def graph(n_free):
    return make_graph(n_free)


@functools.lru_cache(maxsize=None)
def reference(n_free, iterations=20):
    """the restatement on graph(n_free): ONE run of `iterations`; a shorter run is its prefix (essential_graph_cases.prefix)"""
    return R.optimize(*K.args(graph(n_free)), iterations=iterations)


def qualify(n_free, max_iterations):
    """essential_graph_cases.qualify() on this family: that function builds its graph with the module's make_graph when it is given
    keyword arguments, so for the length of the call that name is this module's generator"""
    g = graph(n_free)
    theirs = K.make_graph
    K.make_graph = lambda n, **kw: g
    try:
        return K.qualify(n_free, max_iterations=max_iterations, seed=0)
    finally:
        K.make_graph = theirs


def closed_form_minimum(g):
    """(nv, 8): S_v = true_v * G, G = true_f^-1 * est_f at the fixed vertex f; the isolated vertex keeps its estimate"""
    f = g["fixed_v"]
    G = s3.sim3_mul(s3.sim3_inverse(tuple(float(x) for x in g["true"][f])), tuple(float(x) for x in g["estimates"][f]))
    out = g["estimates"].copy()
    for v in range(len(out)):
        if v != g["isolated"] and v != f:
            out[v] = s3.sim3_mul(tuple(float(x) for x in g["true"][v]), G)
    return out


def align_sign(est, want):
    """q and -q are one rotation: every row of est with the quaternion sign of the row of want"""
    s = np.where((est[:, :4] * want[:, :4]).sum(1) < 0, -1.0, 1.0)
    out = est.copy()
    out[:, :4] *= s[:, None]
    return out


def lower_pattern(g):
    """the block structure of Hpp: (nb, sorted list of (i, j), i > j, of the joined pairs of block rows)"""
    slot = np.full(len(g["fixed"]), -1, np.int64)
    free = np.flatnonzero(g["fixed"] == 0)
    slot[free] = np.arange(free.size)
    pairs = set()
    for a, b in g["edges"]:
        i, j = int(slot[a]), int(slot[b])
        if i >= 0 and j >= 0:
            pairs.add((max(i, j), min(i, j)))
    return int(free.size), sorted(pairs)


def symbolic(nb, pairs):
    """Elimination tree and fill, restated: column k of the factor has the rows of the matrix's column k and, from every child c (the
    columns whose first row below the diagonal is k), the rows of c except k.  -> (parent [nb], rows [nb] ascending, diagonal first)"""
    rows = [{k} for k in range(nb)]
    for i, j in pairs:
        rows[min(i, j)].add(max(i, j))
    parent = [-1] * nb
    for k in range(nb):
        below = sorted(rows[k] - {k})
        if below:
            parent[k] = below[0]
            rows[below[0]] |= set(below[1:])
    return parent, [[k] + sorted(r - {k}) for k, r in enumerate(rows)]


def spd_system(nb, pairs, seed):
    """a block-sparse SPD system with that pattern: (low_row, low_col, blocks (n_low, 36) row-major, dense (6 nb, 6 nb), rhs); the
    diagonal blocks first, in order.  Off-diagonal blocks are random with entries of order 1; a diagonal block is M M^T plus the block
    row's absolute row sums (diagonal dominance), so the matrix is positive definite whatever the pattern."""
    rng = np.random.default_rng(seed)
    n = 6 * nb
    A = np.zeros((n, n))
    for i, j in pairs:
        B = rng.normal(size=(6, 6))
        A[6 * i:6 * i + 6, 6 * j:6 * j + 6] = B
        A[6 * j:6 * j + 6, 6 * i:6 * i + 6] = B.T
    dom = np.abs(A).sum(1)
    for k in range(nb):
        M = rng.normal(size=(6, 6))
        A[6 * k:6 * k + 6, 6 * k:6 * k + 6] = M @ M.T + np.diag(dom[6 * k:6 * k + 6] + 1.0)
    A = 0.5 * (A + A.T)
    low = [(k, k) for k in range(nb)] + [(max(i, j), min(i, j)) for i, j in pairs]
    blocks = np.array([A[6 * i:6 * i + 6, 6 * j:6 * j + 6].reshape(36) for i, j in low])
    return (np.array([p[0] for p in low], np.int32), np.array([p[1] for p in low], np.int32), blocks, A, rng.normal(size=n))


# ---- a large scene for tests/cpp/test_essential_dropin.cpp ----------------------------------------------------------------------------
def dropin_chain_scene(n):
    """A map of n good keyframes (ids 0 .. n - 1) after a loop closure, in the input format of tests/cpp/test_essential_dropin.cpp: a chain
    with the spanning tree i -> i - 1 and covisibility 150 / 120 to the first and second neighbours; current n - 1, loop keyframe 1 (fixed,
    not id 0); the last five keyframes corrected by the loop Sim3; loop connections (n - 1, 1) and (n - 1, 2); an older loop edge
    (n - 3, 4) between two non-fixed keyframes, which is what fills the factor.  Returns (text, dict(ids))."""
    rng = np.random.default_rng(n)
    ids = list(range(n))
    S = K._rand_sim3(rng, 0.8, 1.0)
    model = {}
    for i in ids:
        S = s3.sim3_mul(K._rand_sim3(rng, 0.1, 0.2), S)
        model[i] = s3.sim3_to_model(S)
    G = K._rand_sim3(rng, 0.02, 0.1)
    moved = ids[-5:]
    corrected = {i: s3.sim3_to_model(s3.sim3_mul(s3.sim3_from_model(model[i]), G)) for i in moved}
    uncorrected = {i: model[i] for i in moved}
    cov = {i: [(j, w) for j, w in ((i - 1, 150), (i + 1, 150), (i - 2, 120), (i + 2, 120)) if 0 <= j < n] for i in ids}
    cov[n - 1].append((2, 60))
    cov[2].append((n - 1, 60))
    loops = {n - 3: [4]}
    conn = {n - 1: [1, 2]}
    fl = lambda a: " ".join(repr(float(v)) for v in np.asarray(a, np.float32))
    lines = [f"{n} {n - 1}"]
    for i in ids:
        lines.append(f"{i} 0 {i - 1} {fl(model[i])} {len(loops.get(i, []))} " + " ".join(map(str, loops.get(i, []))) +
                     f" {len(cov[i])} " + " ".join(f"{a} {w}" for a, w in cov[i]))
    for m in (corrected, uncorrected):
        lines.append(str(len(m)))
        lines += [f"{i} {fl(v)}" for i, v in m.items()]
    lines.append(str(len(conn)))
    lines += [f"{i} {len(v)} " + " ".join(map(str, v)) for i, v in conn.items()]
    lines.append(f"1 {n - 1} 50")
    lines.append("1")
    lines.append(f"0 {fl(rng.normal(size=3))} 7 -1 -1")
    return "\n".join(lines) + "\n", dict(ids=ids)
