"""Restatement of Optimizer::optimizeEssentialGraph (src/Optimizer.cc:746-920) from the point where the graph is built, under the rules
G1 .. G8 of DESIGN 4.24: the reference for the device optimiser (orbfe_pose_graph_optimize, k_posegraph.hip) and, operation by operation,
for the edge model header csrc/posegraph_edge_dev.h.

Plain fp64, every operation in evaluation order (numpy rounds each elementwise operation once, no fused multiply-add), vectorised over
the edges; acos / sin / cos go through the C library one value at a time (math.*), as the header's host build does.  The group
(quaternions, product, inverse, exp, oplus) is tests/sim3_opt_restatement.py's; its functions take arrays wherever they only do
arithmetic.  A Sim3 is a tuple (qx, qy, qz, qw, tx, ty, tz, s) of floats or of arrays.

  G1  fixed scale only: update[6] = 0, error[6] = log(1) = 0, the 7x7 block problem is the 6x6 one.
  G3  EdgeSim3: err = log(C * S_v0 * S_v1^-1), identity information, chi2 = err . err in index order.
  G4  Sim3::log, sigma = 0 branch: d, deltaR, the d > 1 - 1e-5 switch, W = A Omega + B Omega^2 + I, upsilon = W^-1 t by 3x3
      partial-pivot LU (first largest pivot; the right-hand side eliminated with the rows; U solved a column at a time).
  G5  numeric Jacobians of both vertices: +-1e-9, column = (1 / 2e-9)(e+ - e-); a fixed vertex has none.
  G6  H_ii += Ji^T Ji, H_jj += Jj^T Jj, H_ij += Ji^T Jj, b_i -= Ji^T e, b_j -= Jj^T e; every block summed over its edges in ascending
      edge index (reverse=True: descending, the qualification's second run).
  G7  g2o's Levenberg-Marquardt control (tests/sim3_opt_restatement.py optimize): lambda_0 = 1e-5 max |diag|, at most 10 trials per
      iteration, a failed Cholesky is a rejected trial.
  G8  S <- exp((omega, upsilon, 0)) * S; a step that is exactly zero leaves the estimate's bytes.
"""
from __future__ import annotations

import math

import numpy as np

import sim3_opt_restatement as s3

F64 = np.float64
NUM_DELTA = s3.NUM_DELTA
NUM_SCALE = s3.NUM_SCALE
DBL_MAX = s3.DBL_MAX
LOG_EPS = 1e-5


def cols(a):
    """(n, 8) array -> a Sim3 of 8 arrays"""
    a = np.asarray(a, F64).reshape(-1, 8)
    return tuple(a[:, k].copy() for k in range(8))


def take(S, idx):
    return tuple(c[idx] for c in S)


def _each(f, v):
    return np.array([f(float(x)) for x in v], F64)


# ---- G4 ------------------------------------------------------------------------------------------------------------------------
def lu3_solve(M):
    """x = W^-1 t; M[i][j], j = 0 .. 3: the rows of W with t as the fourth column (arrays or floats)"""
    a, b, c = ([np.asarray(v, F64) for v in M[i]] for i in range(3))
    pb = np.abs(b[0]) > np.abs(a[0])
    big = np.where(pb, np.abs(b[0]), np.abs(a[0]))
    pc = np.abs(c[0]) > big
    for j in range(4):
        aj, bj, cj = a[j], b[j], c[j]
        a[j] = np.where(pc, cj, np.where(pb, bj, aj))
        b[j] = np.where(pc, bj, np.where(pb, aj, bj))
        c[j] = np.where(pc, aj, cj)
    l1, l2 = b[0] / a[0], c[0] / a[0]
    for j in range(1, 4):
        b[j] = b[j] - l1 * a[j]
        c[j] = c[j] - l2 * a[j]
    pc = np.abs(c[1]) > np.abs(b[1])
    for j in range(1, 4):
        bj, cj = b[j], c[j]
        b[j] = np.where(pc, cj, bj)
        c[j] = np.where(pc, bj, cj)
    l3 = c[1] / b[1]
    for j in range(2, 4):
        c[j] = c[j] - l3 * b[j]
    x2 = c[3] / c[2]
    y1 = b[3] - b[2] * x2
    y0 = a[3] - a[2] * x2
    x1 = y1 / b[1]
    y0 = y0 - a[1] * x1
    x0 = y0 / a[0]
    return x0, x1, x2


def sim3_log(S):
    """(n, 6): omega, upsilon of a Sim3 of arrays (or of floats: n = 1)"""
    S = tuple(np.atleast_1d(np.asarray(c, F64)) for c in S)
    R = s3.quat_to_rot(S[:4])
    d = 0.5 * (R[0] + R[4] + R[8] - 1)
    dR = (R[7] - R[5], R[2] - R[6], R[3] - R[1])
    small = d > 1 - LOG_EPS
    with np.errstate(all="ignore"):
        ds = np.where(small, 0.0, d)  # (the other branch's value where the small-angle one is taken: never used)
        theta = _each(lambda v: math.acos(v) if -1.0 <= v <= 1.0 else math.nan, ds)
        theta2 = theta * theta
        k = theta / (2 * np.sqrt(1 - ds * ds))
        A = np.where(small, 0.5, (1 - _each(math.cos, theta)) / theta2)
        B = np.where(small, 1.0 / 6.0, (theta - _each(math.sin, theta)) / (theta2 * theta))
        w = [np.where(small, 0.5 * dR[i], k * dR[i]) for i in range(3)]
        z = np.zeros_like(d)
        Om = [[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]]
        M = []
        for i in range(3):
            row = []
            for j in range(3):
                o2 = 0.0
                for q in range(3):
                    o2 = o2 + Om[i][q] * Om[q][j]
                row.append(A * Om[i][j] + B * o2 + (1.0 if i == j else 0.0))
            row.append(S[4 + i])
            M.append(row)
        u = lu3_solve(M)
    return np.stack([w[0], w[1], w[2], u[0], u[1], u[2]], 1)


# ---- G3, G5 --------------------------------------------------------------------------------------------------------------------
def edge_error(C, S0, S1):
    """(n, 6): log(C * S0 * S1^-1)"""
    with np.errstate(all="ignore"):
        return sim3_log(s3.sim3_mul(s3.sim3_mul(C, S0), s3.sim3_inverse(S1)))


def edge_chi2(E):
    return E[:, 0] * E[:, 0] + E[:, 1] * E[:, 1] + E[:, 2] * E[:, 2] + E[:, 3] * E[:, 3] + E[:, 4] * E[:, 4] + E[:, 5] * E[:, 5]


def perturbed(S, m):
    """sim3_perturbed of every estimate: oplus(+1e-9 e_d) for m = 2 d, oplus(-1e-9 e_d) for m = 2 d + 1"""
    u = [0.0] * 6
    u[m >> 1] = -NUM_DELTA if m & 1 else NUM_DELTA
    return s3.sim3_mul(s3.sim3_exp(u), S)


class Graph:
    def __init__(self, estimates, fixed, edges, meas):
        self.est0 = np.asarray(estimates, F64).reshape(-1, 8).copy()
        self.fixed = np.asarray(fixed, np.uint8).reshape(-1).astype(bool)
        self.edges = np.asarray(edges, np.int32).reshape(-1, 2)
        self.v0, self.v1 = self.edges[:, 0].astype(np.int64), self.edges[:, 1].astype(np.int64)
        self.C = cols(meas)
        self.nv, self.ne = len(self.est0), len(self.edges)
        self.slot = np.full(self.nv, -1, np.int64)
        self.slot[~self.fixed] = np.arange(int((~self.fixed).sum()))
        self.nf = int((~self.fixed).sum())


def errors(G, est):
    S = cols(est)
    return edge_error(G.C, take(S, G.v0), take(S, G.v1))


def linearize(G, est):
    """(E (ne, 6), J0 (ne, 6, 6), J1 (ne, 6, 6)), J[e][row][d]; the Jacobian of a fixed vertex is zero"""
    S = cols(est)
    S0, S1 = take(S, G.v0), take(S, G.v1)
    E = edge_error(G.C, S0, S1)
    J0, J1 = np.zeros((G.ne, 6, 6), F64), np.zeros((G.ne, 6, 6), F64)
    for d in range(6):
        Pp, Pm = perturbed(S, 2 * d), perturbed(S, 2 * d + 1)
        with np.errstate(all="ignore"):
            J0[:, :, d] = NUM_SCALE * (edge_error(G.C, take(Pp, G.v0), S1) - edge_error(G.C, take(Pm, G.v0), S1))
            J1[:, :, d] = NUM_SCALE * (edge_error(G.C, S0, take(Pp, G.v1)) - edge_error(G.C, S0, take(Pm, G.v1)))
    J0[G.fixed[G.v0]] = 0.0
    J1[G.fixed[G.v1]] = 0.0
    return E, J0, J1


def _jtj(Ja, Jb):
    """(ne, 6, 6): sum over the rows r, in order, of Ja[r][a] Jb[r][c]"""
    h = None
    for r in range(6):
        t = Ja[:, r, :, None] * Jb[:, r, None, :]
        h = t if h is None else h + t
    return h


def _jte(J, E):
    s = None
    for r in range(6):
        t = J[:, r, :] * E[:, r, None]
        s = t if s is None else s + t
    return s


# ---- G6 ------------------------------------------------------------------------------------------------------------------------
def build_system(G, E, J0, J1, reverse=False):
    """H (6 nf square, both triangles) and b (6 nf), no lambda"""
    n = 6 * G.nf
    H, b = np.zeros((n, n), F64), np.zeros(n, F64)
    H00, H11, H01 = _jtj(J0, J0), _jtj(J1, J1), _jtj(J0, J1)
    b0, b1 = _jte(J0, E), _jte(J1, E)
    order = range(G.ne - 1, -1, -1) if reverse else range(G.ne)
    for e in order:
        i, j = int(G.slot[G.v0[e]]), int(G.slot[G.v1[e]])
        if i >= 0:
            H[6 * i:6 * i + 6, 6 * i:6 * i + 6] += H00[e]
            b[6 * i:6 * i + 6] -= b0[e]
        if j >= 0:
            H[6 * j:6 * j + 6, 6 * j:6 * j + 6] += H11[e]
            b[6 * j:6 * j + 6] -= b1[e]
        if i >= 0 and j >= 0:
            H[6 * i:6 * i + 6, 6 * j:6 * j + 6] += H01[e]
            H[6 * j:6 * j + 6, 6 * i:6 * i + 6] += H01[e].T
    return H, b


def solve_chol(A, b):
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return False, np.zeros_like(b)
    if not np.isfinite(L).all():
        return False, np.zeros_like(b)
    return True, np.linalg.solve(L.T, np.linalg.solve(L, b))


def solve_lu(A, b):
    try:
        np.linalg.cholesky(A)  # (the accept / reject rule is the factorisation's; the numbers are the LU's)
    except np.linalg.LinAlgError:
        return False, np.zeros_like(b)
    return True, np.linalg.solve(A, b)


# ---- G8 ------------------------------------------------------------------------------------------------------------------------
def update(G, est, x):
    out = est.copy()
    for v in range(G.nv):
        s = int(G.slot[v])
        if s < 0:
            continue
        u = [float(t) for t in x[6 * s:6 * s + 6]]
        if all(t == 0.0 for t in u):
            continue
        out[v] = s3.sim3_oplus(tuple(float(t) for t in est[v]), u)
    return out


# ---- G7 ------------------------------------------------------------------------------------------------------------------------
def optimize(estimates, fixed, edges, meas, iterations=20, reverse=False, lu=False):
    """Returns a dict: est (nv, 8), chi2 (ne,) at est, iterations, trials, accepts (one bool per trial), rhos (the gain ratio of every
    trial), trial_iter (the iteration of every trial), trial_chi ((chi2 before, chi2 of the trial) of every trial), chis (the chi2 the accepted trials reached, the initial one first), est_after
    (the estimates after every iteration: a run of k iterations is the prefix of a longer one)."""
    G = Graph(estimates, fixed, edges, meas)
    est = G.est0.copy()
    out = dict(est=est, chi2=None, iterations=0, trials=0, accepts=[], rhos=[], trial_iter=[], trial_chi=[], chis=[], est_after=[])
    if G.ne == 0 or iterations == 0 or G.nf == 0:
        return out
    solve = solve_lu if lu else solve_chol
    lam, ni = 0.0, 2.0
    n = 6 * G.nf
    for it in range(iterations):
        out["iterations"] += 1
        E, J0, J1 = linearize(G, est)
        c2 = edge_chi2(E)
        current_chi = float(np.cumsum(c2[::-1] if reverse else c2)[-1])
        if it == 0:
            out["chis"].append(current_chi)
        H, b = build_system(G, E, J0, J1, reverse)
        if it == 0:
            lam = 1e-5 * float(np.max(np.abs(np.diag(H)))) if n else 0.0
            ni = 2.0
        rho, qmax = 0.0, 0
        while True:
            A = H.copy()
            A[np.arange(n), np.arange(n)] += lam
            ok2, x = solve(A, b)
            trial = update(G, est, x)
            c2 = edge_chi2(errors(G, trial))
            temp_chi = float(np.cumsum(c2[::-1] if reverse else c2)[-1]) if ok2 else DBL_MAX
            out["trials"] += 1
            scale = float(np.cumsum(x * (lam * x + b))[-1]) + 1e-3
            rho = (current_chi - temp_chi) / scale
            if not ok2:
                rho = -1.0
            out["rhos"].append(rho)
            out["trial_iter"].append(it)
            out["trial_chi"].append((current_chi, temp_chi))
            if rho > 0 and math.isfinite(temp_chi):
                alpha = 1.0 - (2 * rho - 1) ** 3
                alpha = min(alpha, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                current_chi = temp_chi
                est = trial
                out["accepts"].append(True)
                out["chis"].append(current_chi)
            else:
                lam *= ni
                ni *= 2
                out["accepts"].append(False)
                if not math.isfinite(lam):
                    break
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        out["est_after"].append(est)
        if qmax == 10 or rho == 0 or not math.isfinite(lam):
            break
    out["est"] = est
    out["chi2"] = edge_chi2(errors(G, est))
    return out
