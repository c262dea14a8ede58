"""Restatement of Optimizer::OptimizeSim3 (src/Optimizer.cc:464-619) under the rules O1 .. O8 of DESIGN 4.22: the reference for the
device optimiser (orbfe_sim3_optimize, k_sim3opt.hip) and, operation by operation, for the edge model header csrc/sim3_edge_dev.h.

Plain fp64, every operation in evaluation order (numpy rounds each elementwise operation once, no fused multiply-add), vectorised over
the pairs; the estimate is a tuple of Python floats (qx, qy, qz, qw, tx, ty, tz, s).

  O1  fixed scale only: update[6] = 0, so exp has sigma = 0 and the 7x7 system is the 6x6 one.
  O2  model (float R, t) -> double, Eigen's Quaternion(R), g2o's Sim3(r, t, s) normalisation; back through toRotationMatrix, cast to float.
  O3  EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ, chi2 = e . (w e), Huber delta = (double)(float)sqrt(9.210).
  O4  numeric Jacobians: central differences with 1e-9, column = (1 / (2e-9)) (e+ - e-).
  O5  oplus = exp(update) * estimate; small-angle R = I + Omega + Omega^2 / 2 (decision D1), no renormalisation in the product (D2).
  O6  g2o's Levenberg-Marquardt control as oracle/pose_oracle.cpp restates it; chi2() after optimize() = the last computeError that ran.
  O7  the driver: optimize(5), drop pairs with a chi2 > 9.210, fewer than 20 left: return 0 untouched, else optimize(nBad ? 10 : 5),
      inliers = both chi2 <= 9.210.
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
F64 = np.float64
TH = 9.210
DELTA = float(F32(math.sqrt(9.210)))
NUM_DELTA = 1e-9
NUM_SCALE = 1.0 / (2 * NUM_DELTA)
DBL_MAX = 1.7976931348623157e308


# ---- quaternions and the Sim3 group (O2, O5) -------------------------------------------------------------------------------------
def quat_rotate(q, v):
    """Eigen's quaternion-vector product (se3_dev.h quat_rotate); v = (v0, v1, v2), scalars or arrays"""
    qx, qy, qz, qw = q
    ux = qy * v[2] - qz * v[1]
    uy = qz * v[0] - qx * v[2]
    uz = qx * v[1] - qy * v[0]
    ux = ux + ux
    uy = uy + uy
    uz = uz + uz
    return (v[0] + qw * ux + (qy * uz - qz * uy), v[1] + qw * uy + (qz * ux - qx * uz), v[2] + qw * uz + (qx * uy - qy * ux))


def rot_to_quat(R):
    """Eigen's Quaternion(Matrix3): R row-major 3x3 of floats -> (qx, qy, qz, qw)"""
    tr = R[0][0] + R[1][1] + R[2][2]
    q = [0.0] * 4
    if tr > 0:
        t = math.sqrt(tr + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[2][1] - R[1][2]) * t
        q[1] = (R[0][2] - R[2][0]) * t
        q[2] = (R[1][0] - R[0][1]) * t
    else:
        i = 0
        if R[1][1] > R[0][0]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k][j] - R[j][k]) * t
        q[j] = (R[j][i] + R[i][j]) * t
        q[k] = (R[k][i] + R[i][k]) * t
    return tuple(q)


def quat_to_rot(q):
    """Eigen's toRotationMatrix (ba_edge_dev.h quat_to_rot), row-major list of 9"""
    qx, qy, qz, qw = q
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]


def sim3_from_model(model):
    """ConvertSim3G2o: float R, t -> double, Quaternion(R), g2o's Sim3(r, t, s) constructor; s = 1 (O1, O2)"""
    m = [float(v) for v in np.asarray(model, F32).reshape(12)]
    q = list(rot_to_quat([m[0:3], m[3:6], m[6:9]]))
    if q[3] < 0:
        q = [-v for v in q]
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    q = [v / n for v in q]
    return (q[0], q[1], q[2], q[3], m[9], m[10], m[11], 1.0)


def sim3_to_model(est):
    """ConvertG2o2Sim3: toRotationMatrix in double, every entry cast to float; t cast to float"""
    return np.array(quat_to_rot(est[:4]) + list(est[4:7]), F64).astype(F32)


def sim3_map(S, P):
    """s * (r * P) + t"""
    r = quat_rotate(S[:4], P)
    return (S[7] * r[0] + S[4], S[7] * r[1] + S[5], S[7] * r[2] + S[6])


def sim3_inverse(S):
    """(r*, r* * ((-1 / s) * t), 1 / s)"""
    qi = (-S[0], -S[1], -S[2], S[3])
    k = -1.0 / S[7]
    ti = quat_rotate(qi, (k * S[4], k * S[5], k * S[6]))
    return qi + tuple(ti) + (1.0 / S[7],)


def sim3_mul(A, B):
    """r = rA rB, t = sA (rA * tB) + tA, s = sA sB; no renormalisation (D2)"""
    ax, ay, az, aw = A[:4]
    bx, by, bz, bw = B[:4]
    qw = aw * bw - ax * bx - ay * by - az * bz
    qx = aw * bx + ax * bw + ay * bz - az * by
    qy = aw * by + ay * bw + az * bx - ax * bz
    qz = aw * bz + az * bw + ax * by - ay * bx
    rt = quat_rotate(A[:4], B[4:7])
    return (qx, qy, qz, qw, A[7] * rt[0] + A[4], A[7] * rt[1] + A[5], A[7] * rt[2] + A[6], A[7] * B[7])


def sim3_exp(u):
    """g2o's Sim3(Vector7) with sigma = 0 (O1): u = (omega, upsilon); eps = 1e-5"""
    wx, wy, wz = u[0], u[1], u[2]
    theta = math.sqrt(wx * wx + wy * wy + wz * wz)
    Om = [[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]]
    Om2 = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            a = 0.0
            for k in range(3):
                a = a + Om[i][k] * Om[k][j]
            Om2[i][j] = a
    if theta < 0.00001:
        A, B = 0.5, 1.0 / 6.0
        R = [[(1.0 if i == j else 0.0) + Om[i][j] + 0.5 * Om2[i][j] for j in range(3)] for i in range(3)]  # D1
    else:
        st, ct = math.sin(theta), math.cos(theta)
        A = (1 - ct) / (theta * theta)
        B = (theta - st) / (theta * theta * theta)
        R = [[(1.0 if i == j else 0.0) + st / theta * Om[i][j] + A * Om2[i][j] for j in range(3)] for i in range(3)]
    W = [[A * Om[i][j] + B * Om2[i][j] + (1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    t = [W[i][0] * u[3] + W[i][1] * u[4] + W[i][2] * u[5] for i in range(3)]
    return rot_to_quat(R) + (t[0], t[1], t[2], 1.0)


def sim3_oplus(est, u):
    return sim3_mul(sim3_exp(u), est)


# ---- the edges (O3, O4) ----------------------------------------------------------------------------------------------------------
class Problem:
    """the arrays of orbfe_sim3_optimize: pc = cPc, pm = mPc (float32 [n][3]), uv_c, uv_m (float32 [n][2]), info_c, info_m (float64 [n])"""

    def __init__(self, pc, pm, uv_c, uv_m, info_c, info_m, cam):
        pc = np.asarray(pc, F32).reshape(-1, 3).astype(F64)
        pm = np.asarray(pm, F32).reshape(-1, 3).astype(F64)
        self.n = len(pc)
        self.Pc = (pc[:, 0].copy(), pc[:, 1].copy(), pc[:, 2].copy())
        self.Pm = (pm[:, 0].copy(), pm[:, 1].copy(), pm[:, 2].copy())
        self.uvc = np.asarray(uv_c, F32).reshape(-1, 2).astype(F64)
        self.uvm = np.asarray(uv_m, F32).reshape(-1, 2).astype(F64)
        self.wc = np.asarray(info_c, F64).reshape(-1)
        self.wm = np.asarray(info_m, F64).reshape(-1)
        self.fx, self.fy, self.cx, self.cy = (float(F32(v)) for v in cam)


def edge_errors(P, S):
    """both computeError at the estimate S: (n, 4) = e1 (EdgeSim3ProjectXYZ, in pCurr), e2 (EdgeInverseSim3ProjectXYZ, in pMatch)"""
    with np.errstate(all="ignore"):
        p = sim3_map(S, P.Pm)
        e10 = P.uvc[:, 0] - (p[0] / p[2] * P.fx + P.cx)
        e11 = P.uvc[:, 1] - (p[1] / p[2] * P.fy + P.cy)
        p = sim3_map(sim3_inverse(S), P.Pc)
        e20 = P.uvm[:, 0] - (p[0] / p[2] * P.fx + P.cx)
        e21 = P.uvm[:, 1] - (p[1] / p[2] * P.fy + P.cy)
    return np.stack([e10, e11, e20, e21], 1)


def edge_chi2(P, E):
    """(n, 2): e . (w e) as Eigen evaluates it"""
    with np.errstate(all="ignore"):
        c1 = E[:, 0] * (P.wc * E[:, 0]) + E[:, 1] * (P.wc * E[:, 1])
        c2 = E[:, 2] * (P.wm * E[:, 2]) + E[:, 3] * (P.wm * E[:, 3])
    return np.stack([c1, c2], 1)


def huber(c2, delta=DELTA):
    """RobustKernelHuber::robustify: (rho, rho')"""
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(c2)
        big = c2 > dsqr
        rho = np.where(big, 2 * sq * delta - dsqr, c2)
        drho = np.where(big, delta / sq, 1.0)
    return rho, drho


def numeric_jacobian(P, S):
    """(n, 4, 6): rows e1.u, e1.v, e2.u, e2.v; columns omega, upsilon (column 6 is 0, O1)"""
    J = np.empty((P.n, 4, 6), F64)
    for d in range(6):
        u = [0.0] * 6
        u[d] = NUM_DELTA
        ep = edge_errors(P, sim3_oplus(S, u))
        u[d] = -NUM_DELTA
        em = edge_errors(P, sim3_oplus(S, u))
        with np.errstate(all="ignore"):
            J[:, :, d] = NUM_SCALE * (ep - em)
    return J


# ---- the optimiser (O6) ----------------------------------------------------------------------------------------------------------
def _seqsum(terms, reverse):
    t = terms[::-1] if reverse else terms
    return np.cumsum(t, axis=0)[-1] if len(t) else np.zeros(terms.shape[1:], F64)


def build_system(P, S, E, active, reverse=False):
    """constructQuadraticForm of every active edge at S with the errors E: the 21 + 6 sums, added in edge order (pair 0 edge 1, pair 0
    edge 2, pair 1 ...), or in the reverse of it"""
    idx = np.nonzero(active)[0]
    J = numeric_jacobian(P, S)[idx]
    Ea = E[idx]
    chi = edge_chi2(P, E)[idx]
    terms = np.empty((len(idx), 2, 27), F64)
    with np.errstate(all="ignore"):
        for ed, w in ((0, P.wc[idx]), (1, P.wm[idx])):
            _, r1 = huber(chi[:, ed])
            J0, J1 = J[:, 2 * ed, :], J[:, 2 * ed + 1, :]
            e0, e1 = Ea[:, 2 * ed], Ea[:, 2 * ed + 1]
            k = 0
            for a in range(6):
                terms[:, ed, 21 + a] = -(r1 * (J0[:, a] * (w * e0) + J1[:, a] * (w * e1)))
                for c in range(a, 6):
                    terms[:, ed, k] = J0[:, a] * (r1 * w) * J0[:, c] + J1[:, a] * (r1 * w) * J1[:, c]
                    k += 1
    tot = _seqsum(terms.reshape(-1, 27), reverse)
    H = np.zeros((6, 6), F64)
    k = 0
    for a in range(6):
        for c in range(a, 6):
            H[a, c] = H[c, a] = tot[k]
            k += 1
    return H, tot[21:].copy()


def solve6(A, b):
    """pose_oracle.cpp's solve6: plain Cholesky; (ok, x) with x = 0 where the factorisation fails"""
    L = [[0.0] * 6 for _ in range(6)]
    x = [0.0] * 6
    for i in range(6):
        for j in range(i + 1):
            s = float(A[i][j])
            for k in range(j):
                s -= L[i][k] * L[j][k]
            if i == j:
                if not s > 0:
                    return False, x
                L[i][i] = math.sqrt(s)
            else:
                L[i][j] = s / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        s = float(b[i])
        for k in range(i):
            s -= L[i][k] * y[k]
        y[i] = s / L[i][i]
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s -= L[k][i] * x[k]
        x[i] = s / L[i][i]
    return True, x


class State:
    def __init__(self, P, S):
        self.S = S
        self.E = np.zeros((P.n, 4), F64)        # the _error of every edge: what the last computeError left
        self.active = np.ones(P.n, bool)
        self.iterations = 0
        self.trials = 0


def _active_chi(P, st, reverse):
    """computeActiveErrors + activeRobustChi2"""
    E = edge_errors(P, st.S)
    st.E[st.active] = E[st.active]
    rho, _ = huber(edge_chi2(P, st.E)[st.active])
    return float(_seqsum(rho.reshape(-1, 1), reverse)[0])


def optimize(P, st, iterations, reverse=False):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg on the one vertex"""
    if not st.active.any():
        return
    lam, ni = 0.0, 2.0
    for it in range(iterations):
        current_chi = _active_chi(P, st, reverse)
        H, b = build_system(P, st.S, st.E, st.active, reverse)
        if it == 0:
            md = 0.0
            for j in range(6):
                md = max(abs(float(H[j, j])), md)
            lam = 1e-5 * md
            ni = 2.0
        st.iterations += 1
        rho, qmax = 0.0, 0
        while True:
            backup = st.S
            Hl = H.copy()
            for j in range(6):
                Hl[j, j] += lam
            ok2, x = solve6(Hl, b)
            st.S = sim3_oplus(st.S, x)
            temp_chi = _active_chi(P, st, reverse)
            st.trials += 1
            if not ok2:
                temp_chi = DBL_MAX
            rho = current_chi - temp_chi
            scale = 0.0
            for j in range(6):
                scale += x[j] * (lam * x[j] + float(b[j]))
            scale += 1e-3
            rho /= scale
            if rho > 0 and math.isfinite(temp_chi):
                alpha = 1.0 - (2 * rho - 1) ** 3
                alpha = min(alpha, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                current_chi = temp_chi
            else:
                lam *= ni
                ni *= 2
                st.S = backup
                if not math.isfinite(lam):
                    break
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0 or not math.isfinite(lam):
            break


# ---- the driver (O7) -------------------------------------------------------------------------------------------------------------
def optimize_sim3(pc, pm, uv_c, uv_m, info_c, info_m, cam, model, reverse=False):
    """Optimizer::OptimizeSim3 from the point where the graph is built.  Returns a dict: n_inliers, model (float32[12]), flags (uint8
    [n]: which pairs stay in the list), est (the final estimate, 8 doubles; the start estimate on the early return), branch ('short',
    'few', 'ten', 'five'), chi2_a / chi2_b (the chi2 the two classifications read), n_bad."""
    P = Problem(pc, pm, uv_c, uv_m, info_c, info_m, cam)
    model = np.asarray(model, F32).reshape(12).copy()
    n = P.n
    est0 = sim3_from_model(model)
    out = dict(n_inliers=0, model=model, flags=np.ones(n, np.uint8), est=np.array(est0, F64), branch="short", chi2_a=None, chi2_b=None,
               n_bad=0, iterations=0, trials=0)
    if n < 20:
        return out
    st = State(P, est0)
    optimize(P, st, 5, reverse)
    chi_a = edge_chi2(P, st.E)
    with np.errstate(invalid="ignore"):
        bad = (chi_a[:, 0] > TH) | (chi_a[:, 1] > TH)
    n_bad = int(bad.sum())
    out.update(chi2_a=chi_a, n_bad=n_bad, iterations=st.iterations, trials=st.trials)
    if n - n_bad < 20:
        out["branch"] = "few"
        return out
    st.active = ~bad
    optimize(P, st, 10 if n_bad else 5, reverse)
    chi_b = edge_chi2(P, st.E)
    with np.errstate(invalid="ignore"):
        inl = st.active & (chi_b[:, 0] <= TH) & (chi_b[:, 1] <= TH)
    out.update(n_inliers=int(inl.sum()), model=sim3_to_model(st.S), flags=inl.astype(np.uint8), est=np.array(st.S, F64),
               branch="ten" if n_bad else "five", chi2_b=np.where(st.active[:, None], chi_b, np.nan), iterations=st.iterations,
               trials=st.trials)
    return out
