"""Restatement of PnPSolver + Ransac<PnPRet> (src/PnPSolver.cc, include/ORB_SLAM2/Ransac.hpp) under the numerical decisions of
DESIGN 4.16: the reference for the device solver (orbfe_pnp_*, k_pnp.hip), which must equal it bit for bit.

  * EPnP runs in fp64 without contraction.  Every sum is sequential in list order and starts from its first term; numpy elementwise
    operations are exact per element, so the hypotheses are vectorised along a leading axis and every reduction is an explicit loop
    (np.add.accumulate is sequential).
  * Symmetric eigen-decompositions: cyclic Jacobi (jacobi()), then a selection sort to descending eigenvalues and the P7 sign rule
    (each eigenvector's largest-|component|, ties to the lower index, is made positive).
  * 3x3 solves: Cramer's rule (OpenCV's DECOMP_LU path for 3 rows); a zero determinant gives alphas 0 (cv::solve's zeroed output).
  * DECOMP_SVD solves: min-norm pseudo-inverse from the eigen-decomposition of the symmetric system; eigenvalues <= rel * max are cut.
  * The pose is rounded to float, and the inlier test runs in float in the reference's order (Rcw * X + tcw as k_guided.hip states it).
  * Sampling: the process-wide minstd_rand0 and libstdc++'s uniform_int_distribution<size_t> scaling path (P6).
"""
from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
MAX_SWEEPS = 50           # Jacobi sweeps at most (a NaN input runs them all)
NEGLIGIBLE_SWEEP = 4      # from this sweep on an off-diagonal that cannot change its diagonals is set to 0
PINV_REL_BETA = 1e-24     # betas: eigenvalues of L4^T L4 (squared singular values of L4) <= 1e-24 * max are cut
PINV_REL_GN = 1e-12       # Gauss-Newton: eigenvalues of J J^T (its singular values) <= 1e-12 * max are cut
ICP_REL = 1e-12           # ICP: singular values <= 1e-12 * the largest are rank-deficient
DEGENERATE_EIG = 1e-3     # computeCtlPoint's eigenvalue floor
GN_ITERS = 5
QNAN32 = np.uint32(0x7FC00000)
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
JI = [[1, 5, 6, 7], [5, 2, 8, 9], [6, 8, 3, 10], [7, 9, 10, 4]]

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.logf.restype, _libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]
_libm.log.restype, _libm.log.argtypes = ctypes.c_double, [ctypes.c_double]
_libm.pow.restype, _libm.pow.argtypes = ctypes.c_double, [ctypes.c_double, ctypes.c_double]


# ---- engine (P6) -----------------------------------------------------------------------------------------------------------------
class Engine:
    """std::default_random_engine (minstd_rand0), default seed 1; `state` is its x"""

    def __init__(self, state=1):
        self.state = int(state)

    def __call__(self):
        self.state = self.state * 16807 % 2147483647
        return self.state


def uniform_int(eng, n):
    """uniform_int_distribution<size_t>(0, n - 1)(eng), libstdc++'s scaling / rejection path (minstd's range is not 2^32 - 1)"""
    urngrange, urange = 2147483646 - 1, n - 1
    if urngrange > urange:
        uerange = urange + 1
        scaling = urngrange // uerange
        past = uerange * scaling
        while True:
            r = eng() - 1
            if r < past:
                return r // scaling
    assert urngrange == urange, "ranges above minstd's are not used"
    return eng() - 1


def random_sample(eng, n, k=4):
    out = []
    while len(out) != k:
        r = uniform_int(eng, n)
        if r not in out:
            out.append(r)
    return out


# ---- setRansacParams -------------------------------------------------------------------------------------------------------------
def _cv_round(x):
    """cvRound(double) on x86-64: cvtsd2si, nearest-even; NaN / out of range -> INT_MIN"""
    if not np.isfinite(x) or not (-2147483648.5 < x < 2147483647.5):
        return -2147483648
    r = round(x)  # Python rounds half to even
    return int(r) if -2147483648 <= r <= 2147483647 else -2147483648


def ransac_params(N, min_set=4, max_iterations=100, ratio=0.4, prob=0.99):
    """(mnMinInlier, mnMaxIterations) of setRansacParams() for N points, with its float / double mix"""
    min_inlier = int(max(F32(min_set), F32(N) * F32(ratio)))
    with np.errstate(all="ignore"):
        r = F32(min_inlier) / F32(N)
    if r >= 1:
        return min_inlier, 0
    num = float(_libm.logf(float(F32(1) - F32(prob))))
    den = _libm.log(1.0 - _libm.pow(float(r), float(min_set)))
    with np.errstate(all="ignore"):
        q = np.float64(num) / np.float64(den)
    return min_inlier, min(max_iterations, _cv_round(float(q)))


# ---- linear algebra --------------------------------------------------------------------------------------------------------------
def seqsum(x, axis):
    """sequential sum along axis, starting from the first term"""
    return np.take(np.add.accumulate(x, axis=axis), -1, axis=axis)


def jacobi(a):
    """cyclic Jacobi on a batch of symmetric matrices (H, n, n): (eigenvalues (H, n), eigenvectors as columns (H, n, n)), unsorted.
    A sweep starts only while some off-diagonal is non-zero; pairs (p, q) in row-major order; a zero a_pq is skipped; from sweep 4 on an
    a_pq with |a_pp| + 100|a_pq| == |a_pp| and the same for a_qq is set to 0; else the trig-free rotation below."""
    a = np.array(a, np.float64, copy=True)
    H, n, _ = a.shape
    V = np.broadcast_to(np.eye(n), a.shape).copy()
    done = np.zeros(H, bool)
    with np.errstate(all="ignore"):
        for sweep in range(MAX_SWEEPS):
            off = np.zeros(H, bool)
            for p in range(n - 1):
                for q in range(p + 1, n):
                    off |= a[:, p, q] != 0
            done |= ~off
            if done.all():
                break
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = a[:, p, q]
                    act = ~done & (apq != 0)
                    if sweep >= NEGLIGIBLE_SWEEP:
                        g = 100.0 * np.abs(apq)
                        app, aqq = np.abs(a[:, p, p]), np.abs(a[:, q, q])
                        negl = act & (app + g == app) & (aqq + g == aqq)
                        a[negl, p, q] = 0.0
                        a[negl, q, p] = 0.0
                        act &= ~negl
                    i = np.nonzero(act)[0]
                    if len(i) == 0:
                        continue
                    A = a[i]
                    Vv = V[i]
                    apq, app, aqq = A[:, p, q], A[:, p, p], A[:, q, q]
                    theta = (aqq - app) / (2.0 * apq)
                    t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    t = np.where(theta < 0, -t, t)
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    tau = s / (1.0 + c)
                    h = t * apq
                    A[:, p, p] = app - h
                    A[:, q, q] = aqq + h
                    A[:, p, q] = 0.0
                    A[:, q, p] = 0.0
                    rs = [r for r in range(n) if r != p and r != q]
                    gg, hh = A[:, rs, p].copy(), A[:, rs, q].copy()
                    sc, tc = s[:, None], tau[:, None]
                    np_ = gg - sc * (hh + gg * tc)
                    nq_ = hh + sc * (gg - hh * tc)
                    A[:, rs, p] = np_
                    A[:, p, rs] = np_
                    A[:, rs, q] = nq_
                    A[:, q, rs] = nq_
                    gg, hh = Vv[:, :, p].copy(), Vv[:, :, q].copy()
                    Vv[:, :, p] = gg - sc * (hh + gg * tc)
                    Vv[:, :, q] = hh + sc * (gg - hh * tc)
                    a[i] = A
                    V[i] = Vv
    return np.array([np.diagonal(x) for x in a]).reshape(H, n), V


def eig_sorted(a):
    """jacobi, then a selection sort to descending eigenvalues (position p takes the first strictly larger one after it, swapped in),
    then the P7 sign rule on every eigenvector"""
    w, V = jacobi(a)
    H, n = w.shape
    ar = np.arange(H)
    for p in range(n - 1):
        best = np.full(H, p)
        bv = w[:, p].copy()
        for q in range(p + 1, n):
            m = w[:, q] > bv
            best = np.where(m, q, best)
            bv = np.where(m, w[:, q], bv)
        wp, Vp = w[:, p].copy(), V[:, :, p].copy()
        w[:, p] = w[ar, best]
        V[:, :, p] = V[ar, :, best]
        w[ar, best] = wp
        V[ar, :, best] = Vp
    for k in range(n):
        bi = np.zeros(H, int)
        bv = np.abs(V[:, 0, k])
        for j in range(1, n):
            m = np.abs(V[:, j, k]) > bv
            bi = np.where(m, j, bi)
            bv = np.where(m, np.abs(V[:, j, k]), bv)
        neg = V[ar, bi, k] < 0
        V[neg, :, k] = -V[neg, :, k]
    return w, V


def pinv_sym4(N, g, rel):
    """min-norm solve of the symmetric 4x4 system N x = g: x = sum over eigenpairs with lam > 0 and lam > rel * max(lam) of
    (v . g) / lam * v, x starting at 0, eigenpairs in Jacobi's order"""
    lam, V = jacobi(N)
    lmax = lam[:, 0].copy()
    for k in range(1, 4):
        lmax = np.where(lam[:, k] > lmax, lam[:, k], lmax)
    tol = lmax * rel
    x = np.zeros_like(g)
    with np.errstate(all="ignore"):
        for k in range(4):
            use = (lam[:, k] > 0) & (lam[:, k] > tol)
            proj = V[:, 0, k] * g[:, 0] + V[:, 1, k] * g[:, 1] + V[:, 2, k] * g[:, 2] + V[:, 3, k] * g[:, 3]
            coef = proj / lam[:, k]
            for j in range(4):
                x[:, j] = np.where(use, x[:, j] + coef * V[:, j, k], x[:, j])
    return x


def _dot3(x, y):
    return x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1] + x[..., 2] * y[..., 2]


def _fullbeta(b):
    b0, b1, b2, b3 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return np.stack([b0 * b0, b1 * b1, b2 * b2, b3 * b3, b0 * b1, b0 * b2, b0 * b3, b1 * b2, b1 * b3, b2 * b3], 1)


def _residual(L, fb, rho):
    return seqsum(L * fb[:, None, :], 2) - rho


def epnp(P, uv, cam):
    """PnPSolver::modelFunc on a batch: P (H, n, 3) and uv (H, n, 2) (float values), cam (fx, fy, cx, cy) floats.
    Returns (degenerate (H,) bool, R (H, 9) float32, t (H, 3) float32); a degenerate row's pose is meaningless."""
    P = np.asarray(P, np.float64)
    uv = np.asarray(uv, np.float64)
    H, n, _ = P.shape
    fx, fy, cx, cy = (float(F32(v)) for v in cam)
    with np.errstate(all="ignore"):
        # 1. control points: centroid + PCA axes
        c = seqsum(P, 1) / float(n)
        d = P - c[:, None, :]
        A = np.empty((H, 3, 3))
        for i, j in [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]:
            A[:, i, j] = A[:, j, i] = seqsum(d[:, :, i] * d[:, :, j], 1)
        lam, E = eig_sorted(A)
        degen = (lam[:, 0] < DEGENERATE_EIG) | (lam[:, 1] < DEGENERATE_EIG) | (lam[:, 2] < DEGENERATE_EIG)
        ctl = np.empty((H, 4, 3))
        ctl[:, 0] = c
        for k in range(3):
            s = np.sqrt(lam[:, k] / float(n))
            ctl[:, k + 1] = c + s[:, None] * E[:, :, k]
        # 2. alphas (Cramer; B[r][k] = ctl[k + 1][r] - c[r])
        B = ctl[:, 1:, :] - c[:, None, :]
        m00, m01, m02 = B[:, 0, 0], B[:, 1, 0], B[:, 2, 0]
        m10, m11, m12 = B[:, 0, 1], B[:, 1, 1], B[:, 2, 1]
        m20, m21, m22 = B[:, 0, 2], B[:, 1, 2], B[:, 2, 2]
        D = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20)
        invD = (1.0 / D)[:, None]
        m00, m01, m02, m10, m11, m12, m20, m21, m22 = (x[:, None] for x in (m00, m01, m02, m10, m11, m12, m20, m21, m22))
        b0, b1, b2 = d[:, :, 0], d[:, :, 1], d[:, :, 2]
        a1 = invD * (b0 * (m11 * m22 - m12 * m21) - m01 * (b1 * m22 - m12 * b2) + m02 * (b1 * m21 - m11 * b2))
        a2 = invD * (m00 * (b1 * m22 - m12 * b2) - b0 * (m10 * m22 - m12 * m20) + m02 * (m10 * b2 - b1 * m20))
        a3 = invD * (m00 * (m11 * b2 - b1 * m21) - m01 * (m10 * b2 - b1 * m20) + b0 * (m10 * m21 - m11 * m20))
        z = (D == 0)[:, None]
        a1, a2, a3 = np.where(z, 0.0, a1), np.where(z, 0.0, a2), np.where(z, 0.0, a3)
        a0 = 1.0 - a1 - a2 - a3
        alpha = np.stack([a0, a1, a2, a3], 2)  # (H, n, 4)
        # 3. M^T M, rows 2i / 2i + 1 of M interleaved in list order
        du, dv = cx - uv[:, :, 0], cy - uv[:, :, 1]
        r0 = np.zeros((H, n, 12))
        r1 = np.zeros((H, n, 12))
        for j in range(4):
            r0[:, :, 3 * j] = alpha[:, :, j] * fx
            r0[:, :, 3 * j + 2] = alpha[:, :, j] * du
            r1[:, :, 3 * j + 1] = alpha[:, :, j] * fy
            r1[:, :, 3 * j + 2] = alpha[:, :, j] * dv
        MtM = np.empty((H, 12, 12))
        for a in range(12):
            for b in range(a, 12):
                t = np.empty((H, 2 * n))
                t[:, 0::2] = r0[:, :, a] * r0[:, :, b]
                t[:, 1::2] = r1[:, :, a] * r1[:, :, b]
                MtM[:, a, b] = MtM[:, b, a] = seqsum(t, 1)
        _, E12 = eig_sorted(MtM)
        v = np.stack([E12[:, :, 11 - k].reshape(H, 4, 3) for k in range(4)], 1)  # v[:, k, j] = point j of vMREVec[k]
        # 4. L, rho, betas
        L = np.empty((H, 6, 10))
        rho = np.empty((H, 6))
        for row, (a, b) in enumerate(PAIRS):
            x = [v[:, k, a] - v[:, k, b] for k in range(4)]
            L[:, row, 0], L[:, row, 1], L[:, row, 2], L[:, row, 3] = (_dot3(x[k], x[k]) for k in range(4))
            L[:, row, 4] = 2.0 * _dot3(x[0], x[1])
            L[:, row, 5] = 2.0 * _dot3(x[0], x[2])
            L[:, row, 6] = 2.0 * _dot3(x[0], x[3])
            L[:, row, 7] = 2.0 * _dot3(x[1], x[2])
            L[:, row, 8] = 2.0 * _dot3(x[1], x[3])
            L[:, row, 9] = 2.0 * _dot3(x[2], x[3])
            dd = ctl[:, a] - ctl[:, b]
            rho[:, row] = _dot3(dd, dd)
        L4 = L[:, :, [0, 4, 5, 6]]
        N4 = np.empty((H, 4, 4))
        for i in range(4):
            for j in range(4):
                N4[:, i, j] = seqsum(L4[:, :, i] * L4[:, :, j], 1)
        g4 = np.stack([seqsum(L4[:, :, i] * rho, 1) for i in range(4)], 1)
        beta = pinv_sym4(N4, g4, PINV_REL_BETA)
        neg = beta[:, 0] < 0
        beta[neg] = -beta[neg]
        b1 = np.sqrt(beta[:, 0])
        beta[:, 0] = b1
        beta[:, 1] = beta[:, 1] / b1
        beta[:, 2] = beta[:, 2] / b1
        beta[:, 3] = beta[:, 3] / b1
        # 5. Gauss-Newton
        old = np.full(H, FLT_MAX)
        active = np.ones(H, bool)
        for _ in range(GN_ITERS):
            fb = _fullbeta(beta)
            J = np.empty((H, 4, 6))
            for row in range(4):
                for col in range(6):
                    terms = [(2.0 * L[:, col, JI[row][i] - 1]) * beta[:, i] if i == row else L[:, col, JI[row][i] - 1] * beta[:, i]
                             for i in range(4)]
                    J[:, row, col] = ((terms[0] + terms[1]) + terms[2]) + terms[3]
            r = _residual(L, fb, rho)
            Hm = np.empty((H, 4, 4))
            for i in range(4):
                for j in range(4):
                    Hm[:, i, j] = seqsum(J[:, i, :] * J[:, j, :], 1)
            g = np.stack([-seqsum(J[:, i, :] * r, 1) for i in range(4)], 1)
            delta = pinv_sym4(Hm, g, PINV_REL_GN)
            nrm = np.sqrt(((delta[:, 0] * delta[:, 0] + delta[:, 1] * delta[:, 1]) + delta[:, 2] * delta[:, 2]) + delta[:, 3] * delta[:, 3])
            active &= ~(nrm < 1e-4)
            beta = np.where(active[:, None], beta + delta, beta)
            r2 = _residual(L, _fullbeta(beta), rho)
            err = np.sqrt(seqsum(r2 * r2, 1))
            undo = active & (err > old)
            beta = np.where(undo[:, None], beta - delta, beta)
            active &= ~undo
            old = np.where(active, err, old)
        # 6. camera control points
        Cc = ((beta[:, 0, None, None] * v[:, 0] + beta[:, 1, None, None] * v[:, 1]) + beta[:, 2, None, None] * v[:, 2]) + \
            beta[:, 3, None, None] * v[:, 3]
        # 7. ICP
        cW = (((ctl[:, 0] + ctl[:, 1]) + ctl[:, 2]) + ctl[:, 3]) / 4.0
        cC = (((Cc[:, 0] + Cc[:, 1]) + Cc[:, 2]) + Cc[:, 3]) / 4.0
        Aw, Bc = ctl - cW[:, None], Cc - cC[:, None]
        Hx = np.empty((H, 3, 3))
        for i in range(3):
            for j in range(3):
                Hx[:, i, j] = seqsum(Bc[:, :, i] * Aw[:, :, j], 1)
        S = np.empty((H, 3, 3))
        for i in range(3):
            for j in range(3):
                S[:, i, j] = seqsum(Hx[:, :, i] * Hx[:, :, j], 1)
        lam3, V3 = eig_sorted(S)
        sig = np.where(lam3 > 0, np.sqrt(lam3), 0.0)
        U = np.zeros((H, 3, 3))
        ok = [sig[:, 0] > 0]
        ok += [ok[0] & (sig[:, k] > sig[:, 0] * ICP_REL) for k in (1, 2)]
        for k in range(3):
            hv = Hx[:, :, 0] * V3[:, None, 0, k] + Hx[:, :, 1] * V3[:, None, 1, k] + Hx[:, :, 2] * V3[:, None, 2, k]
            U[:, :, k] = np.where(ok[k][:, None], hv / sig[:, k, None], 0.0)
        u0, u1 = U[:, :, 0], U[:, :, 1]
        cross = np.stack([u0[:, 1] * u1[:, 2] - u0[:, 2] * u1[:, 1], u0[:, 2] * u1[:, 0] - u0[:, 0] * u1[:, 2],
                          u0[:, 0] * u1[:, 1] - u0[:, 1] * u1[:, 0]], 1)
        U[:, :, 2] = np.where((~ok[2] & ok[1])[:, None], cross, U[:, :, 2])
        R = (U[:, :, 0, None] * V3[:, None, :, 0] + U[:, :, 1, None] * V3[:, None, :, 1]) + U[:, :, 2, None] * V3[:, None, :, 2]
        det = (((((R[:, 0, 0] * R[:, 1, 1]) * R[:, 2, 2] + (R[:, 0, 1] * R[:, 1, 2]) * R[:, 2, 0]) + (R[:, 0, 2] * R[:, 1, 0]) * R[:, 2, 1])
                - (R[:, 0, 2] * R[:, 1, 1]) * R[:, 2, 0]) - (R[:, 0, 1] * R[:, 1, 0]) * R[:, 2, 2]) - (R[:, 0, 0] * R[:, 1, 2]) * R[:, 2, 1]
        flip = det < 0
        R[flip, 2, :] = -R[flip, 2, :]
        t = cC - ((R[:, :, 0] * cW[:, None, 0] + R[:, :, 1] * cW[:, None, 1]) + R[:, :, 2] * cW[:, None, 2])
    return degen, to_f32(R.reshape(H, 9)), to_f32(t)


def to_f32(x):
    """round to float, NaN made the canonical quiet NaN"""
    y = np.asarray(x, np.float64).astype(np.float32)
    y.view(np.uint32)[np.isnan(y)] = QNAN32
    return y


def check_inliers(xyz, uv, thr, cam, R, t):
    """PnPSolver::checkInliers in float for a batch of poses R (H, 9), t (H, 3): (H, N) bool"""
    R = np.asarray(R, F32)
    t = np.asarray(t, F32)
    X = np.asarray(xyz, F32)
    fx, fy, cx, cy = (F32(v) for v in cam)
    with np.errstate(all="ignore"):
        pc = []
        for r in range(3):
            s = (R[:, 3 * r, None] * X[None, :, 0] + R[:, 3 * r + 1, None] * X[None, :, 1]) + R[:, 3 * r + 2, None] * X[None, :, 2]
            pc.append((s.astype(np.float64) + t[:, r, None].astype(np.float64)).astype(F32))
        u = pc[0] / pc[2] * fx + cx
        v = pc[1] / pc[2] * fy + cy
        du = uv[None, :, 0].astype(F32) - u
        dv = uv[None, :, 1].astype(F32) - v
        err = du * du + dv * dv
        return err < np.asarray(thr, F32)[None, :]


def thresholds(octave, level_sigma2):
    """mvfErrors: (float)(5.991 * Frame::getScaledFactor2(octave))"""
    s2 = np.asarray(level_sigma2, F32)
    return np.array([F32(5.991 * float(s2[o])) for o in np.asarray(octave)], F32)


# ---- Ransac<PnPRet> --------------------------------------------------------------------------------------------------------------
class Solver:
    """one PnPSolver: create() + iterate() with the reference's state (P1-P6); the pose is None (empty Mats) or (R f32[9], t f32[3])"""

    def __init__(self, xyz, uv, octave, level_sigma2, cam, params=(4, 100, 0.4, 0.99)):
        self.xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
        self.uv = np.ascontiguousarray(uv, F32).reshape(-1, 2)
        self.thr = thresholds(octave, level_sigma2)
        self.cam = tuple(float(F32(v)) for v in cam)
        self.N = len(self.xyz)
        self.min_set = params[0]
        self.min_inlier, self.max_it = ransac_params(self.N, *params)
        self.cur = 0
        self.best = 0
        self.best_pose = None
        self.best_list = []
        self.n_hyp = 0  # hypotheses evaluated (statistics)

    def model(self, idx):
        idx = np.asarray(idx, np.int64)
        deg, R, t = epnp(self.xyz[idx][None].astype(np.float64), self.uv[idx][None].astype(np.float64), self.cam)
        return None if deg[0] else (R[0], t[0])

    def check(self, pose):
        m = check_inliers(self.xyz, self.uv, self.thr, self.cam, pose[0][None], pose[1][None])[0]
        return np.nonzero(m)[0].tolist()

    def iterate(self, eng, n, pose=None, inliers=()):
        """Ransac::iterate(n, pose, bNoMore, inliers): returns (ret, no_more, pose, inliers); no_more is only ever set"""
        lst = list(inliers)
        if self.N < self.min_set:
            return False, True, pose, lst
        k = max(0, min(n, self.max_it - self.cur))
        # the draws of every hypothesis this call may try, and the engine after each (a successful refine ends the call early)
        probe = Engine(eng.state)
        samples, after = [], []
        for _ in range(k):
            samples.append(random_sample(probe, self.N, self.min_set))
            after.append(probe.state)
        if k:
            deg, R, t = epnp(self.xyz[np.array(samples)].astype(np.float64), self.uv[np.array(samples)].astype(np.float64), self.cam)
            masks = check_inliers(self.xyz, self.uv, self.thr, self.cam, R, t)
            self.n_hyp += k
        last = None  # the inliers of modelRet as it stands (P2: a degenerate sample recounts it)
        if pose is not None:
            last = self.check(pose)
        for h in range(k):
            if not deg[h]:
                pose = (R[h], t[h])
                last = np.nonzero(masks[h])[0].tolist()
            if pose is not None:
                lst += last
                cnt = len(last)
                if cnt > self.min_inlier:
                    if cnt > self.best:
                        self.best, self.best_pose, self.best_list = cnt, pose, list(lst)
                    rp = self.model(lst)
                    if rp is not None:
                        pose = rp
                    lst = self.check(pose)
                    last = list(lst)
                    if len(lst) > self.min_inlier:
                        eng.state = after[h]  # P3: budget not spent
                        return True, False, pose, lst
            self.cur += 1
        if k:
            eng.state = after[-1]
        no_more = self.cur >= self.max_it
        if self.best == 0:
            return False, no_more, pose, lst
        return True, no_more, self.best_pose, list(self.best_list)


def tracking_loop(iterate, n_problems, n=5, accept=None):
    """Tracking::trackReLocalize's step 3 over `iterate(problem, n) -> (ret, no_more, pose, inliers)`; `accept(problem, pose, inliers)`
    stands for OptimizePoseOnly / searchByProjection (default: never).  Returns the list of (problem, result) in call order."""
    discard = [False] * n_problems
    left = n_problems
    log = []
    while left:
        for p in range(n_problems):
            if discard[p]:
                continue
            r = iterate(p, n)
            log.append((p, r))
            if r[1]:
                discard[p] = True
                left -= 1
            if r[0] and accept is not None and accept(p, r[2], r[3]):
                return log
    return log


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
CAM = (517.3, 516.5, 318.6, 255.3)
SIGMA2 = np.array([1.2 ** (2 * i) for i in range(8)], F32)


def rot(rng, scale=0.3):
    w = rng.normal(size=3) * scale
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def scene(rng, N, outlier=0.0, noise=0.5, degenerate=None, cam=CAM):
    """N map points in front of a random camera, their projections (+ noise), a share of outliers, octaves 0..7.
    degenerate: None, 'collinear' (half the points on one line) or 'repeat' (a quarter repeat other points).  Returns
    (xyz f32, uv f32, octave i32, R_true, t_true)"""
    R = rot(rng)
    t = rng.normal(size=3) * 0.5
    pc = np.stack([rng.uniform(-2, 2, N), rng.uniform(-1.5, 1.5, N), rng.uniform(2, 8, N)], 1)
    X = (pc - t) @ R  # R^T (pc - t)
    if degenerate == "collinear" and N:
        m = N // 2
        a, b = X[0], X[0] + rng.normal(size=3)
        s = rng.uniform(0, 1, m)
        X[:m] = a + s[:, None] * (b - a)
    elif degenerate == "repeat" and N > 1:
        m = max(1, N // 4)
        X[:m] = X[rng.integers(0, N, m)]
    pc = X @ R.T + t
    fx, fy, cx, cy = cam
    uv = np.stack([pc[:, 0] / pc[:, 2] * fx + cx, pc[:, 1] / pc[:, 2] * fy + cy], 1) + rng.normal(size=(N, 2)) * noise
    out = rng.uniform(0, 1, N) < outlier
    uv[out] = np.stack([rng.uniform(0, 640, out.sum()), rng.uniform(0, 480, out.sum())], 1)
    return X.astype(F32), uv.astype(F32), rng.integers(0, 8, N).astype(np.int32), R, t
