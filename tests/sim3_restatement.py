"""Restatement of Sim3Solver + Ransac<Sim3Ret> (src/Sim3Solver.cc, include/ORB_SLAM2/Sim3Solver.h, Ransac.hpp) under the numerical
decisions of DESIGN 4.21: the reference for the device solver (orbfe_sim3_*, k_sim3.hip), which must equal it bit for bit.

  * Everything is float as the reference's CV_32F Mats are, except where OpenCV itself goes through double: `A x + t` and
    `Oq - s R Op` are gemm's `(float)(alpha * (double)sum + (double)t)` with the sum in float left to right (matcher_ext._affine),
    `Mat / n` multiplies by `1.0 / n` in double, `std::pow(float, 2)` is double.
  * cv::eigen of the 4x4 N: pnp_restatement.jacobi on N promoted to double; the largest eigenvalue (first strictly larger wins), its
    eigenvector cast to float as (w, x, y, z).  The sign of the eigenvector cancels in R.
  * Eigen's Quaternionf::normalize and toRotationMatrix in float.
  * The model's NaNs are made the canonical quiet NaN (as pnp_restatement.to_f32 does).
  * Sampling: Ransac<Sim3Ret>'s own minstd_rand0 (S7), three distinct indices per draw.
"""
from __future__ import annotations

import numpy as np

from pnp_restatement import CAM, SIGMA2, Engine, jacobi, random_sample, ransac_params, rot, seqsum, uniform_int  # noqa: F401

F32 = np.float32
F64 = np.float64
QNAN32 = np.uint32(0x7FC00000)
MIN_SET = 3


# ---- float pieces ----------------------------------------------------------------------------------------------------------------
def _row3(a0, a1, a2, x0, x1, x2):
    """(a0 x0 + a1 x1) + a2 x2 in float"""
    return (a0 * x0 + a1 * x1) + a2 * x2


def affine(alpha, R, X, t):
    """(float)(alpha * (double)(R X) + (double)t): R (..., 9), X (..., 3), t (..., 3), all float32, broadcast; alpha a float"""
    out = []
    for r in range(3):
        s = _row3(R[..., 3 * r], R[..., 3 * r + 1], R[..., 3 * r + 2], X[..., 0], X[..., 1], X[..., 2])
        out.append((F64(alpha) * s.astype(F64) + t[..., r].astype(F64)).astype(F32))
    return np.stack(np.broadcast_arrays(*out), -1)


def project(X, cam):
    """Camera::project in float: x = X / Z, u = fx * x + cx"""
    fx, fy, cx, cy = (F32(v) for v in cam)
    with np.errstate(all="ignore"):
        x = X[..., 0] / X[..., 2]
        y = X[..., 1] / X[..., 2]
        return np.stack([fx * x + cx, fy * y + cy], -1)


def canon(x):
    y = np.array(x, F32, copy=True)
    y.view(np.uint32)[np.isnan(y)] = QNAN32
    return y


def thresholds(octave, level_sigma2):
    """mvfErrorsP / Q: (float)(9.210 * KeyFrame::getScaledFactor2(octave))"""
    s2 = np.asarray(level_sigma2, F32)
    return np.array([F32(9.210 * float(s2[o])) for o in np.asarray(octave)], F32)


# ---- modelFunc (Horn) ------------------------------------------------------------------------------------------------------------
def model_func(P, Q):
    """Sim3Solver::modelFunc with the scale fixed, on a batch: P, Q (H, n, 3) float32 -> model (H, 12) float32 (Rqp row-major, tqp)"""
    P = np.asarray(P, F32)
    Q = np.asarray(Q, F32)
    H, n, _ = P.shape
    with np.errstate(all="ignore"):
        inv_n = F64(1.0) / F64(F32(n))
        zero = np.zeros((H, 1, 3), F32)
        Op = (seqsum(np.concatenate([zero, P], 1), 1).astype(F64) * inv_n).astype(F32)   # sums start from 0
        Oq = (seqsum(np.concatenate([zero, Q], 1), 1).astype(F64) * inv_n).astype(F32)
        Pc = P - Op[:, None, :]
        Qc = Q - Oq[:, None, :]
        M = np.empty((H, 3, 3), F32)
        for i in range(3):
            for j in range(3):
                M[:, i, j] = seqsum(Pc[:, :, i] * Qc[:, :, j], 1)                       # sums start from their first term
        Sxx, Sxy, Sxz = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2]
        Syx, Syy, Syz = M[:, 1, 0], M[:, 1, 1], M[:, 1, 2]
        Szx, Szy, Szz = M[:, 2, 0], M[:, 2, 1], M[:, 2, 2]
        N = np.empty((H, 4, 4), F32)
        N[:, 0, 0] = (Sxx + Syy) + Szz
        N[:, 1, 1] = (Sxx - Syy) - Szz
        N[:, 2, 2] = (-Sxx + Syy) - Szz
        N[:, 3, 3] = (-Sxx - Syy) + Szz
        N[:, 0, 1] = N[:, 1, 0] = Syz - Szy
        N[:, 0, 2] = N[:, 2, 0] = Szx - Sxz
        N[:, 0, 3] = N[:, 3, 0] = Sxy - Syx
        N[:, 1, 2] = N[:, 2, 1] = Sxy + Syx
        N[:, 1, 3] = N[:, 3, 1] = Szx + Sxz
        N[:, 2, 3] = N[:, 3, 2] = Syz + Szy
        lam, V = jacobi(N.astype(F64))
        best = np.zeros(H, int)
        bv = lam[:, 0].copy()
        for k in range(1, 4):
            m = lam[:, k] > bv
            best = np.where(m, k, best)
            bv = np.where(m, lam[:, k], bv)
        q = V[np.arange(H), :, best].astype(F32)                                        # (w, x, y, z)
        w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        nrm = np.sqrt(((x * x + y * y) + z * z) + w * w)
        w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
        two = F32(2)
        tx, ty, tz = two * x, two * y, two * z
        twx, twy, twz = tx * w, ty * w, tz * w
        txx, txy, txz = tx * x, ty * x, tz * x
        tyy, tyz, tzz = ty * y, tz * y, tz * z
        one = F32(1)
        R = np.stack([one - (tyy + tzz), txy - twz, txz + twy,
                      txy + twz, one - (txx + tzz), tyz - twx,
                      txz - twy, tyz + twx, one - (txx + tyy)], 1).astype(F32)
        t = affine(-1.0, R, Op, Oq)
    return canon(np.concatenate([R, t], 1))


def check_inliers(P3, Q3, P2, Q2, thrP, thrQ, cam, model):
    """Sim3Solver::checkInliers for a batch of models (H, 12): (H, N) bool"""
    model = np.asarray(model, F32)
    R, t = model[:, :9], model[:, 9:]
    Rt = R[:, [0, 3, 6, 1, 4, 7, 2, 5, 8]]
    with np.errstate(all="ignore"):
        ti = np.stack([-_row3(Rt[:, 3 * r], Rt[:, 3 * r + 1], Rt[:, 3 * r + 2], t[:, 0], t[:, 1], t[:, 2]) for r in range(3)], 1)
        q_ = project(affine(1.0, R[:, None, :], P3[None], t[:, None, :]), cam)           # Sqp * P3d -> Q2d_
        p_ = project(affine(1.0, Rt[:, None, :], Q3[None], ti[:, None, :]), cam)         # Spq * Q3d -> P2d_

        def err(a, b):
            du = (a[..., 0] - b[None, :, 0]).astype(F64)
            dv = (a[..., 1] - b[None, :, 1]).astype(F64)
            return (du * du + dv * dv).astype(F32)
        eP, eQ = err(p_, P2), err(q_, Q2)
        return ~(eP > thrP[None, :]) & ~(eQ > thrQ[None, :])


# ---- Ransac<Sim3Ret> -------------------------------------------------------------------------------------------------------------
class Solver:
    """one Sim3Solver: create + iterate with the reference's state (S1-S7).  The model is None (empty Mats) or float32[12]."""

    def __init__(self, posP, posQ, octP, octQ, poseP, poseQ, level_sigma2=SIGMA2, cam=CAM, params=(3, 100, 0.4, 0.99)):
        posP = np.ascontiguousarray(posP, F32).reshape(-1, 3)
        posQ = np.ascontiguousarray(posQ, F32).reshape(-1, 3)
        poseP = np.asarray(poseP, F32).reshape(12)
        poseQ = np.asarray(poseQ, F32).reshape(12)
        self.cam = tuple(float(F32(v)) for v in cam)
        self.P3 = affine(1.0, poseP[None, :9], posP, poseP[None, 9:]).reshape(-1, 3)
        self.Q3 = affine(1.0, poseQ[None, :9], posQ, poseQ[None, 9:]).reshape(-1, 3)
        self.P2 = project(self.P3, self.cam).reshape(-1, 2)
        self.Q2 = project(self.Q3, self.cam).reshape(-1, 2)
        self.thrP = thresholds(octP, level_sigma2)
        self.thrQ = thresholds(octQ, level_sigma2)
        self.N = len(self.P3)
        assert params[0] == MIN_SET  # S1
        self.min_inlier, self.max_it = ransac_params(self.N, *params)
        self.cur = 0
        self.best = 0
        self.best_model = None
        self.best_list = []
        self.n_hyp = 0
        self.stats = dict(refine_success=0, fallback_best=0, failed=0, too_few=0, zero_budget=0, refine_failed=0)

    def model(self, idx):
        idx = np.asarray(idx, np.int64)
        return model_func(self.P3[idx][None], self.Q3[idx][None])[0]

    def check(self, model):
        m = check_inliers(self.P3, self.Q3, self.P2, self.Q2, self.thrP, self.thrQ, self.cam, model[None])[0]
        return np.nonzero(m)[0].tolist()

    def iterate(self, eng, n, model=None, inliers=()):
        """Ransac::iterate(n, model, bNoMore, inliers): (ret, no_more, model, inliers); no_more is only ever set"""
        lst = list(inliers)
        if self.N < MIN_SET:                                                             # S5
            self.stats["too_few"] += 1
            return False, True, model, lst
        k = max(0, min(n, self.max_it - self.cur))
        if k == 0:
            self.stats["zero_budget"] += 1
        probe = Engine(eng.state)
        samples, after = [], []
        for _ in range(k):
            samples.append(random_sample(probe, self.N, MIN_SET))
            after.append(probe.state)
        if k:
            sm = np.array(samples)
            models = model_func(self.P3[sm], self.Q3[sm])
            masks = check_inliers(self.P3, self.Q3, self.P2, self.Q2, self.thrP, self.thrQ, self.cam, models)
            self.n_hyp += k
        for h in range(k):
            model = models[h]
            lst = np.nonzero(masks[h])[0].tolist()                                       # S2: cleared by every checkInliers
            if len(lst) > self.min_inlier:
                if len(lst) > self.best:
                    self.best, self.best_model, self.best_list = len(lst), model, list(lst)
                model = self.model(lst)
                lst = self.check(model)
                if len(lst) > self.min_inlier:
                    eng.state = after[h]                                                 # S3: the budget is not spent
                    self.stats["refine_success"] += 1
                    return True, False, model, lst
                self.stats["refine_failed"] += 1
            self.cur += 1
        if k:
            eng.state = after[-1]
        no_more = self.cur >= self.max_it
        if self.best == 0:
            self.stats["failed"] += 1
            return False, no_more, model, lst
        self.stats["fallback_best"] += 1                                                 # S4
        return True, no_more, self.best_model, list(self.best_list)


def loop_closing_loop(iterate, n_problems, n=5, accept=None, max_calls=20000):
    """the second loop of LoopClosing::computeSim3 over `iterate(problem, n) -> (ret, no_more, model, inliers)`: round-robin over the
    problems not discarded; `accept(problem, model, inliers)` stands for searchBySim3 + OptimizeSim3 (default: never).  Returns the
    list of (problem, result) in call order.  A problem whose every call succeeds at once never spends its budget (S3) and the
    reference's loop then runs until a model is accepted: more than max_calls calls is an error here."""
    discard = [False] * n_problems
    left = n_problems
    log = []
    while left:
        for p in range(n_problems):
            if discard[p]:
                continue
            if len(log) >= max_calls:
                raise RuntimeError(f"loop_closing_loop: {max_calls} calls without an end")
            r = iterate(p, n)
            log.append((p, r))
            if r[1]:
                discard[p] = True
                left -= 1
            if r[0] and accept is not None and accept(p, r[2], r[3]):
                return log
    return log


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def scene(rng, N, outlier=0.0, noise=0.5, cam=CAM):
    """N map-point pairs seen 2 .. 20 m in front of both keyframes, related by a true rigid motion: keyframe p's pose, keyframe q's pose,
    the world positions of p's map points (exact) and of q's (moved by `noise` pixels at their depth; a share `outlier` of them anywhere
    in q's view), octaves 0 .. 7.  Returns (posP f32 (N, 3), posQ f32, octP i32, octQ i32, poseP f32[12], poseQ f32[12])."""
    fx, fy, cx, cy = cam
    Rp, tp = rot(rng), rng.normal(size=3) * 0.5
    Rqp, tqp = rot(rng, 0.1), rng.normal(size=3) * 0.3                                   # q's camera frame from p's
    Rq, tq = Rqp @ Rp, Rqp @ tp + tqp

    def in_view(m):
        z = rng.uniform(2, 20, m)
        return np.stack([rng.uniform(-0.4, 0.4, m) * z, rng.uniform(-0.3, 0.3, m) * z, z], 1)
    pc = in_view(N)
    qc = pc @ Rqp.T + tqp
    qc[:, 2] = np.clip(qc[:, 2], 2.0, 20.0)
    qc[:, :2] += rng.normal(size=(N, 2)) * noise * qc[:, 2:3] / np.array([fx, fy])
    out = rng.uniform(0, 1, N) < outlier
    qc[out] = in_view(int(out.sum()))
    posP = (pc - tp) @ Rp
    posQ = (qc - tq) @ Rq
    pose = lambda R, t: np.concatenate([R.reshape(9), t]).astype(F32)
    return (posP.astype(F32), posQ.astype(F32), rng.integers(0, 8, N).astype(np.int32), rng.integers(0, 8, N).astype(np.int32),
            pose(Rp, tp), pose(Rq, tq))
