"""Synthetic local-BA problem of BASELINE config 5: 60 keyframes on a 3 m arc, 3000 points in a
6x3x4 m box, each point observed by 3..8 keyframes that see it, 80 % stereo / 20 % mono edges, integer-only
Irwin-Hall measurement noise scaled by the octave sigma, 5 % gross outliers.  Intrinsics from
config/tum_config_f2.yaml (fx 520.9 fy 521.0 cx 325.1 cy 249.7, bf = fx*0.0767889)."""
from __future__ import annotations

import numpy as np

from .synth import hash_u64

FX, FY, CX, CY = 520.908620, 521.007327, 325.141442, 249.701764
BF = FX * 0.0767889


def _u(seed, stream, idx):
    """uniform [0,1) doubles with 53 random bits"""
    return (hash_u64(seed, stream, idx) >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def _irwin_hall(seed, stream, idx):
    """~N(0,1): sum of 12 uniform 16-bit draws, integer-only generator"""
    idx = np.asarray(idx, np.uint64)
    s = np.zeros(idx.shape, np.float64)
    for k in range(12):
        s += (hash_u64(seed, stream + k, idx) & np.uint64(0xFFFF)).astype(np.float64)
    return s / 65536.0 - 6.0


def _quat_from_yaw(yaw):
    return np.stack([np.zeros_like(yaw), np.sin(yaw / 2), np.zeros_like(yaw), np.cos(yaw / 2)], 1)  # rotation about y


def make_problem(seed=42, n_kf=60, n_pt=3000, scale_factor=1.2, n_levels=8, with_truth=False):
    # camera centres on an arc of radius 3 m looking roughly along +z
    ang = np.linspace(-0.5, 0.5, n_kf)
    centres = np.stack([3.0 * np.sin(ang), 0.05 * np.cos(7 * ang), 3.0 * (1 - np.cos(ang))], 1)
    yaw = -0.6 * ang
    q_cw = _quat_from_yaw(yaw)  # world -> camera rotation (about y)

    def rot(q, v):
        qv, qw = q[..., :3], q[..., 3:4]
        uv = 2 * np.cross(qv, v)
        return v + qw * uv + np.cross(qv, uv)

    t_cw = -rot(q_cw, centres)
    poses = np.concatenate([q_cw, t_cw], 1)
    pid = np.arange(n_pt)
    points = np.stack([(_u(seed, 1, pid) - 0.5) * 6.0, (_u(seed, 2, pid) - 0.5) * 3.0, 2.0 + _u(seed, 3, pid) * 4.0], 1)

    sigma = np.float32(scale_factor) ** np.arange(n_levels, dtype=np.float32)
    e_pose, e_pt, meas, stereo, info, delta = [], [], [], [], [], []
    d_mono, d_stereo = float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815)))
    eid = 0
    for p in range(n_pt):
        want = 3 + int(hash_u64(seed, 4, p) % np.uint64(6))
        start = int(hash_u64(seed, 5, p) % np.uint64(n_kf))
        got = 0
        for j in range(n_kf):
            k = (start + j * 7) % n_kf
            pc = rot(poses[k, :4], points[p]) + poses[k, 4:]
            if pc[2] < 0.3:
                continue
            u, v = FX * pc[0] / pc[2] + CX, FY * pc[1] / pc[2] + CY
            if not (0 <= u < 640 and 0 <= v < 480):
                continue
            octave = int(hash_u64(seed, 6, eid) % np.uint64(n_levels))
            s = float(sigma[octave])
            nz = _irwin_hall(seed, 10, np.array([3 * eid, 3 * eid + 1, 3 * eid + 2])) * s
            if hash_u64(seed, 7, eid) % np.uint64(20) == 0:  # 5 % gross outliers
                nz = nz + np.array([35.0, -28.0, 31.0])
            is_st = (hash_u64(seed, 8, eid) % np.uint64(5)) != 0  # 80 % stereo
            ur = u - BF / pc[2]
            # measurements are float32 in the reference (kp.pt.x, rightU stored from float math)
            meas.append([np.float32(u + nz[0]), np.float32(v + nz[1]), np.float32(ur + nz[2]) if is_st else -1.0])
            inv_s = np.float32(1.0) / sigma[octave]
            # quirk Q9: stereo edges use invSigma^2, mono edges use invSigma (Optimizer.cc:301 vs :319)
            info.append(float(np.float32(inv_s) ** 2) if is_st else float(inv_s))
            delta.append(d_stereo if is_st else d_mono)
            stereo.append(1 if is_st else 0)
            e_pose.append(k)
            e_pt.append(p)
            eid += 1
            got += 1
            if got >= want:
                break
    # perturb the estimates so errors/Jacobians are not trivially zero
    kid = np.arange(n_kf)
    poses_est = poses.copy()
    poses_est[:, 4:] += 0.02 * np.stack([_irwin_hall(seed, 30, kid), _irwin_hall(seed, 50, kid), _irwin_hall(seed, 70, kid)], 1)
    points_est = points + 0.03 * np.stack([_irwin_hall(seed, 90, pid), _irwin_hall(seed, 110, pid), _irwin_hall(seed, 130, pid)], 1)
    out = dict(poses=poses_est, points=points_est, edge_pose=np.asarray(e_pose, np.int32), edge_point=np.asarray(e_pt, np.int32),
               meas=np.asarray(meas, np.float64), is_stereo=np.asarray(stereo, np.uint8), info=np.asarray(info, np.float64),
               huber_delta=np.asarray(delta, np.float64), fx=FX, fy=FY, cx=CX, cy=CY, bf=BF)
    if with_truth:  # the noise-free vertices the measurements were generated from
        out.update(poses_true=poses, points_true=points)
    return out


def make_pose_problem(seed=7, n=1000, scale_factor=1.2, n_levels=8, outlier_every=12):
    """One frame for Optimizer::OptimizePoseOnly (Optimizer.cc:33-203): n map points seen by a camera whose initial pose is a
    perturbed version of the truth; 70 % stereo / 30 % mono observations with octave-scaled noise, every `outlier_every`-th
    observation a gross outlier.  Returns the arrays of the C-ABI call."""
    idx = np.arange(n)
    X = np.stack([(_u(seed, 1, idx) - 0.5) * 8.0, (_u(seed, 2, idx) - 0.5) * 4.0, 3.0 + _u(seed, 3, idx) * 9.0], 1)
    q_true = np.array([0.02, -0.03, 0.01, 0.0])
    q_true[3] = np.sqrt(1 - (q_true[:3] ** 2).sum())
    t_true = np.array([0.10, -0.05, 0.20])

    def rot(q, v):
        qv, qw = q[:3], q[3]
        uv = 2 * np.cross(qv, v)
        return v + qw * uv + np.cross(qv, uv)

    Pc = rot(q_true, X) + t_true
    u = FX * Pc[:, 0] / Pc[:, 2] + CX
    v = FY * Pc[:, 1] / Pc[:, 2] + CY
    ur = u - BF / Pc[:, 2]
    octave = (hash_u64(seed, 4, idx) % np.uint64(n_levels)).astype(np.int64)
    sig = (np.float32(scale_factor) ** octave.astype(np.float32)).astype(np.float32)
    nz = np.stack([_irwin_hall(seed, 10, idx), _irwin_hall(seed, 30, idx), _irwin_hall(seed, 50, idx)], 1) * sig[:, None]
    out = (idx % outlier_every) == 0
    nz[out] += np.array([40.0, -33.0, 36.0])
    stereo = (hash_u64(seed, 5, idx) % np.uint64(10)) < np.uint64(7)
    meas = np.stack([np.float32(u + nz[:, 0]), np.float32(v + nz[:, 1]), np.where(stereo, np.float32(ur + nz[:, 2]), -1.0)], 1).astype(np.float64)
    inv_s = (np.float32(1.0) / sig).astype(np.float32)
    info = (inv_s.astype(np.float32) ** 2).astype(np.float64)   # getScaledFactorInv2 (float pow), both edge kinds (Optimizer.cc:85,106)
    sigma2 = (sig ** 2).astype(np.float32)                        # getScaledFactor2
    q0 = q_true + np.array([0.004, -0.003, 0.002, 0.0])
    q0 /= np.linalg.norm(q0)
    pose0 = np.concatenate([q0, t_true + np.array([0.05, -0.04, 0.06])])
    return dict(Xw=X, meas=meas, info=info, sigma2=sigma2, pose=pose0, fx=FX, fy=FY, cx=CX, cy=CY, bf=BF,
                truth=np.concatenate([q_true, t_true]), outlier=out)


def _rot_from_rotvec(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * (K @ K)


def make_sim3_problem(seed=11, n=200, n_outliers=20, noise_px=0.5, scale_factor=1.2, n_levels=8):
    """One loop candidate for Optimizer::OptimizeSim3 (Optimizer.cc:464-619): n matched map points of two keyframes related by a known
    rigid motion p_c = R p_m + t (scale 1), all in front of both cameras; key points with octave-scaled noise of noise_px pixels at
    octave 0, exactly n_outliers pairs with a gross error of tens of pixels in the current image, the matched one, or both; the
    information of both edges from the octaves; the start model the truth moved by about two degrees and a few centimetres, as a
    RANSAC result is.  Returns the arrays of orbfe_sim3_optimize plus truth_R, truth_t and the outlier mask."""
    idx = np.arange(n)
    z = 3.0 + _u(seed, 3, idx) * 9.0
    Pm = np.stack([(_u(seed, 1, idx) - 0.5) * 0.7 * z, (_u(seed, 2, idx) - 0.5) * 0.5 * z, z], 1)
    R = _rot_from_rotvec([0.05, -0.12, 0.03])
    t = np.array([0.30, -0.05, 0.15])
    Pc = Pm @ R.T + t
    cam = np.array([FX, FY, CX, CY])

    def proj(P):
        return np.stack([FX * P[:, 0] / P[:, 2] + CX, FY * P[:, 1] / P[:, 2] + CY], 1)
    oct_c = (hash_u64(seed, 4, idx) % np.uint64(n_levels)).astype(np.int64)
    oct_m = (hash_u64(seed, 5, idx) % np.uint64(n_levels)).astype(np.int64)
    sig_c = (np.float32(scale_factor) ** oct_c.astype(np.float32)).astype(np.float32)
    sig_m = (np.float32(scale_factor) ** oct_m.astype(np.float32)).astype(np.float32)
    nz_c = np.stack([_irwin_hall(seed, 10, idx), _irwin_hall(seed, 30, idx)], 1) * sig_c[:, None] * noise_px
    nz_m = np.stack([_irwin_hall(seed, 50, idx), _irwin_hall(seed, 70, idx)], 1) * sig_m[:, None] * noise_px
    order = np.argsort(hash_u64(seed, 6, idx), kind="stable")
    out = np.zeros(n, bool)
    out[order[:n_outliers]] = True
    kind = np.zeros(n, np.int64)
    kind[order[:n_outliers]] = np.arange(n_outliers) % 3                       # 0: current image, 1: matched image, 2: both
    gross = np.stack([30.0 + 40.0 * _u(seed, 7, idx), -(25.0 + 30.0 * _u(seed, 8, idx))], 1)
    nz_c[out & (kind != 1)] += gross[out & (kind != 1)]
    nz_m[out & (kind != 0)] -= gross[out & (kind != 0)]
    inv2 = lambda s: ((np.float32(1.0) / s).astype(np.float32) ** 2).astype(np.float64)   # getScaledFactorInv2
    R0 = _rot_from_rotvec([0.02, 0.025, -0.015]) @ R
    t0 = t + np.array([0.04, -0.03, 0.05])
    return dict(pc=Pc.astype(np.float32), pm=Pm.astype(np.float32), uv_c=(proj(Pc) + nz_c).astype(np.float32),
                uv_m=(proj(Pm) + nz_m).astype(np.float32), info_c=inv2(sig_c), info_m=inv2(sig_m), cam=tuple(float(v) for v in cam),
                model=np.concatenate([R0.reshape(9), t0]).astype(np.float32), truth_R=R, truth_t=t, outlier=out)


def make_trajectory_problem(seed, n_kf, per_kf, loop=3, huber=True, outliers=0.05, scale_factor=1.2, n_levels=8, with_truth=False):
    """A map as Optimizer::globalOptimization sees it after a loop closure: n_kf identity-rotation cameras stepping 0.25 m along x, the
    last `loop` of them placed back near the start (at x = 0.1 + 0.25 k); per_kf * n_kf points spread along the path at depth 3..7 m,
    each observed by 2..8 keyframes that are consecutive among the ones that see it (in keyframe order, so a window over the first
    keyframes may run into the loop keyframes); 80 % stereo edges; information 1 / sigma^2 of a random octave for both edge kinds
    (Optimizer.cc:975, :990); Huber deltas of the reference if `huber`, none (-1) otherwise; a fraction `outliers` of gross measurement
    errors; keyframe 0 at its true pose (the reference fixes it).  The reduced camera system is a band of half-width <= 7 blocks plus the
    loop blocks.  Deterministic: every draw comes from the integer hash generators of this module.  Returns the arrays of
    orbfe_ba_problem."""
    assert n_kf >= 2 and 0 <= loop < n_kf - 1 and per_kf >= 1
    step, n_main = 0.25, n_kf - loop
    cx_kf = np.concatenate([step * np.arange(n_main), 0.1 + step * np.arange(loop)])
    poses = np.zeros((n_kf, 7))
    poses[:, 3] = 1.0
    poses[:, 4] = -cx_kf                                                       # t_cw = -R centre, R = I
    n_pt = per_kf * n_kf
    pid = np.arange(n_pt)
    z = 3.0 + 4.0 * _u(seed, 3, pid)
    points = np.stack([_u(seed, 1, pid) * step * (n_main - 1), (_u(seed, 2, pid) - 0.5) * 2.0, z], 1)
    # the keyframes that see a point, in keyframe order: a window of the main chain around it, then the loop keyframes
    half = int(np.ceil(0.65 * 7.0 / step)) + 1
    cand = np.rint(points[:, 0] / step).astype(np.int64)[:, None] + np.arange(-half, half + 1)[None, :]
    cand = np.concatenate([cand, np.broadcast_to(n_main + np.arange(loop), (n_pt, loop))], 1)
    valid = (cand >= 0) & (cand < n_kf) & ((cand < n_main) | (np.arange(cand.shape[1])[None, :] > 2 * half))
    ck = np.clip(cand, 0, n_kf - 1)
    u_all = FX * (points[:, 0:1] - cx_kf[ck]) / z[:, None] + CX
    v_pt = FY * points[:, 1] / z + CY
    vis = valid & (u_all >= 0) & (u_all < 640) & ((v_pt >= 0) & (v_pt < 480))[:, None]
    cnt = vis.sum(1)
    want = np.minimum(2 + (hash_u64(seed, 4, pid) % np.uint64(7)).astype(np.int64), cnt)
    start = (hash_u64(seed, 5, pid) % np.maximum(cnt - want + 1, 1).astype(np.uint64)).astype(np.int64)
    rank = np.cumsum(vis, 1) - 1
    take = vis & (rank >= start[:, None]) & (rank < (start + want)[:, None])
    e_pt, col = np.nonzero(take)                                              # point-major, keyframes ascending
    e_pose = ck[e_pt, col]
    E = e_pt.size
    eid = np.arange(E)
    sigma = np.float32(scale_factor) ** np.arange(n_levels, dtype=np.float32)
    octave = (hash_u64(seed, 6, eid) % np.uint64(n_levels)).astype(np.int64)
    s = sigma[octave].astype(np.float64)
    nz = np.stack([_irwin_hall(seed, 10, 3 * eid), _irwin_hall(seed, 10, 3 * eid + 1), _irwin_hall(seed, 10, 3 * eid + 2)], 1) * s[:, None]
    if outliers > 0:
        gross = (hash_u64(seed, 7, eid) % np.uint64(10000)).astype(np.int64) < int(round(outliers * 10000))
        nz[gross] += np.array([35.0, -28.0, 31.0])
    is_st = (hash_u64(seed, 8, eid) % np.uint64(5)) != 0                       # 80 % stereo
    ze = z[e_pt]
    u = FX * (points[e_pt, 0] - cx_kf[e_pose]) / ze + CX
    v = FY * points[e_pt, 1] / ze + CY
    ur = u - BF / ze
    # measurements are float32 in the reference (kp.pt.x, rightU stored from float math)
    meas = np.stack([np.float32(u + nz[:, 0]), np.float32(v + nz[:, 1]), np.where(is_st, np.float32(ur + nz[:, 2]), -1.0)], 1).astype(np.float64)
    inv_s = (np.float32(1.0) / sigma[octave]).astype(np.float32)
    info = (inv_s ** 2).astype(np.float64)                                    # getScaledFactorInv2 for both edge kinds
    d_mono, d_stereo = float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815)))
    delta = np.where(is_st, d_stereo, d_mono) if huber else np.full(E, -1.0)
    kid = np.arange(n_kf)
    poses_est = poses.copy()
    poses_est[1:, 4:] += 0.02 * np.stack([_irwin_hall(seed, 30, kid), _irwin_hall(seed, 50, kid), _irwin_hall(seed, 70, kid)], 1)[1:]
    points_est = points + 0.03 * np.stack([_irwin_hall(seed, 90, pid), _irwin_hall(seed, 110, pid), _irwin_hall(seed, 130, pid)], 1)
    out = dict(poses=poses_est, points=points_est, edge_pose=e_pose.astype(np.int32), edge_point=e_pt.astype(np.int32), meas=meas,
               is_stereo=is_st.astype(np.uint8), info=info, huber_delta=np.asarray(delta, np.float64), fx=FX, fy=FY, cx=CX, cy=CY, bf=BF)
    if with_truth:
        out.update(poses_true=poses, points_true=points)
    return out
