"""Independent references for the SE3 code (test helper, plain Python): a gauge transform that gives every synthetic problem general
rotations without changing its measurements, and 40- to 50-digit mpmath restatements of the projection edges and of the exp-map update.

Nothing here shares a formula's spelling with the code under test: the rotation matrix is I + 2w[v]x + 2[v]x^2 (not the twelve products
of Eigen's toRotationMatrix), the point Jacobian is a central difference, the pose Jacobian perturbs the camera-frame point."""
from __future__ import annotations

import numpy as np
from mpmath import matrix, mp, mpf

# The gauges: a skew 2.9 rad one, and pi - 0.2 about axes a few percent off x, y and z.  The generators' poses are rotations about y by
# -0.3 .. 0.3 rad, so behind a near-axis gauge one quaternion component changes sign somewhere along the arc (w at yaw = -0.2 for near_y);
# the skews are chosen so that for the 6 keyframes of the edge tests (and the pose-only start poses, near_x) every component stays above
# 0.01: the tests assert it.
T_G = (1.5, -0.7, 2.2)                                           # |t_g| = 2.75 m <= 3 m: magnitudes stay those of the ungauged problems
GAUGES = {
    "skew": ((0.3, -0.5, 0.8), 2.9, T_G),
    "near_x": ((1.0, -0.05, 0.06), np.pi - 0.2, T_G),
    "near_y": ((-0.08, 1.0, 0.08), np.pi - 0.2, T_G),
    "near_z": ((-0.06, -0.05, 1.0), np.pi - 0.2, T_G),
}


# ---- numpy side: quaternions are (x, y, z, w) ---------------------------------------------------------------------------------------
def quat_of(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([np.sin(angle / 2) * a, [np.cos(angle / 2)]])


def quat_mul(a, b):
    """Hamilton product a (x) b, broadcasting over leading axes"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    av, aw, bv, bw = a[..., :3], a[..., 3:4], b[..., :3], b[..., 3:4]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), aw * bw - (av * bv).sum(-1, keepdims=True)], -1)


def quat_to_R(q):
    x, y, z, w = (float(v) for v in q)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + 2 * w * K + 2 * K @ K


def gauge_poses(poses, axis, angle, t_g):
    """world -> camera poses (q, t) after the world change X' = R_g X + t_g:  q' = q (x) g^-1,  t' = t - R(q') t_g"""
    poses = np.asarray(poses, np.float64)
    flat = poses.reshape(-1, 7)
    g = quat_of(axis, angle)
    q = quat_mul(flat[:, :4], g * np.array([-1.0, -1.0, -1.0, 1.0]))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = np.stack([flat[i, 4:] - quat_to_R(q[i]) @ np.asarray(t_g, np.float64) for i in range(len(flat))])
    return np.concatenate([q, t], 1).reshape(poses.shape)


def ungauge_poses(poses, axis, angle, t_g):
    """the inverse of gauge_poses:  q = q' (x) g,  t = t' + R(q') t_g"""
    poses = np.asarray(poses, np.float64)
    flat = poses.reshape(-1, 7)
    q = quat_mul(flat[:, :4], quat_of(axis, angle))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = np.stack([flat[i, 4:] + quat_to_R(flat[i, :4]) @ np.asarray(t_g, np.float64) for i in range(len(flat))])
    return np.concatenate([q, t], 1).reshape(poses.shape)


def gauge_points(X, axis, angle, t_g):
    return np.asarray(X, np.float64) @ quat_to_R(quat_of(axis, angle)).T + np.asarray(t_g, np.float64)


_POSE_KEYS, _POINT_KEYS = ("poses", "poses_true", "pose", "truth"), ("points", "points_true", "Xw")


def gauge(problem, axis, angle, t_g):
    """A copy of a ba_synth.make_problem / make_pose_problem dict in the world X' = R_g X + t_g.  Edges, measurements, information and
    deltas are untouched: every camera-frame point, hence every projection, is what it was (to the rounding of the new vertices)."""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in problem.items()}
    for k in _POSE_KEYS:
        if k in out:
            out[k] = gauge_poses(out[k], axis, angle, t_g)
    for k in _POINT_KEYS:
        if k in out:
            out[k] = gauge_points(out[k], axis, angle, t_g)
    return out


def negate_q(problem):
    """the same rotations written with the other sign of every pose quaternion"""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in problem.items()}
    for k in _POSE_KEYS:
        if k in out:
            out[k][..., :4] = -out[k][..., :4]
    return out


def trace_branch(q):
    """(trace, i) of R(q): i is the index Eigen's Quaternion(Matrix3) takes when trace <= 0 (the largest diagonal element, the first of
    equals), whatever the trace is"""
    d = np.diag(quat_to_R(q))
    i = 0
    if d[1] > d[0]:
        i = 1
    if d[2] > d[i]:
        i = 2
    return float(d.sum()), i


def pose_dist_R(a, b):
    """(max |R(qa) - R(qb)|, max |ta - tb|) of two (q, t) poses: blind to the sign of the quaternion"""
    return float(np.abs(quat_to_R(a[:4]) - quat_to_R(b[:4])).max()), float(np.abs(np.asarray(a[4:]) - np.asarray(b[4:])).max())


# ---- mpmath side --------------------------------------------------------------------------------------------------------------------
def _skew(v):
    return matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def _mp_R(q):
    K = _skew(q[:3])
    return matrix(3, 3) + mp.eye(3) + 2 * q[3] * K + 2 * K * K


def _project(P, meas, stereo, cam):
    fx, fy, cx, cy, bf = cam
    u, v = fx * P[0] / P[2] + cx, fy * P[1] / P[2] + cy
    return [meas[0] - u, meas[1] - v, meas[2] - (u - bf / P[2]) if stereo else mpf(0)]


def mp_edge(T, X, meas, stereo, cam):
    """One projection edge at 40 digits.  T = (q xyzw, t) world -> camera, cam = (fx, fy, cx, cy, bf); a mono edge has a zero third row.
    -> (error [3], d e / d X [3][3] by central differences at h = 1e-15, d e / d (omega, upsilon) [3][6] of exp(delta) * T, by central
    differences on the camera-frame point P + omega x P + upsilon), as float64 arrays"""
    old = mp.dps
    mp.dps = 40
    try:
        T, X, meas, cam = [mpf(float(v)) for v in T], [mpf(float(v)) for v in X], [mpf(float(v)) for v in meas], [mpf(float(v)) for v in cam]
        R, t = _mp_R(T[:4]), matrix(T[4:])
        cam_pt = lambda x: R * matrix(x) + t
        P = cam_pt(X)
        err = _project(P, meas, stereo, cam)
        h = mpf(10) ** -15
        jx, jp = np.zeros((3, 3)), np.zeros((3, 6))
        for a in range(3):
            xp, xm = list(X), list(X)
            xp[a] += h
            xm[a] -= h
            ep, em = _project(cam_pt(xp), meas, stereo, cam), _project(cam_pt(xm), meas, stereo, cam)
            jx[:, a] = [float((ep[r] - em[r]) / (2 * h)) for r in range(3)]
        for a in range(6):
            d = [mpf(0)] * 6
            d[a] = h
            moved = []
            for s in (1, -1):
                om, up = matrix([s * v for v in d[:3]]), matrix([s * v for v in d[3:]])
                moved.append(_project(P + _skew(om) * P + up, meas, stereo, cam))
            jp[:, a] = [float((moved[0][r] - moved[1][r]) / (2 * h)) for r in range(3)]
        return np.array([float(e) for e in err]), jx, jp
    finally:
        mp.dps = old


def mp_edges(prob):
    """mp_edge over every edge of a problem dict -> dict(error (E,3), j_point (E,3,3), j_pose (E,3,6))"""
    cam = (prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"])
    E = len(prob["edge_pose"])
    out = dict(error=np.zeros((E, 3)), j_point=np.zeros((E, 3, 3)), j_pose=np.zeros((E, 3, 6)))
    for e in range(E):
        out["error"][e], out["j_point"][e], out["j_pose"][e] = mp_edge(prob["poses"][prob["edge_pose"][e]], prob["points"][prob["edge_point"][e]],
                                                                        prob["meas"][e], bool(prob["is_stereo"][e]), cam)
    return out


def mp_oplus(T, upd):
    """exp(upd) * T at 50 digits with the closed-form R and V (upd = (omega, upsilon)) -> (R [3][3], t [3]) as float64 arrays, and the
    branch the fp64 code takes for this update: 'series' (theta < 1e-5), 'tr>0', or the largest-diagonal index 0 / 1 / 2 (trace <= 0)"""
    old = mp.dps
    mp.dps = 50
    try:
        T, upd = [mpf(float(v)) for v in T], [mpf(float(v)) for v in upd]
        om, ups = upd[:3], matrix(upd[3:])
        th = mp.sqrt(sum(v * v for v in om))
        Om = _skew(om)
        I = mp.eye(3)
        Re = I + mp.sin(th) / th * Om + (1 - mp.cos(th)) / th ** 2 * Om * Om
        V = I + (1 - mp.cos(th)) / th ** 2 * Om + (th - mp.sin(th)) / th ** 3 * Om * Om
        n = mp.sqrt(sum(v * v for v in T[:4]))
        R = Re * _mp_R([v / n for v in T[:4]])
        t = Re * matrix(T[4:]) + V * ups
        tr = Re[0, 0] + Re[1, 1] + Re[2, 2]
        if th < mpf("0.00001"):
            branch = "series"
        elif tr > 0:
            branch = "tr>0"
        else:
            branch = 0
            if Re[1, 1] > Re[0, 0]:
                branch = 1
            if Re[2, 2] > Re[branch, branch]:
                branch = 2
        return np.array([[float(R[i, j]) for j in range(3)] for i in range(3)]), np.array([float(t[i]) for i in range(3)]), branch
    finally:
        mp.dps = old


def oplus_cases():
    """The exp-map case table: two base poses with every component large (w < 0 and w > 0), update angles either side of the 1e-5
    series threshold and of the trace <= 0 boundary (2 pi / 3), each about axes near x, near y, near z and the diagonal.
    upsilon is 0.18 m long: the closed form's (1 - cos theta) / theta^2 carries cos's rounding, eps / theta^2, into t as
    eps |upsilon| / theta = 1e-12 at theta = 2e-5, a tenth of the 1e-11 bound.  -> (poses (48, 7), upd (48, 6))"""
    bases = []
    for q in ((0.41, -0.52, 0.33, -0.67), (-0.36, 0.48, 0.59, 0.54)):
        q = np.array(q) / np.linalg.norm(q)
        bases.append(np.concatenate([q, [0.8, -1.3, 2.1]]))
    axes = [(1.0, 0.04, -0.03), (-0.03, 1.0, 0.04), (0.04, -0.03, 1.0), (0.55, -0.6, 0.58)]
    angles = [3e-6, 2e-5, 1e-2, 1.6, 2.6, np.pi - 1e-3]
    poses, upd = [], []
    for b in bases:
        for ang in angles:
            for ax in axes:
                a = np.array(ax) / np.linalg.norm(ax)
                poses.append(b)
                upd.append(np.concatenate([ang * a, [0.1, -0.12, 0.08]]))
    return np.array(poses), np.array(upd)
