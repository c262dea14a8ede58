"""Seeded multi-view scenes for the createNewMapPoints tests: known 3D points seen by a current keyframe and its neighbours, with
descriptors that stay close across views, stereo depth on part of the features and FeatureVectors from a node function (host) or
from the device BoW transform (GPU tests)."""
from __future__ import annotations

import numpy as np

from orb_slam2_ros2_amd._lib import KP_DTYPE

F32 = np.float32
CAM = (F32(500.0), F32(500.0), F32(320.0), F32(240.0))
BF = 40.0
W, H = 640, 480
SF = (F32(1.2) ** np.arange(8)).astype(F32)


def k_inv(cam=CAM):
    fx, fy, cx, cy = cam
    return np.array([[F32(1) / fx, 0, F32(-cx / fx)], [0, F32(1) / fy, F32(-cy / fy)], [0, 0, 1]], F32)


def yaw(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def pose(center, R=None):
    """(Tcw, Twc, Ow) float32 from a camera centre and a world-to-camera rotation"""
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    C = np.asarray(center, np.float64)
    Tcw = np.eye(4)
    Tcw[:3, :3], Tcw[:3, 3] = R, -R @ C
    Twc = np.eye(4)
    Twc[:3, :3], Twc[:3, 3] = R.T, C
    return Tcw.astype(F32), Twc.astype(F32), C.astype(F32)


def csr_from_nodes(node_of):
    """FeatureVector CSR (nodes ascending, features ascending inside a node) from a node per feature (-1: none)"""
    node_of = np.asarray(node_of, np.int64)
    idx = np.flatnonzero(node_of >= 0)
    order = idx[np.lexsort((idx, node_of[idx]))]
    nodes, starts = np.unique(node_of[order], return_index=True)
    offs = np.append(starts, len(order)).astype(np.int32)
    return nodes.astype(np.uint32), offs, order.astype(np.uint32)


def make_kf(rng, pts, base_desc, centre, R=None, n=2000, stereo_frac=0.4, n_nodes=97, flip_bits=6, good_frac=0.15, unproc=False, px_noise=0.3):
    Tcw, Twc, Ow = pose(centre, R)
    fx, fy, cx, cy = (float(v) for v in CAM)
    pc = (Tcw[:3, :3].astype(np.float64) @ pts.T).T + Tcw[:3, 3]
    with np.errstate(all="ignore"):
        u = fx * pc[:, 0] / pc[:, 2] + cx
        v = fy * pc[:, 1] / pc[:, 2] + cy
    vis = np.flatnonzero((pc[:, 2] > 0.5) & (u > 5) & (u < W - 5) & (v > 5) & (v < H - 5))
    pid = rng.permutation(vis)[:n]
    m = len(pid)
    kps = np.zeros(m, KP_DTYPE)
    kps["x"] = (u[pid] + rng.normal(0, px_noise, m)).astype(F32)
    kps["y"] = (v[pid] + rng.normal(0, px_noise, m)).astype(F32)
    kps["size"], kps["class_id"] = 7.0, -1
    kps["octave"] = (pid * 31) % 3   # one octave per point, as a consistent scale would give
    desc = base_desc[pid].copy()
    for i in range(m):
        for b in rng.integers(0, 256, rng.integers(0, flip_bits + 1)):
            desc[i, b >> 3] ^= np.uint8(1 << (b & 7))
    depth = np.full(m, -1.0)
    right_u = np.full(m, -1.0)
    st = rng.random(m) < stereo_frac
    depth[st] = pc[pid[st], 2] * (1 + rng.normal(0, 0.002, st.sum()))
    right_u[st] = kps["x"][st].astype(np.float64) - BF / depth[st]
    r = rng.random(m)
    flags = np.where(r < good_frac, 3, np.where(r < good_frac + 0.05, 1, 0)).astype(np.uint8)
    kf = dict(kps=kps, desc=desc, fv=csr_from_nodes((pid * 7919) % n_nodes), flags=flags, depth=depth, right_u=right_u,
              Tcw=Tcw, Twc=Twc, Ow=Ow, pid=pid)
    if unproc:
        un = st & (flags == 0) & (rng.random(m) < 0.6)
        kf["unproc"] = un
        kf["unproc_pos"] = (pts[pid] + rng.normal(0, 0.01, (m, 3))).astype(F32)
    return kf


def scene(seed=0, n_nb=10, n=2000, n_pts=6000, baselines=None, **kw):
    """current keyframe + n_nb neighbours looking down +z at points 4..14 m away"""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-6, 6, n_pts), rng.uniform(-4, 4, n_pts), rng.uniform(4, 14, n_pts)], 1)
    base = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)
    cur = make_kf(rng, pts, base, (0, 0, 0), n=n, unproc=True, **kw)
    if baselines is None:
        baselines = [0.06, 0.1, 0.3, 0.6, 1.0, 0.08, 0.5, 0.2, 0.12, 0.8, 0.07, 0.4][:n_nb] + [0.3] * max(0, n_nb - 12)
    nbs = []
    for i, b in enumerate(baselines):
        ang = rng.uniform(0, 2 * np.pi)
        c = (b * np.cos(ang), 0.3 * b * np.sin(ang), 0.2 * b * rng.normal())
        nbs.append(make_kf(rng, pts, base, c, yaw(rng.normal(0, 0.02)), n=n, **kw))
    return cur, nbs, pts


BL = F32(0.05)   # Camera::mfBl = bf / fx (0.08) would skip the closest neighbours; the tests pick their own
