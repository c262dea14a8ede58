"""Seeded scenes for the fuseMapPoints tests: a current keyframe, K target keyframes with their own feature counts and poses, the map
points in the current keyframe's slots, and a small mutable map model (MapModel) that the replay of
orb_slam2_ros2_amd.matcher_ext.MatcherExt.fuseIntoKeyframes and the plain sequential chain both run on."""
from __future__ import annotations

import copy
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tri_scenes as ts  # noqa: E402
import fuse_restatement as fr  # noqa: E402
from orb_slam2_ros2_amd._lib import KP_DTYPE  # noqa: E402
from orb_slam2_ros2_amd.matcher_ext import is_in_vision, tlc_z  # noqa: E402

F32 = np.float32
CAM, SF, W, H = ts.CAM, ts.SF, ts.W, ts.H
BL = F32(0.05)
BOUNDS = np.array([0, W, 0, H], F32)
CUR = 0          # the current keyframe's id in the model; target k is keyframe 1 + k (or CUR itself)
FAR0 = 1000      # keyframes that only observe: far to the side, so that a point they dominate looks sideways


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


class MapModel:
    """Keyframes (pose, centre, descriptors, slot -> point id) and map points (position, view direction, distance range, descriptor,
    observations keyframe -> feature, bad flag) with MapPoint::addObservation / replace / updateNormalAndDepth after
    src/MapPoint.cc:21-45, 213-233, 429-484 in float32.  Not modelled: updateDescriptor (a point keeps its descriptor), bad keyframes and
    an invalid reference keyframe (so the distance range never changes), the map's own point list."""

    def __init__(self):
        self.kf = {}       # id -> dict(Rcw, tcw, bounds, centre, desc or None)
        self.slots = {}    # id -> {feature: point id}
        self.pt = {}       # id -> dict(pos, view_dir, max_dist, min_dist, desc, obs {kf: feature}, bad)

    def copy(self):
        return copy.deepcopy(self)

    def add_kf(self, kid, Rcw, tcw, centre, desc=None, bounds=BOUNDS):
        self.kf[kid] = dict(Rcw=np.asarray(Rcw, F32), tcw=np.asarray(tcw, F32), centre=np.asarray(centre, F32), desc=desc, bounds=bounds)
        self.slots.setdefault(kid, {})

    def add_point(self, pid, pos, desc, max_dist=F32(100), min_dist=F32(0.01)):
        self.pt[pid] = dict(pos=np.asarray(pos, F32), view_dir=np.array([0, 0, 1], F32), max_dist=F32(max_dist), min_dist=F32(min_dist),
                            desc=np.asarray(desc, np.uint8), obs={}, bad=False)

    # ---- what the replay needs -----------------------------------------------------------------------------------------------------
    def slot(self, kf, i):
        return self.slots[kf].get(i, -1)

    def is_bad(self, pid):
        return self.pt[pid]["bad"]

    def n_obs(self, pid):
        return len(self.pt[pid]["obs"])

    def set_slot(self, kf, i, pid):
        self.slots[kf][i] = pid

    def in_vision(self, pid, kf):
        p, k = self.pt[pid], self.kf[kf]
        return is_in_vision(p["pos"], p["view_dir"], p["max_dist"], p["min_dist"], k["Rcw"], k["tcw"], CAM, k["bounds"])

    def add_observation(self, pid, kf, feat):
        obs = self.pt[pid]["obs"]
        if kf not in obs:
            obs[kf] = feat
            return
        d = self.kf[kf]["desc"]   # both features of pKf against the point's descriptor: the closer one stays (MapPoint.cc:36-42)
        if d is not None:
            obs[kf] = obs[kf] if hamming(d[obs[kf]], self.pt[pid]["desc"]) < hamming(d[feat], self.pt[pid]["desc"]) else feat

    def update_normal_and_depth(self, pid):
        p = self.pt[pid]
        if not p["obs"]:
            p["bad"] = True
            return
        v = np.zeros(3, F32)
        for kf in sorted(p["obs"]):
            v = (v + (p["pos"] - self.kf[kf]["centre"]).astype(F32)).astype(F32)
        nrm = np.sqrt(np.float64(v[0]) ** 2 + np.float64(v[1]) ** 2 + np.float64(v[2]) ** 2)   # cv::normalize: the scale 1 / norm in double
        p["view_dir"] = (v.astype(np.float64) * (1.0 / nrm)).astype(F32) if nrm > 0 else v

    def replace(self, keep, drop):
        d = self.pt[drop]
        d["bad"] = True
        obs, d["obs"] = d["obs"], {}
        for kf in sorted(obs):
            if kf in self.pt[keep]["obs"]:
                continue
            self.slots[kf][obs[kf]] = keep
            self.add_observation(keep, kf, obs[kf])
        self.update_normal_and_depth(keep)

    # ---- views of the state ----------------------------------------------------------------------------------------------------------
    def slot_points(self, kf, n):
        """the arrays of orbfe_fuse_points for the points in kf's slots now"""
        out = dict(has_point=np.zeros(n, np.uint8), pos=np.zeros((n, 3), F32), view_dir=np.zeros((n, 3), F32), max_dist=np.zeros(n, F32),
                   min_dist=np.zeros(n, F32))
        for i, pid in self.slots[kf].items():
            p = self.pt[pid]
            if pid < 0 or p["bad"]:
                continue
            out["has_point"][i] = 1
            out["pos"][i], out["view_dir"][i], out["max_dist"][i], out["min_dist"][i] = p["pos"], p["view_dir"], p["max_dist"], p["min_dist"]
        return out

    def state(self):
        """everything the tests compare: slot -> point id per keyframe, observations, bad flags"""
        return ({k: sorted(v.items()) for k, v in self.slots.items()}, {i: sorted(p["obs"].items()) for i, p in self.pt.items()},
                {i: p["bad"] for i, p in self.pt.items()})


def view(rng, pts, base, centre, R, n, flip_bits=4, px_noise=0.4):
    Tcw, _, Ow = ts.pose(centre, R)
    fx, fy, cx, cy = (float(v) for v in CAM)
    pc = (Tcw[:3, :3].astype(np.float64) @ pts.T).T + Tcw[:3, 3]
    with np.errstate(all="ignore"):
        u = fx * pc[:, 0] / pc[:, 2] + cx
        v = fy * pc[:, 1] / pc[:, 2] + cy
    vis = np.flatnonzero((pc[:, 2] > 0.5) & (u > 2) & (u < W - 2) & (v > 2) & (v < H - 2))
    pid = rng.permutation(vis)[:n]
    m = len(pid)
    kps = np.zeros(m, KP_DTYPE)
    kps["x"] = (u[pid] + rng.normal(0, px_noise, m)).astype(F32)
    kps["y"] = (v[pid] + rng.normal(0, px_noise, m)).astype(F32)
    kps["size"], kps["class_id"] = 7.0, -1
    kps["octave"] = (pid * 31) % 8            # one octave per world point: every octave 0 .. 7 occurs, and a point keeps it across views
    desc = base[pid].copy()
    for i in range(m):
        for b in rng.integers(0, 256, rng.integers(0, flip_bits + 1)):
            desc[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return dict(kps=kps, desc=desc, Rcw=Tcw[:3, :3].copy(), tcw=Tcw[:3, 3].copy(), bounds=BOUNDS, centre=Ow, pid=pid)


def scene(seed=0, K=6, n=400, n_t=None, n_pts=None, include_cur=True, has_frac=0.7, side_frac=0.5):
    """-> dict(cur, targets, z, pts, model, target_kfs).  Targets move along the optical axis by +-0.08 m (beyond BL) or 0.01 m (inside),
    in turn, so all three octave-window cases occur from K = 3 on; target 0 is the current keyframe itself when include_cur (as in
    sTargetKfs, LocalMapping.cc:357).  A share of the duplicated points is dominated by far sideways observers: when such a point wins
    a replace and moves into cur's slot, it is no longer visible from the later targets."""
    rng = np.random.default_rng(seed)
    n_pts = n_pts or max(3 * n, 300)
    pts = np.stack([rng.uniform(-5, 5, n_pts), rng.uniform(-3.5, 3.5, n_pts), rng.uniform(4, 12, n_pts)], 1)
    base = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)
    cur = view(rng, pts, base, (0, 0, 0), None, n)
    n = len(cur["kps"])
    n_t = [n] * K if n_t is None else ([n_t] * K if np.isscalar(n_t) else list(n_t))
    model = MapModel()
    model.add_kf(CUR, cur["Rcw"], cur["tcw"], cur["centre"], cur["desc"])
    for f in range(5):
        model.add_kf(FAR0 + f, np.eye(3), np.zeros(3), (30 + f, 0, 6))
    model.add_kf(900, np.eye(3), np.zeros(3), (0.3, 0.1, 0))
    targets, target_kfs = [], []
    dz = [0.08, -0.08, 0.01]
    for k in range(K):
        if include_cur and k == 0:
            targets.append(cur)
            target_kfs.append(CUR)
            continue
        c = (rng.normal(0, 0.01), rng.normal(0, 0.01), dz[k % 3])
        t = view(rng, pts, base, c, ts.yaw(rng.normal(0, 0.002)), n_t[k])
        targets.append(t)
        target_kfs.append(1 + k)
        model.add_kf(1 + k, t["Rcw"], t["tcw"], t["centre"], t["desc"])
    z = np.array([tlc_z(t["Rcw"], t["tcw"], cur["Rcw"], cur["tcw"]) for t in targets], F32)

    # the points of cur's slots: ids 0 .. n - 1
    cur_of_pid = {}
    for i in range(n):
        if rng.random() >= has_frac:
            continue
        pid = int(cur["pid"][i])
        pos = (pts[pid] + rng.normal(0, 0.01, 3)).astype(F32)
        d = F32(np.linalg.norm(pos))
        model.add_point(i, pos, base[pid], max_dist=d * F32(1.004 if rng.random() < 0.15 else 1.5), min_dist=d * F32(0.6))
        model.set_slot(CUR, i, i)
        model.add_observation(i, CUR, i)
        if rng.random() < 0.3:
            model.add_observation(i, 900, 10000 + i)
        cur_of_pid[pid] = i
    # the points of the targets' slots: shared with cur, a duplicate of cur's (id 100000 + world point), its own (200000 + ..) or none
    for k, t in enumerate(targets):
        kid = target_kfs[k]
        if kid == CUR:
            continue
        for j, pid in enumerate(t["pid"]):
            pid, r = int(pid), rng.random()
            if pid in cur_of_pid:
                new = cur_of_pid[pid] if r < 0.25 else (100000 + pid if r < 0.65 else -1)
            else:
                new = 200000 + pid if r < 0.5 else -1
            if new < 0:
                continue
            if new not in model.pt:
                pos = (pts[pid] + rng.normal(0, 0.01, 3)).astype(F32)
                d = F32(np.linalg.norm(pos))
                model.add_point(new, pos, base[pid], max_dist=d * F32(1.5), min_dist=d * F32(0.6))
                if new < 200000 and rng.random() < side_frac:
                    for f in range(5):
                        model.add_observation(new, FAR0 + f, len(model.slots[FAR0 + f]))
                        model.set_slot(FAR0 + f, len(model.slots[FAR0 + f]), new)
            model.set_slot(kid, j, new)
            model.add_observation(new, kid, j)
    for pid in model.pt:
        model.update_normal_and_depth(pid)
    for i in list(model.slots[CUR]):   # some of cur's points look sideways from the start: not visible anywhere
        if rng.random() < 0.12:
            vd = model.pt[i]["view_dir"].astype(np.float64)
            model.pt[i]["view_dir"] = (ts.yaw(np.deg2rad(75)) @ vd).astype(F32)
    return dict(cur=cur, targets=targets, z=z, pts=model.slot_points(CUR, n), model=model, target_kfs=target_kfs)


def sequential_chain(orc, sc, model):
    """The reference's loop, the slow way: per target in order, visibility and search recomputed from the LIVE model for that one target
    (the restatement with one target), the match list in ascending i, processFuseMps with live isBad / getObsNum.  -> nFuse per target"""
    cur, n = sc["cur"], len(sc["cur"]["kps"])
    out = []
    for k, kf in enumerate(sc["target_kfs"]):
        live = model.slot_points(CUR, n)
        bi, bd, vis = fr.fuse_into_keyframes(orc, cur, live, [sc["targets"][k]], sc["z"][k:k + 1], CAM, BL, SF)
        v_ids = [model.slot(CUR, i) for i in range(n)]
        matches = [(int(bi[0][i]), i) for i in range(n) if live["has_point"][i] and vis[0][i] and bi[0][i] >= 0]
        f_ids = {q: model.slot(kf, q) for q, _ in matches}
        nf = 0
        for q, tr in matches:
            p1, p2 = f_ids[q], v_ids[tr]
            if p2 < 0 or model.is_bad(p2):
                continue
            if p1 < 0 or model.is_bad(p1):
                model.set_slot(kf, q, p2)
                model.add_observation(p2, kf, q)
                nf += 1
            elif p1 != p2:
                if model.n_obs(p1) >= model.n_obs(p2):
                    model.replace(p1, p2)
                else:
                    model.replace(p2, p1)
                nf += 1
        out.append(nf)
    return out


def restated(orc):
    """search_in hook of MatcherExt.fuseIntoKeyframes: the restatement in place of the device"""
    return lambda cur, pts, targets, z, cam, bl, sf, th, ratio, dist: fr.fuse_into_keyframes(orc, cur, pts, targets, z, cam, bl, sf, th, ratio, dist)


# ---- constructions for the device's edge cases ----------------------------------------------------------------------------------------
def _kf(kps, desc, centre=(0, 0, 0), bounds=BOUNDS):
    Tcw, _, Ow = ts.pose(centre)
    return dict(kps=kps, desc=desc, Rcw=Tcw[:3, :3].copy(), tcw=Tcw[:3, 3].copy(), bounds=np.asarray(bounds, F32), centre=Ow)


def _points_in_front(rng, kps):
    """a visible point behind every feature (depth 6 m along the feature's ray), except every third slot, which stays empty"""
    n = len(kps)
    fx, fy, cx, cy = (float(v) for v in CAM)
    pos = np.stack([(kps["x"] - cx) / fx * 6.0, (kps["y"] - cy) / fy * 6.0, np.full(n, 6.0)], 1).astype(F32)
    vd = pos / np.linalg.norm(pos, axis=1, keepdims=True)
    return dict(has_point=(np.arange(n) % 3 != 2).astype(np.uint8), pos=pos, view_dir=vd.astype(F32), max_dist=np.full(n, 20, F32),
                min_dist=np.full(n, 1, F32))


def dense_cell_scene(count, seed=0):
    """one target whose cell (col 3, row 2) holds exactly `count` features inside the octave window of the queries (plus others outside
    it, interleaved), and queries in that cell: the staging of 64-candidate chunks at 63 / 64 / 65 and beyond"""
    rng = np.random.default_rng(seed)
    m = count + 40
    kps = np.zeros(m, KP_DTYPE)
    kps["x"] = rng.uniform(3 * 64 + 20, 4 * 64 - 20, m).astype(F32)
    kps["y"] = rng.uniform(2 * 48 + 18, 3 * 48 - 18, m).astype(F32)
    octv = np.full(m, 6)
    octv[rng.permutation(m)[:count]] = 2
    kps["octave"] = octv
    desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    q = np.zeros(6, KP_DTYPE)
    q["x"] = rng.uniform(3 * 64 + 25, 4 * 64 - 25, 6).astype(F32)
    q["y"] = rng.uniform(2 * 48 + 20, 3 * 48 - 20, 6).astype(F32)
    q["octave"] = 2                                  # radius 3 * 1.44^2 = 6.2 px: the box stays inside the cell
    qd = desc[np.flatnonzero(octv == 2)[[0, 1, 62 % count, count - 1, count // 2, 5 % count]]].copy()
    qd[:, 0] ^= 1                                    # distance 1 to its source: accepted; the rest of the list decides the second best
    cur = _kf(q, qd)
    return dict(cur=cur, targets=[_kf(kps, desc)], z=np.array([0.0], F32), pts=_points_in_front(rng, q), in_window=count)


def border_scene(seed=0):
    """queries on the right / bottom border, at x == width (640, a multiple of 64: the reference would index one column past the grid)
    and outside the image, against targets with features in the border cells; every octave 0 .. 7 among the queries"""
    rng = np.random.default_rng(seed)
    m = 300
    kps = np.zeros(m, KP_DTYPE)
    kps["x"] = np.concatenate([rng.uniform(W - 60, W, 150), rng.uniform(0, W, 150)]).astype(F32)
    kps["y"] = np.concatenate([rng.uniform(0, H, 150), rng.uniform(H - 40, H, 150)]).astype(F32)
    kps["octave"] = rng.integers(0, 8, m)
    desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    xy = [(W, 100), (W, H), (W - 0.5, H - 0.5), (100, H), (W + 30, 50), (-20, -20), (0, 0), (W, 0)] + \
         [(float(kps["x"][j]), float(kps["y"][j])) for j in range(0, m, 7)]
    q = np.zeros(len(xy), KP_DTYPE)
    q["x"], q["y"] = np.array(xy, F32).T
    q["octave"] = np.arange(len(xy)) % 8
    qd = desc[rng.integers(0, m, len(xy))].copy()
    qd[:, 1] ^= 3
    return dict(cur=_kf(q, qd), targets=[_kf(kps, desc, (0, 0, 0.2)), _kf(kps[::-1].copy(), desc[::-1].copy(), (0, 0, -0.2)), _kf(kps, desc)],
                z=np.array([0.2, -0.2, 0.0], F32), pts=_points_in_front(rng, q))


def cut(sc, idx):
    """the same scene with only the features `idx` of the current keyframe (no model: the device tests compare tables only)"""
    idx = np.asarray(idx)
    cur = dict(sc["cur"], kps=sc["cur"]["kps"][idx].copy(), desc=sc["cur"]["desc"][idx].copy())
    return dict(cur=cur, targets=sc["targets"], z=sc["z"], pts={k: v[idx].copy() for k, v in sc["pts"].items()})


_CACHE = {}


def gpu_scene(name):
    """the seeded scenes of tests/test_gpu_fuse.py by name; tests/test_fuse_host.py asserts on each that the expected tables are not
    vacuous (matches in at least half of the targets, both visibility values, all three octave-window cases)"""
    if name in _CACHE:
        return _CACHE[name]
    if name == "k3":
        sc = scene(11, K=3, n=300, include_cur=False)
    elif name.startswith("n"):           # n1 / n63 / n64 / n65: the first features of k3's current keyframe (n1: one that matches twice)
        m = int(name[1:])
        sc = cut(gpu_scene("k3"), [N1_FEATURE] if m == 1 else np.arange(m))
    elif name == "k64":
        sc = scene(12, K=64, n=65, n_t=90, n_pts=300)
    elif name == "mixed":
        sc = scene(13, K=4, n=300, n_t=[500, 0, 1, 500], n_pts=1500, include_cur=False)
    elif name == "mid":
        sc = scene(14, K=6, n=400)
    elif name == "full":
        sc = scene(15, K=61, n=2000, n_pts=6000)
    else:
        raise KeyError(name)
    _CACHE[name] = sc
    return sc


GPU_SCENES = ["k3", "n1", "n63", "n64", "n65", "k64", "mixed", "mid", "full"]
N1_FEATURE = 25    # of k3: accepted in all three targets, visible from two of them


def write_dropin_input(sc, path, conn):
    """the scene's map as text for tests/cpp/test_fuse_dropin.cpp: keyframes (the current one first), covisibility lists `conn`
    {keyframe id: [ids, strongest first]}, points and slots.  Points of the targets alone (ids >= 100000) are in the map only when their
    id is a multiple of 3, so the forward fuse leaves most duplicates to the inverse fuses."""
    m = sc["model"]
    f = lambda v: repr(float(v))  # noqa: E731
    arrays = {CUR: sc["cur"]}
    arrays.update({kid: t for kid, t in zip(sc["target_kfs"], sc["targets"])})
    ids = [CUR] + sorted(k for k in m.kf if k != CUR)
    lines = [" ".join(f(v) for v in CAM) + " " + f(BL), f"{len(SF)} " + " ".join(f(v) for v in SF), str(len(ids))]
    for kid in ids:
        k, a = m.kf[kid], arrays.get(kid)
        n = 0 if a is None else len(a["kps"])
        lines.append(f"{kid} {n} " + " ".join(f(v) for v in np.concatenate([k["centre"], k["Rcw"].reshape(9), k["tcw"].reshape(3), k["bounds"]])))
        for i in range(n):
            kp = a["kps"][i]
            lines.append(f"{f(kp['x'])} {f(kp['y'])} {int(kp['octave'])} " + " ".join(str(int(b)) for b in a["desc"][i]))
    for kid in ids:
        c = conn.get(kid, [])
        lines.append(f"{kid} {len(c)} " + " ".join(str(x) for x in c))
    lines.append(str(len(m.pt)))
    for pid, p in sorted(m.pt.items()):
        inmap = 1 if pid < 100000 or pid % 3 == 0 else 0
        obs = " ".join(f"{k} {ft}" for k, ft in sorted(p["obs"].items()))
        lines.append(f"{pid} " + " ".join(f(v) for v in np.concatenate([p["pos"], p["view_dir"], [p["max_dist"], p["min_dist"]]])) + f" {inmap} " +
                     " ".join(str(int(b)) for b in p["desc"]) + f" {len(p['obs'])} {obs}")
    for kid in ids:
        s = sorted(m.slots[kid].items())
        lines.append(f"{kid} {len(s)} " + " ".join(f"{ft} {pid}" for ft, pid in s))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
