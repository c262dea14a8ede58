"""Scenes for the forward-fuse tests (orbfe_fuse_points_into_keyframes_stored): seeded keyframes that see one cloud through
differing bounds with a list of map points, one scene placed by hand whose every point is there for a reason, single-window scenes with a
chosen candidate list, and a small loop (LoopModel, loop_scene) in which a MapPoint::replace changes a surviving loop point's view
direction and descriptor.  A keyframe and the points are the dicts of fuse_points_restatement.py."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tri_scenes as ts  # noqa: E402
import fuse_points_restatement as fr  # noqa: E402
from fuse_scenes import MapModel, hamming  # noqa: E402
from sim3_search_scenes import flipped, ray, rot  # noqa: E402
from orb_slam2_ros2_amd._lib import KP_DTYPE  # noqa: E402

F32 = np.float32
CAM, SF, W, H = ts.CAM, ts.SF, ts.W, ts.H
IMAGE = (0.0, float(W), 0.0, float(H))
BOUNDS = [(-12.5, 655.0, -9.25, 492.5), IMAGE, (4.0, 630.5, 6.0, 470.25), (-30.0, 700.0, -20.0, 520.0)]   # none of them every keyframe's
TH, RATIO = 4.0, 0.8                      # LoopClosing::correctLoop's fuse (src/LoopClosing.cc:515-517)
POINT_KEYS = ("usable", "pos", "view_dir", "max_dist", "min_dist", "desc")


def keyframe(kps, desc, centre=(0, 0, 0), R=None, bounds=IMAGE):
    Tcw = ts.pose(centre, R)[0].astype(np.float64)
    return dict(kps=kps, desc=np.ascontiguousarray(desc, np.uint8), bounds=tuple(float(b) for b in bounds), Rcw=Tcw[:3, :3].astype(F32),
                tcw=Tcw[:3, 3].astype(F32), centre=np.asarray(centre, F32))


def make_kps(x, y, octave):
    kps = np.zeros(len(x), KP_DTYPE)
    kps["x"], kps["y"], kps["octave"] = x, y, octave
    kps["size"], kps["class_id"] = 7.0, -1
    return kps


def poses(kfs):
    return [(kf["Rcw"], kf["tcw"]) for kf in kfs]


def take(pts, idx):
    """the points `idx` of a list"""
    idx = np.asarray(idx, np.int64)
    return {k: np.asarray(pts[k])[idx].copy() for k in POINT_KEYS}


def noisy(rng, desc, max_bits):
    d = np.array(desc, np.uint8)
    for b in rng.integers(0, 256, rng.integers(0, max_bits + 1)):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


# ---- seeded ------------------------------------------------------------------------------------------------------------------------------
def seeded(seed=0, K=4, m=300, n=300, n_levels=8, n_pts=None):
    """K keyframes around the origin, turned by up to half a radian so that their fields of view overlap only in part, each with bounds of
    its own; m map points of the cloud they look at.  A world point keeps one octave in every view, and the distance range of its map point
    is centred on it.  -> dict(kfs, pts, sf)"""
    rng = np.random.default_rng(seed)
    n_pts = n_pts or max(2 * n, 500)
    cloud = np.stack([rng.uniform(-9, 9, n_pts), rng.uniform(-4, 4, n_pts), rng.uniform(5, 12, n_pts)], 1)
    base = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)
    octave = (np.arange(n_pts) * 31) % n_levels
    fx, fy, cx, cy = (float(c) for c in CAM)
    kfs = []
    for k in range(K):
        centre = (rng.normal(0, 0.15), rng.normal(0, 0.1), rng.normal(0, 0.15))
        R = rot(rng.normal(0, 0.02), (k % 4 - 1.5) * 0.3 + rng.normal(0, 0.02), rng.normal(0, 0.02))
        b = BOUNDS[k % len(BOUNDS)]
        Tcw = ts.pose(centre, R)[0].astype(np.float64)
        pc = (Tcw[:3, :3] @ cloud.T).T + Tcw[:3, 3]
        u, v = fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy
        vis = np.flatnonzero((pc[:, 2] > 0.5) & (u > b[0] + 1) & (u < b[1] - 1) & (v > b[2] + 1) & (v < b[3] - 1))
        pid = rng.permutation(vis)[:n]
        kps = make_kps((u[pid] + rng.normal(0, 0.4, len(pid))).astype(F32), (v[pid] + rng.normal(0, 0.4, len(pid))).astype(F32), octave[pid])
        kf = keyframe(kps, np.stack([noisy(rng, base[p], 6) for p in pid]) if len(pid) else np.zeros((0, 32), np.uint8), centre, R, b)
        kf["pid"] = pid
        kfs.append(kf)
    sel = rng.permutation(n_pts)[:m] if m <= n_pts else rng.integers(0, n_pts, m)       # (a long list: world points repeat)
    pos = (cloud[sel] + rng.normal(0, 0.01, (m, 3))).astype(F32)
    d = np.linalg.norm(pos, axis=1)
    vd = pos / d[:, None]
    turn = rng.random(m)
    for j in np.flatnonzero(turn < 0.25):                                               # seen from the side, some past 60 degrees
        vd[j] = rot(0, np.deg2rad(rng.uniform(40, 80)) * rng.choice([-1, 1]), 0) @ vd[j]
    vd[turn > 0.95] *= -1
    tight = rng.random(m) < 0.12
    pts = dict(usable=(rng.random(m) < 0.85).astype(np.uint8), pos=pos, view_dir=vd.astype(F32),
               max_dist=(d * np.where(tight, 0.99, 1.2 ** octave[sel] * rng.uniform(0.97, 1.03, m))).astype(F32),
               min_dist=(d * rng.uniform(0.2, 0.5, m)).astype(F32), desc=np.stack([noisy(rng, base[p], 6) for p in sel]))
    return dict(kfs=kfs, pts=pts, sf=SF[:n_levels])


# ---- one window with a chosen candidate list ---------------------------------------------------------------------------------------------
def window(n_cand, dists=None, at=(352.0, 264.0), bounds=IMAGE, seed=5, n_decoys=40):
    """One keyframe (identity pose) with exactly n_cand features of octaves 0 .. 2 around `at`, all in one grid cell when `at` is a cell's
    centre (list order = index order), between decoys of octaves 4 .. 7; one point that projects to `at`, is seen head-on (radius 2.5 * th *
    1.44) and predicts level 1.  dists[k]: the Hamming distance of candidate k (default 20 + k % 30)."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, 32, dtype=np.uint8)
    rows, k = [], 0
    for slot in rng.permutation(n_cand + n_decoys):
        ang, r = rng.uniform(0, 2 * np.pi), rng.uniform(0, 6.0)
        x, y = at[0] + r * np.cos(ang), at[1] + r * np.sin(ang)
        if slot < n_cand:
            d = (20 + k % 30) if dists is None else dists[k]
            rows.append((x, y, int(rng.integers(0, 3)), flipped(q, rng.permutation(256)[:d])))
            k += 1
        else:
            rows.append((x, y, int(rng.integers(4, 8)), flipped(q, [1])))
    kf = keyframe(make_kps([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]), np.stack([r[3] for r in rows]), bounds=bounds)
    p = ray(at[0], at[1], 6.0)
    dist = float(np.linalg.norm(p))
    pts = dict(usable=np.ones(1, np.uint8), pos=np.array([p], F32), view_dir=np.array([p / dist], F32), max_dist=np.array([dist * 1.2], F32),
               min_dist=np.array([dist * 0.5], F32), desc=q[None].copy())
    return dict(kfs=[kf], pts=pts, sf=SF, th=3.0)


# ---- by hand -----------------------------------------------------------------------------------------------------------------------------
def hand():
    """One keyframe with the wide bounds and an identity pose; every reason a pair can end for, both radius classes with cosTheta just on
    either side of 0.998f, levels 0 and 7.  Every case has a grid cell of its own (cells are 64 x 48 pixels, and findFeaturesInArea returns
    whole cells).  -> dict(kfs, pts, sf, notes {name: point index}, feats {name: feature index})"""
    rng = np.random.default_rng(31)
    rnd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)  # noqa: E731
    b = BOUNDS[0]
    feats, rows, notes, fnotes = [], [], {}, {}
    spots = iter([(64.0 * i + 32, 48.0 * j + 24) for j in range(1, 9) for i in range(1, 9)])

    def feature(x, y, octave, desc, name=None):
        feats.append((x, y, octave, np.array(desc, np.uint8)))
        if name:
            fnotes[name] = len(feats) - 1

    def point(name, cam_xyz, level, desc, usable=1, mx_f=None, mn_f=0.5, tilt=0.0):
        Y = np.asarray(cam_xyz, np.float64)
        dist = np.linalg.norm(Y)
        r = Y / dist
        side = np.cross(r, (0.0, 1.0, 0.0))
        vd = np.cos(tilt) * r + np.sin(tilt) * side / np.linalg.norm(side)       # `tilt` radians off the ray
        rows.append((usable, Y, vd, dist * (1.2 ** level if mx_f is None else mx_f), dist * mn_f, np.array(desc, np.uint8)))
        notes[name] = len(rows) - 1

    u, v = next(spots)
    q = rnd()
    feature(u + 1, v, 1, flipped(q, [3]))
    point("unusable", ray(u, v, 6), 1, q, usable=0)
    point("behind", (0.2, 0.1, -3.0), 1, rnd())
    u, v = next(spots)
    q = rnd()
    feature(u + 1, v, 1, flipped(q, [3]))
    point("distance_max", ray(u, v, 6), 1, q, mx_f=0.9)
    point("distance_min", ray(u, v, 6), 1, q, mx_f=2.0, mn_f=1.1)
    point("outside_u_max", ray(b[1] + 5, 200, 6), 1, rnd())
    point("outside_u_min", ray(b[0] - 5, 200, 6), 1, rnd())
    point("outside_v_max", ray(300, b[3] + 5, 6), 1, rnd())
    point("outside_v_min", ray(300, b[2] - 5, 6), 1, rnd())
    u, v = next(spots)
    q = rnd()
    feature(u + 1, v, 1, flipped(q, [3]))
    point("angle", ray(u, v, 6), 1, q, tilt=np.deg2rad(61))
    point("angle_inside", ray(u + 1, v, 6), 1, q, tilt=np.deg2rad(59))
    u, v = next(spots)
    point("empty", ray(u, v, 6), 1, rnd())
    u, v = next(spots)
    q = rnd()
    feature(u + 2, v, 5, q)                                                   # right place, octave outside 0 .. 2
    point("empty_octave", ray(u, v, 6), 1, q)
    u, v = next(spots)
    q = rnd()
    feature(u + 1, v, 1, flipped(q, range(0, 50)))                            # exactly the threshold: rejected (<)
    point("threshold", ray(u, v, 6), 1, q)
    u, v = next(spots)
    q = rnd()
    feature(u + 1, v, 1, flipped(q, range(0, 49)), "threshold_minus_one")
    point("threshold_minus_one", ray(u, v, 6), 1, q)
    u, v = next(spots)
    q = rnd()
    feature(u + 1, v, 1, flipped(q, range(0, 8))), feature(u - 1, v, 1, flipped(q, range(10, 20)))     # 8 / 10 = 0.8: rejected (<)
    point("ratio", ray(u, v, 6), 1, q)
    u, v = next(spots)
    q = rnd()
    feature(u + 1, v, 1, flipped(q, range(0, 7)), "ratio_inside"), feature(u - 1, v, 1, flipped(q, range(10, 20)))   # 0.7
    point("ratio_inside", ray(u, v, 6), 1, q)
    u, v = next(spots)
    q = rnd()
    feature(u + 1, v, 1, flipped(q, [3, 77]), "single")                       # one candidate: second = INT_MAX
    point("single", ray(u, v, 6), 1, q)
    # levels 0 and 7: windows 0 .. 1 and 6 .. 7 (clamped)
    u, v = next(spots)
    q = rnd()
    feature(u, v + 1, 2, q), feature(u + 1, v, 0, flipped(q, [1, 2, 3]), "level0")
    point("level0", ray(u, v, 6), 0, q, mx_f=1.05)
    u, v = next(spots)
    q = rnd()
    feature(u, v + 1, 5, q), feature(u + 1, v, 7, flipped(q, [1, 2, 3]), "level7")
    point("level7", ray(u, v, 6), 7, q, mx_f=1.2 ** 9)                        # predicted 9, clamped to 7
    # the radius classes at level 0, th = 4: 2.5 * 4 = 10 px against 4 * 4 = 16 px.  The point sits 12 px left of a cell boundary and
    # the only feature that fits 3 px right of it: the narrow window ends in the point's own cell, the wide one reaches the next
    half = np.arccos(0.998)
    for name, tilt in (("narrow", half - 1e-4), ("wide", half + 1e-4)):
        u, v = next(spots)
        next(spots)
        q = rnd()
        feature(u + 32 + 3, v, 0, flipped(q, [5]), name)
        point(name, ray(u + 32 - 12, v, 6), 0, q, mx_f=1.05, tilt=tilt)
    # a feature outside the image, inside the bounds
    q = rnd()
    feature(-8.0, -5.0, 1, flipped(q, [9]), "outside_image")
    point("outside_image", ray(-6.0, -4.0, 6), 1, q)
    kf = keyframe(make_kps([f[0] for f in feats], [f[1] for f in feats], [f[2] for f in feats]), np.stack([f[3] for f in feats]), bounds=b)
    pts = dict(usable=np.array([r[0] for r in rows], np.uint8), pos=np.array([r[1] for r in rows], F32), view_dir=np.array([r[2] for r in rows], F32),
               max_dist=np.array([r[3] for r in rows], F32), min_dist=np.array([r[4] for r in rows], F32), desc=np.stack([r[5] for r in rows]))
    return dict(kfs=[kf], pts=pts, sf=SF, notes=notes, feats=fnotes)


# ---- a loop: the replay of MatcherExt.fusePointsIntoKeyframes against the plain sequential loop -------------------------------------------
class LoopModel(MapModel):
    """fuse_scenes.MapModel with what the forward fuse reads besides: isInMap, MapPoint::updateDescriptor in replace (the observation whose
    descriptor has the least median distance to the others, the first such; src/MapPoint.cc:229), the live arrays of a list of points and
    the good points a keyframe holds."""

    def __init__(self):
        super().__init__()
        self.not_in_map = set()

    def in_map(self, pid):
        return pid not in self.not_in_map

    def pose(self, kf):
        return self.kf[kf]["Rcw"], self.kf[kf]["tcw"]

    def held(self, kf):
        return set(p for p in self.slots[kf].values() if p >= 0 and not self.pt[p]["bad"])

    def update_descriptor(self, pid):
        p = self.pt[pid]
        ds = [self.kf[k]["desc"][f] for k, f in sorted(p["obs"].items()) if self.kf[k]["desc"] is not None]
        if not ds:
            return
        med = [sorted(hamming(a, b) for b in ds)[(len(ds) - 1) // 2] for a in ds]
        p["desc"] = np.array(ds[int(np.argmin(med))], np.uint8)

    def replace(self, keep, drop):
        d = self.pt[drop]
        d["bad"] = True
        obs, d["obs"] = d["obs"], {}
        for kf in sorted(obs):
            if kf in self.pt[keep]["obs"]:
                continue
            self.slots[kf][obs[kf]] = keep
            self.add_observation(keep, kf, obs[kf])
        self.update_descriptor(keep)
        self.update_normal_and_depth(keep)

    def point_arrays(self, pids):
        """the arrays of orbfe_sim3_points for the points `pids` as they are now (-1: a null pointer)"""
        m = len(pids)
        out = dict(usable=np.zeros(m, np.uint8), pos=np.zeros((m, 3), F32), view_dir=np.zeros((m, 3), F32), max_dist=np.zeros(m, F32),
                   min_dist=np.zeros(m, F32), desc=np.zeros((m, 32), np.uint8))
        for j, pid in enumerate(pids):
            if pid < 0:
                continue
            p = self.pt[pid]
            out["usable"][j] = 0 if p["bad"] or not self.in_map(pid) else 1
            out["pos"][j], out["view_dir"][j], out["max_dist"][j], out["min_dist"][j], out["desc"][j] = (p["pos"], p["view_dir"], p["max_dist"],
                                                                                                       p["min_dist"], p["desc"])
        return out


SIDE0, LOOP_KF = 1000, 500     # keyframes that only observe: five to the side of the scene, and the loop keyframe the loop points come from


def loop_scene(seed=3, K=3, n_pts=60):
    """K target keyframes (ids 1 .. K) at almost one pose, a loop keyframe that observes every loop point (ids 0 .. n_pts - 1, one per
    world point), and in the targets' slots: duplicates (ids 1000 + ..) of the loop points, observed besides by five keyframes off to the
    side whose features carry ANOTHER descriptor of the world point.  When the fuse into target 1 replaces such a duplicate by its loop
    point, the loop point takes over the side observations: its view direction turns (for `far` points past 60 degrees: no longer in
    vision of targets 2 ..; for `near` points it stays in vision) and its descriptor becomes the side descriptor, which in the later
    targets is closest to another feature (each world point has two features there, one per descriptor).  A few loop points are held by a
    target from the start, one is bad, one is not in the map, one entry is a null pointer.
    -> dict(model, kfs {id: keyframe dict}, target_kfs, point_ids)"""
    rng = np.random.default_rng(seed)
    cloud = np.stack([rng.uniform(-2.5, 2.5, n_pts), rng.uniform(-1.8, 1.8, n_pts), rng.uniform(5, 7, n_pts)], 1)
    d_loop = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)
    d_side = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)
    kind = np.array(["far", "near", "plain"])[np.arange(n_pts) % 3]       # plain: no duplicate anywhere
    fx, fy, cx, cy = (float(c) for c in CAM)
    model, kfs = LoopModel(), {}
    model.add_kf(LOOP_KF, np.eye(3), np.zeros(3), (0.0, 0.0, 0.0), d_loop.copy())
    side_x = {"far": 40.0, "near": 2.5}
    for f in range(5):
        for kd in ("far", "near"):
            kid = SIDE0 + 10 * f + (0 if kd == "far" else 1)
            model.add_kf(kid, np.eye(3), np.zeros(3), (side_x[kd] + 0.1 * f, 0.0, 6.0 if kd == "far" else 0.0), d_side.copy())
    for k in range(1, K + 1):
        centre = (0.02 * k, -0.01 * k, 0.01 * k)
        Tcw = ts.pose(centre)[0].astype(np.float64)
        pc = cloud + Tcw[:3, 3]
        u, v = fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy
        # feature 2 i: the loop descriptor's, feature 2 i + 1: the side descriptor's, a pixel apart
        x = np.stack([u - 0.5, u + 0.5], 1).reshape(-1)
        y = np.stack([v, v], 1).reshape(-1)
        desc = np.stack([np.stack([flipped(d_loop[i], [k]), flipped(d_side[i], [k + 8])]) for i in range(n_pts)]).reshape(-1, 32)
        kf = keyframe(make_kps(x.astype(F32), y.astype(F32), np.ones(2 * n_pts, np.int32)), desc, centre, None, BOUNDS[k % len(BOUNDS)])
        kfs[k] = kf
        model.add_kf(k, kf["Rcw"], kf["tcw"], kf["centre"], kf["desc"], kf["bounds"])
    for i in range(n_pts):
        dist = F32(np.linalg.norm(cloud[i]))
        model.add_point(i, cloud[i], d_loop[i], max_dist=dist * F32(1.2), min_dist=dist * F32(0.5))
        model.add_observation(i, LOOP_KF, i)
        model.set_slot(LOOP_KF, i, i)
        if kind[i] == "plain":
            continue
        dup = 1000 + i
        model.add_point(dup, cloud[i] + 0.005, d_side[i], max_dist=dist * F32(1.2), min_dist=dist * F32(0.5))
        model.add_observation(dup, 1, 2 * i), model.set_slot(1, 2 * i, dup)      # in target 1 it sits on the LOOP descriptor's feature
        for f in range(5):
            kid = SIDE0 + 10 * f + (0 if kind[i] == "far" else 1)
            model.add_observation(dup, kid, i), model.set_slot(kid, i, dup)
    for pid in model.pt:
        model.update_normal_and_depth(pid)
    # points a target holds already, a bad one, one outside the map, a null pointer
    plain = [i for i in range(n_pts) if kind[i] == "plain"]
    for k, i in ((2, plain[0]), (K, plain[1])):
        model.add_observation(i, k, 2 * i), model.set_slot(k, 2 * i, i)
    model.pt[plain[2]]["bad"] = True
    model.not_in_map.add(plain[3])
    point_ids = list(range(n_pts))
    point_ids.insert(7, -1)
    return dict(model=model, kfs=kfs, target_kfs=list(range(1, K + 1)), point_ids=point_ids, kind=kind, held=[(2, plain[0]), (K, plain[1])])


def restated(orc, scene):
    """search_in hook of MatcherExt.fusePointsIntoKeyframes: the restatement in place of the device"""
    def search(kf_names, kf_poses, pts, cam, sf, th, ratio, dist_threshold):
        kfs = [dict(scene["kfs"][k], Rcw=p[0], tcw=p[1]) for k, p in zip(kf_names, kf_poses)]
        t = fr.tables(orc, kfs, pts, cam, sf, th, ratio, dist_threshold)
        return t["best_idx"], t["best_dist"]
    return search


def sequential_loop(orc, scene, model, th=TH, ratio=RATIO, dist_threshold=50, bLoop=True):
    """`for pkf in targets: matcher.fuse(pkf, points, map, bLoop, th)` the slow way: per target in order everything recomputed from the LIVE
    model (src/ORBMatcher.cc:682-707) -> nFuse per target"""
    ids, out = scene["point_ids"], []
    for kf in scene["target_kfs"]:
        held = model.held(kf)
        v = [pid for pid in ids if pid not in held]                                         # vMapPoints (:695-701)
        pose = model.pose(kf)
        t = fr.tables(orc, [dict(scene["kfs"][kf], Rcw=pose[0], tcw=pose[1])], model.point_arrays(v), CAM, SF, th, ratio, dist_threshold)
        matches = [(int(t["best_idx"][0][p]), p) for p in range(len(v)) if t["best_idx"][0][p] >= 0]
        f_ids = {q: model.slot(kf, q) for q, _ in matches}                                  # fMapPoints (:703): a snapshot
        nf = 0
        for q, p in matches:
            p1, p2 = f_ids[q], v[p]
            if p2 < 0 or model.is_bad(p2):
                continue
            if p1 < 0 or model.is_bad(p1):
                model.set_slot(kf, q, p2)
                model.add_observation(p2, kf, q)
                nf += 1
            elif p1 != p2:
                keep, drop = (p2, p1) if bLoop or model.n_obs(p1) < model.n_obs(p2) else (p1, p2)
                model.replace(keep, drop)
                nf += 1
        out.append(nf)
    return out


def write_dropin_input(scene, path):
    """the loop scene's map as text for tests/cpp/test_loopfuse_dropin.cpp, in the format of fuse_scenes.write_dropin_input (the loader is
    test_fuse_dropin.cpp's): keyframes with their features (those that only observe have none), empty covisibility lists, points and slots.
    The format has no bad flag: a bad point is left out, and the slots that hold it stay empty."""
    m = scene["model"]
    f = lambda v: repr(float(v))  # noqa: E731
    ids = sorted(m.kf)
    lines = [" ".join(f(v) for v in CAM) + " " + f(0.05), f"{len(SF)} " + " ".join(f(v) for v in SF), str(len(ids))]
    for kid in ids:
        k, a = m.kf[kid], scene["kfs"].get(kid)
        n = 0 if a is None else len(a["kps"])
        lines.append(f"{kid} {n} " + " ".join(f(v) for v in np.concatenate([k["centre"], np.asarray(k["Rcw"]).reshape(9), np.asarray(k["tcw"]).reshape(3),
                                                                           np.asarray(k["bounds"], F32)])))
        for i in range(n):
            kp = a["kps"][i]
            lines.append(f"{f(kp['x'])} {f(kp['y'])} {int(kp['octave'])} " + " ".join(str(int(b)) for b in a["desc"][i]))
    lines += [f"{kid} 0" for kid in ids]
    good = {pid: p for pid, p in sorted(m.pt.items()) if not p["bad"]}
    lines.append(str(len(good)))
    for pid, p in good.items():
        obs = " ".join(f"{k} {ft}" for k, ft in sorted(p["obs"].items()))
        lines.append(f"{pid} " + " ".join(f(v) for v in np.concatenate([p["pos"], p["view_dir"], [p["max_dist"], p["min_dist"]]])) +
                     f" {1 if m.in_map(pid) else 0} " + " ".join(str(int(b)) for b in p["desc"]) + f" {len(p['obs'])} {obs}")
    for kid in ids:
        sl = sorted((ft, pid) for ft, pid in m.slots[kid].items() if pid in good)
        lines.append(f"{kid} {len(sl)} " + " ".join(f"{ft} {pid}" for ft, pid in sl))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
