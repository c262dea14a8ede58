"""Scenes for orbfe_track_motion_model_slots, built on the CPU: two frames that really move.  One synthetic stereo pair is
drawn 16 pixels wider and 8 higher than the frame and cropped at two offsets (2, 1) pixels apart: the last and the current pair, both
extracted by the oracle.  The map points of the last frame sit at its stereo depth (a drawn one where the matcher found none) under a true
last pose; the true current pose is that pose turned by the small rotation which shifts the image by the crop's offset, the predicted
pose a few centimetres and a fraction of a degree off it.

The builder's arguments say what each last-frame feature holds:
  in_map   a good point that is in the map (flags 3), at the true position with a little noise
  local    a good point that is not in the map (flags 1)
  off      a good in-map point metres off: matched, thrown out by the optimisation
  bad      a point flagged bad (flags 0, its id / position garbage that must not be read)
every other feature is null; with last_pair >= 0 the null and the bad ones become temporaries where the depth is >= 0, with
last_pair = -1 the query count is exactly the number of good points."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reloc_refine_restatement as rr  # noqa: E402
import track_motion_restatement as tm  # noqa: E402
from reloc_refine_scenes import INV_SIGMA2, SIGMA2, quat_to_R  # noqa: E402

from orb_slam2_ros2_amd import synth  # noqa: E402

BASELINE = 0.537166
# the two geometries: the KITTI-shaped frame (2000 features: two strides of the 1024-thread loops) and a small one (500: one stride)
GEOM = {
    "kitti": dict(W=1241, H=376, NF=2000, cam=(718.856, 718.856, 607.1928, 185.2157, 718.856 * BASELINE), seed=5),
    "small": dict(W=640, H=480, NF=500, cam=(500.0, 500.0, 320.0, 240.0, 500.0 * BASELINE), seed=6),
}
OFF_LAST, OFF_CUR = (6, 3), (8, 4)      # the crops' origins (x, y): a feature of the last frame lies (2, 1) pixels further left / up now
SHIFT = (OFF_CUR[0] - OFF_LAST[0], OFF_CUR[1] - OFF_LAST[1])

_frames = {}


def images(geom):
    """-> ((last left, last right), (current left, current right)), contiguous crops of one drawn pair"""
    g = GEOM[geom]
    L, R = synth.stereo_pair(g["seed"], g["W"] + 16, g["H"] + 8)
    crop = lambda im, o: np.ascontiguousarray(im[o[1]:o[1] + g["H"], o[0]:o[0] + g["W"]])
    return (crop(L, OFF_LAST), crop(R, OFF_LAST)), (crop(L, OFF_CUR), crop(R, OFF_CUR))


def frames(orc, geom):
    """the oracle's stereo frames of the last and the current pair -> (last, current), computed once and left unchanged"""
    if geom not in _frames:
        g = GEOM[geom]
        last, cur = images(geom)
        f = lambda p: orc.stereo_frame(p[0], p[1], n_features=g["NF"], fx=g["cam"][0], bf=g["cam"][4])
        _frames[geom] = (f(last), f(cur))
    return _frames[geom]


def _poses(g, dz):
    """-> (true last pose (R, t), predicted current pose (R, t)) in float64; dz: the predicted camera centre moved along its z axis"""
    q = np.array([0.01, -0.02, 0.005, 1.0]); q /= np.linalg.norm(q)
    Rl, tl = quat_to_R(q), np.array([0.05, -0.02, 0.1])
    a, b = SHIFT[0] / g["cam"][0], SHIFT[1] / g["cam"][1]
    Ry = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    Rrel = Rx @ Ry                                       # turns a point of the last camera frame into the current one: u -> u - 2, v -> v - 1
    Rc, tc = Rrel @ Rl, Rrel @ tl
    dq = np.array([0.0015, -0.001, 0.001, 1.0]); dq /= np.linalg.norm(dq)
    Rp = quat_to_R(dq) @ Rc
    tp = quat_to_R(dq) @ tc + np.array([0.03, -0.02, 0.04]) - np.array([0.0, 0.0, dz])
    return (Rl, tl), (Rp, tp)


def build(orc, geom="kitti", in_map=(), local=(), off=(), bad=(), last_pair=1, pair=0, dz=0.0, noise=0.01, rng_seed=1, ids_from=1000):
    """-> the scene dict of track_motion_restatement.py, plus what the device call takes: pair / last_pair, last_ids, the store's rows
    (store_ids, store_pos).  in_map / local / off / bad: arrays of last-frame feature indices."""
    g = GEOM[geom]
    NF = g["NF"]
    last, cur = frames(orc, geom)
    rng = np.random.default_rng(rng_seed)
    lk, ld, ck, cd = last["lk"], last["ld"], cur["lk"], cur["ld"]
    n_l, n_c = len(lk), len(ck)
    (Rl, tl), (Rp, tp) = _poses(g, dz)
    fx, fy, cx, cy = g["cam"][:4]
    dp = last["depth"][:n_l]
    depth = np.where(dp > 0, dp, rng.uniform(4, 30, n_l))
    pc = np.stack([(lk["x"] - cx) / fx * depth, (lk["y"] - cy) / fy * depth, depth], 1)
    Xw = (pc - tl) @ Rl                                                  # Rl^T (pc - tl)
    in_map, local, off, bad = (np.asarray(x, np.int64).reshape(-1) for x in (in_map, local, off, bad))
    flags = np.zeros(NF, np.uint8)
    flags[in_map] = 3
    flags[local] = 1
    flags[off] = 3
    pos = np.zeros((NF, 3), np.float32)
    good = np.concatenate([in_map, local])
    pos[good] = (Xw[good] + rng.normal(0, noise, (len(good), 3))).astype(np.float32)
    pos[off] = (Xw[off] + rng.uniform(2.0, 5.0, (len(off), 3)) * rng.choice([-1.0, 1.0], (len(off), 3))).astype(np.float32)
    pos[bad] = np.float32(1e6)                                           # must not be read
    ids = np.full(NF, 0xFFFFFFFFFFFF, np.uint64)                         # an id no store holds: must not be read where bit 0 is clear
    held = np.flatnonzero(flags & 1)
    ids[held] = ids_from + held.astype(np.uint64)
    ru = l_depth = None
    if pair >= 0:
        ru = np.full(NF, -1.0)
        ru[:n_c] = cur["right_u"][:n_c]
    if last_pair >= 0:
        l_depth = np.full(NF, -1.0)
        l_depth[:n_l] = dp
    Rwc = Rl.T
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    return dict(geom=geom, nf=NF, kps=ck, desc=cd, n_kp=n_c, right_u=ru, l_kps=lk, l_desc=ld, l_n=n_l, l_depth=l_depth, last_flags=flags,
                last_pos=pos, last_ids=ids, store_ids=ids[held].copy(), store_pos=pos[held].copy(), pair=pair, last_pair=last_pair,
                Rcw=f32(Rp).reshape(9), tcw=f32(tp), last_Rcw=f32(Rl).reshape(9), last_tcw=f32(tl), last_Rwc=f32(Rwc).reshape(9),
                last_twc=f32(-Rwc @ tl), cam=g["cam"], bounds=(0.0, float(g["W"]), 0.0, float(g["H"])), baseline=BASELINE, sigma2=SIGMA2,
                inv_sigma2=INV_SIGMA2)


def restate(orc, s, **kw):
    return tm.track(orc, s, **kw)


def margins(orc, s, o):
    """the smallest relative distance of an edge's chi2 from its threshold at the restated estimate (inf without an optimisation)"""
    if o["n_edges"] == 0:
        return np.inf
    _, c2, th = tm.chi2(s, o["q"], o["assigned"], o["pose_se3"])
    return float(np.abs(c2 / th - 1.0).min())


# ---- selecting features with the restatement --------------------------------------------------------------------------------------------
_pools = {}


def pools(orc, geom="kitti", th=15.0, th_second=30.0):
    """the last-frame features by what the restatement's searches do with them when every feature holds a good point (last_pair = -1):
      first   accepted by search 1 (a query's search 1 does not depend on the other queries: the frame arrives empty)
      quiet   those of `first` that search 2, with every feature of search 1 held, does not accept again
      cross   not accepted by a search 1 of th 0.01 (their counterpart lies in another grid cell) but accepted by one of th_second"""
    key = (geom, th, th_second)
    if key not in _pools:
        n_l = len(frames(orc, geom)[0]["lk"])
        s = build(orc, geom, in_map=np.arange(n_l), last_pair=-1)
        q = tm.queries(s, *tm.unproject(s))
        empty = np.full(s["nf"], -1, np.int32)
        r1 = tm.search(orc, s, q, empty, th, tm.DEFAULTS)
        r2 = tm.search(orc, s, q, r1["assigned"], th_second, tm.DEFAULTS)
        tiny = tm.search(orc, s, q, empty, 0.01, tm.DEFAULTS)
        wide = tm.search(orc, s, q, empty, th_second, tm.DEFAULTS)
        first = np.flatnonzero(r1["accepted"])
        _pools[key] = dict(first=first, quiet=np.flatnonzero(r1["accepted"] & (r2["accepted"] == 0)),
                           cross=np.flatnonzero((tiny["accepted"] == 0) & (wide["accepted"] == 1)), tiny=np.flatnonzero(tiny["accepted"]))
    return _pools[key]


def exact_matches(orc, want, **kw):
    """a scene of `want` in-map points whose restatement counts exactly `want` matches after both searches: features of pools()["quiet"],
    any that a second search still accepts replaced until none is.  Asserts the count and the chi-square margin."""
    pool = list(pools(orc)["quiet"][::7])
    for _ in range(50):
        sel = np.array(pool[:want])
        s = build(orc, in_map=sel, last_pair=-1, **kw)
        o = restate(orc, s)
        if o["n_matches"] == want:
            break
        again = set(np.flatnonzero(o["query_matches"] > 1).tolist())
        pool = [f for f in pool if f not in again]
    assert o["n_matches"] == want and (o["query_matches"][sel] == 1).all()
    assert margins(orc, s, o) > 0.01, "an edge within 1 % of its chi-square threshold"
    return s, o


def exact_in_map(orc, want, n=30, **kw):
    """a scene of n good points of which exactly `want` in-map ones are inliers at the end: all n are local first; the flags do not touch
    the searches or the optimisation, so `want` of the restated final inliers are then put in the map.  Asserts the count and the margin."""
    sel = pools(orc)["quiet"][3::11][:n]
    o = restate(orc, build(orc, local=sel, last_pair=-1, **kw))
    fin = o["final_assigned"][o["final_assigned"] >= 0]
    assert len(fin) >= want + 5
    chosen = fin[:want]
    s = build(orc, in_map=chosen, local=np.setdiff1d(sel, chosen), last_pair=-1, **kw)
    o = restate(orc, s)
    assert o["n_in_map"] == want and o["n_matches"] >= 20 and o["passes"] == 1
    assert margins(orc, s, o) > 0.01, "an edge within 1 % of its chi-square threshold"
    return s, o


def second_search(orc):
    """12 features search 1 (th 0.01: the query's own grid cell) accepts, 30 whose counterpart lies across a cell border: search 2
    (th 15) finds those.  -> (scene, parameters of the call)"""
    p = pools(orc, th_second=15.0)
    sel = np.concatenate([p["tiny"][5::40][:12], p["cross"][:30]])
    return build(orc, in_map=sel, last_pair=-1), dict(th=0.01, th_second=15.0)


SCENES = ("forward", "backward", "neither", "second", "few", "temp_inliers", "mono", "zero", "one", "all_temp")
BOUNDARY = {"matches_19": "REJECT_MATCHES", "matches_20": "ACCEPT", "in_map_9": "REJECT_INLIERS", "in_map_10": "ACCEPT"}
_scenes = {}


def scene(orc, name):
    """-> (scene, the restatement's result, parameters of the call), computed once per name, shared by the tests and left unchanged"""
    if name in _scenes:
        return _scenes[name]
    kw = {}
    n_l = len(frames(orc, "kitti")[0]["lk"])
    every = np.arange(n_l)
    if name in ("forward", "backward", "neither"):
        # the predicted camera centre 0.8 m ahead of / behind the last one (the baseline is 0.54 m), or 0.1 m: the octave windows differ
        dz = dict(forward=0.8, backward=-0.8, neither=0.1)[name]
        s = build(orc, in_map=every[::2], off=every[1::40], bad=every[3::40], dz=dz)
    elif name == "second":
        s, kw = second_search(orc)
    elif name == "few":               # eight points: too few after both searches
        s = build(orc, in_map=pools(orc)["quiet"][::9][:8], last_pair=-1)
    elif name == "temp_inliers":      # five in-map points among hundreds of temporaries: many inliers, rejected all the same
        s = build(orc, in_map=pools(orc)["quiet"][::9][:5])
    elif name == "mono":
        s = build(orc, in_map=every[::2], local=every[1::6], pair=-1)
    elif name == "zero":              # no point, no depth: no query
        s = build(orc, last_pair=-1)
    elif name == "one":
        s = build(orc, in_map=pools(orc)["quiet"][4:5], last_pair=-1)
        kw = dict(min_matches=1, min_inliers=1)
    elif name == "all_temp":          # last_flags all zero with depth: every query is a temporary
        s = build(orc)
    elif name.startswith("matches_"):
        s, o = exact_matches(orc, int(name.split("_")[1]))
        _scenes[name] = (s, o, kw)
        return _scenes[name]
    elif name.startswith("in_map_"):
        s, o = exact_in_map(orc, int(name.split("_")[2]))
        _scenes[name] = (s, o, kw)
        return _scenes[name]
    elif name == "small":             # the 640 x 480 geometry with 500 features: one stride of the 1024-thread loops
        n_s = len(frames(orc, "small")[0]["lk"])
        s = build(orc, "small", in_map=np.arange(n_s)[::2], off=np.arange(n_s)[1::30])
    else:
        raise KeyError(name)
    _scenes[name] = (s, restate(orc, s, **kw), kw)
    return _scenes[name]
