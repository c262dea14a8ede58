"""The forward fuse over stored keyframes (orbfe_fuse_points_into_keyframes_stored) restated on the CPU: the two tables
composed from the CPU oracle's single calls -- Oracle.project_map_points per keyframe (MapPoint::isInVision + predictLevel, the level then
clamped to n_levels - 1) and Oracle.search_in_area_ex on the keyframe's bounds (findFeaturesInArea + getBestMatch) -- with the radius, the
octave window and the acceptance test in numpy as frontend.ORBMatcher.searchByProjectionMapPoints does them, and a reason for every pair
that ends in -1.

A keyframe is dict(kps, desc, bounds (minU, maxU, minV, maxV), Rcw, tcw); the points are dict(usable [m], pos [m, 3], view_dir [m, 3],
max_dist [m], min_dist [m], desc [m, 32])."""
from __future__ import annotations

import numpy as np

F32 = np.float32
# why a pair has no match, in the order the tests run; "accepted" otherwise
REASONS = ("unusable", "behind", "distance", "outside", "angle", "empty", "threshold", "ratio")


def why_not_in_vision(pts, kf, cam):
    """The first test of MapPoint::isInVision (src/MapPoint.cc:141-171) that fails, per point, in map_point_dev.h's arithmetic (float
    products summed left to right, the translation added in double, sqrtf): "behind", "distance", "outside", "angle" or None."""
    X = np.asarray(pts["pos"], F32).reshape(-1, 3)
    D = np.asarray(pts["view_dir"], F32).reshape(-1, 3)
    R, t = np.asarray(kf["Rcw"], F32).reshape(3, 3), np.asarray(kf["tcw"], F32).reshape(3)
    fx, fy, cx, cy = (F32(c) for c in cam[:4])
    row = lambda A, r, x: ((A[r, 0] * x[:, 0]).astype(F32) + (A[r, 1] * x[:, 1]).astype(F32)).astype(F32) + (A[r, 2] * x[:, 2]).astype(F32)  # noqa: E731
    pc = [(row(R, r, X).astype(np.float64) + np.float64(t[r])).astype(F32) for r in range(3)]
    x, y, z = pc
    with np.errstate(all="ignore"):
        d = np.sqrt(((x * x).astype(F32) + (y * y).astype(F32)).astype(F32) + (z * z).astype(F32)).astype(F32)
        u = ((x / z).astype(F32) * fx).astype(F32) + cx
        v = ((y / z).astype(F32) * fy).astype(F32) + cy
        min_u, max_u, min_v, max_v = (F32(b) for b in kf["bounds"])
        vd = [row(R, r, D).astype(np.float64) for r in range(3)]
        vabs = np.sqrt(vd[0] * vd[0] + vd[1] * vd[1] + vd[2] * vd[2]).astype(F32)
        dot = vd[0] * x.astype(np.float64) + vd[1] * y.astype(np.float64) + vd[2] * z.astype(np.float64)
        cos = (dot / (d * vabs).astype(F32).astype(np.float64)).astype(F32)
    out = np.full(len(X), None, object)
    out[cos < F32(0.5)] = "angle"
    out[~((u < max_u) & (v < max_v) & (u > min_u) & (v > min_v))] = "outside"
    out[~((d < np.asarray(pts["max_dist"], F32)) & (d > np.asarray(pts["min_dist"], F32)))] = "distance"
    out[z < 0] = "behind"
    return out


def tables(orc, kfs, pts, cam, sf, th, ratio, dist_threshold=50):
    """-> dict(best_idx [K, m], best_dist [K, m], reasons [K][m], level [K, m] (-1: not in vision), cos_theta [K, m], cand [K, m] (the
    length of the candidate list), radius [K, m])"""
    sf = np.asarray(sf, F32)
    n_levels, K, m = len(sf), len(kfs), len(pts["usable"])
    usable = np.asarray(pts["usable"]).astype(bool)
    desc = np.ascontiguousarray(pts["desc"], np.uint8).reshape(-1, 32)
    out = dict(best_idx=np.full((K, m), -1, np.int32), best_dist=np.zeros((K, m), np.int32), reasons=[["unusable"] * m for _ in range(K)],
               level=np.full((K, m), -1, np.int32), cos_theta=np.zeros((K, m), F32), cand=np.zeros((K, m), np.int64), radius=np.zeros((K, m), F32))
    if m == 0:
        return out
    for k, kf in enumerate(kfs):
        pr = orc.project_map_points(pts["pos"], pts["view_dir"], pts["max_dist"], pts["min_dist"], kf["Rcw"], kf["tcw"], cam, kf["bounds"],
                                    scale_factor=sf[1] if n_levels > 1 else 1.2)
        why = why_not_in_vision(pts, kf, cam)
        vis = pr["visible"].astype(bool)
        assert np.array_equal(vis, np.array([w is None for w in why])), "the oracle's isInVision and its restatement differ"
        for j in np.flatnonzero(usable & ~vis):
            out["reasons"][k][j] = why[j]
        rows = np.flatnonzero(usable & vis)
        if not len(rows):
            continue
        lvl = np.minimum(pr["level"][rows].astype(np.int32), n_levels - 1)
        cos = pr["cos_theta"][rows].astype(F32)
        base = np.where(cos > F32(0.998), F32(2.5), F32(4.0)).astype(F32)
        radius = ((base * F32(th)).astype(F32) * (sf[lvl] * sf[lvl]).astype(F32)).astype(F32)
        lo, hi = np.maximum(0, lvl - 1).astype(np.int8), np.minimum(n_levels - 1, lvl + 1).astype(np.int8)
        bi, bd, sd, nc, _ = orc.search_in_area_ex(kf["kps"], kf["desc"], kf["bounds"], pr["uv"][rows], radius, lo, hi, desc[rows], None)
        out["level"][k, rows], out["cos_theta"][k, rows], out["cand"][k, rows], out["radius"][k, rows] = lvl, cos, nc, radius
        for q, j in enumerate(rows):
            if nc[q] <= 0:
                out["reasons"][k][j] = "empty"
            elif not bd[q] < dist_threshold:
                out["reasons"][k][j] = "threshold"
            elif not F32(bd[q]) / F32(sd[q]) < F32(ratio):
                out["reasons"][k][j] = "ratio"
            else:
                out["reasons"][k][j], out["best_idx"][k, j], out["best_dist"][k, j] = "accepted", int(bi[q]), int(bd[q])
    return out
