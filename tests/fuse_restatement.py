"""What orbfe_fuse_into_keyframes must return, composed from the already-pinned single calls of the CPU oracle (oracle/pyoracle.py, used
read-only): Oracle.search_in_area_ex per target for findFeaturesInArea + getBestMatch, Oracle.project_map_points per target for
MapPoint::isInVision.  The octave window, the radius and the acceptance test of ORBMatcher::searchByProjection(pFrame1, pFrame2, .., bFuse)
(src/ORBMatcher.cc:277-280, 300-313, 339) are restated here in numpy."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def octave_window(octave, z, bl):
    """(lo, hi) per query: up -> [octave, 7], down -> [0, octave], else [octave - 1, octave + 1] clipped to 0 .. 7 (7 is hard-coded)"""
    octave = np.asarray(octave, np.int32)
    z, bl = F32(z), F32(bl)
    up = abs(z) > bl and z > 0
    down = abs(z) > bl and not z > 0
    if up:
        return octave.astype(np.int8), np.full(len(octave), 7, np.int8)
    if down:
        return np.zeros(len(octave), np.int8), octave.astype(np.int8)
    return np.maximum(0, octave - 1).astype(np.int8), np.minimum(octave + 1, 7).astype(np.int8)


def window_case(z, bl):
    z, bl = F32(z), F32(bl)
    return 0 if not abs(z) > bl else (1 if z > 0 else 2)


def fuse_into_keyframes(orc, cur, pts, targets, z, cam, bl, scale_factors, th=3.0, ratio=0.6, dist_threshold=50):
    """-> (best_idx [K, n] int32, best_dist [K, n] int32, visible [K, n] uint8) with the semantics of include/orbfe.h"""
    n, K = len(cur["kps"]), len(targets)
    bi, bd, vis = np.full((K, n), -1, np.int32), np.zeros((K, n), np.int32), np.zeros((K, n), np.uint8)
    if n == 0 or K == 0:
        return bi, bd, vis
    sf = np.asarray(scale_factors, F32)
    octave = cur["kps"]["octave"].astype(np.int32)
    radius = (F32(th) * (sf[octave] * sf[octave]).astype(F32)).astype(F32)          # th * getScaledFactor2(octave) (Frame.cc:289)
    qxy = np.stack([cur["kps"]["x"], cur["kps"]["y"]], 1).astype(F32)
    has = np.asarray(pts["has_point"]).astype(bool)
    for k, t in enumerate(targets):
        lo, hi = octave_window(octave, z[k], bl)
        if len(t["kps"]):
            b, d, s, nc, _ = orc.search_in_area_ex(t["kps"], t["desc"], t["bounds"], qxy, radius, lo, hi, cur["desc"])
            with np.errstate(all="ignore"):
                ok = (nc > 0) & (d.astype(F32) / s.astype(F32) < F32(ratio)) & (d < dist_threshold)
            bi[k] = np.where(ok, b, -1)
            bd[k] = np.where(ok, d, 0)
        p = orc.project_map_points(pts["pos"], pts["view_dir"], pts["max_dist"], pts["min_dist"], t["Rcw"], t["tcw"], cam, t["bounds"])
        vis[k] = np.where(has, p["visible"], 0)
    return bi, bd, vis
