"""Restatement of what Tracking::trackReLocalize does with ONE PnP hypothesis (src/Tracking.cc:565-584, addMatchByProject :612-629):
the reference for orbfe_reloc_refine_stored (include/orbfe.h).  Composed from the oracle's pose-only optimiser
(orc.pose_only_optimize), its findFeaturesInArea + getBestMatch (orc.search_in_area_ex) and numpy, stage by stage, so that a test can feed
any stage with the outputs another implementation gave for the stage before.

The rules:

  R1  seed        Tracking::setCurrFrameAttrib (Tracking.cc:500-517): setMapPointsNull, then frame feature f gets the point of keyframe
                  feature held[f] if that point is non-null and not bad (:510-511).  The edges of Optimizer::OptimizePoseOnly are the
                  features that hold a good point, in feature order (Optimizer.cc:58-117); the initial estimate is
                  Converter::ConvertTcw2SE3(mRcw, mtcw) (:119): host/map_pb.hpp's tcw_to_se3 in fp64 (tcw_to_se3 below).
  R2  optimise    Optimizer.cc:122-178: orc.pose_only_optimize.  No edge at all: the estimate stays, nothing is an inlier.
  R3  post-check  Optimizer.cc:179-203: VirtualFrame::project2UV (Frame.cc:320-333) in float, with the pose the frame STILL has (the PnP
                  pose in the first optimisation, the float pose of the first in the second: setPose comes last, :201):
                  p = Rcw X + tcw as cv::gemm does it (the row summed left to right in float, the translation added through double),
                  u = x / z * fx + cx; an inlier is dropped when !(z > 0) || u > maxU || u < 0 || v > maxV || v < 0 (:185 -- 0, not
                  minU); the return value is edges - nBad (:202); every feature that is no inlier loses its point (:191-194); then the
                  frame's float pose becomes Converter::ConvertSE32Tcw of the estimate (:201, se3_to_tcw below).
  R4  decide #1   Tracking.cc:567-584: n < 10: the next hypothesis (REJECT_1); n >= 50: accepted (ACCEPT_1); else addMatchByProject.
  R5  search      ORBMatcher::searchByProjection(frame, keyframe, matches, th) with bFuse == false (ORBMatcher.cc:265-347):
                  twc = -Rcw^T tcw, tlc = Rkf twc + tkf (:274-275) in float, a row times a vector summed left to right; up / down iff
                  |tlc.z| > Camera::mfBl (:279-280); the queries are the keyframe's features with a good point, in index order (:283-287);
                  findFeaturesInArea(feature, th, lo, hi): radius th * getScaledFactor2(octave), octaves [o, 7] (up), [0, o] (down) or
                  [max(0, o - 1), min(o + 1, 7)] (:300-313); candidates that hold a good point are dropped, each occurrence counted by
                  addMatchInTrack (:321-331); getBestMatch; accepted when ratio < mfRatio && best < mnMinThreshold (:339); setMapPoints
                  in query order, the last one wins (:344-345); the return value is the number of accepted queries (:346).
  R6  decide #2   Tracking.cc:619: nAddition + nInliers < 50: REJECT_2.
  R7  optimise #2 Tracking.cc:621: from tcw_to_se3 of the float pose of R3, on what the frame holds now; then R3 again.
  R8  decide #3   Tracking.cc:622-627: n >= 50: ACCEPT_2; else the search with th 3 and the pose of R7, then nAddition + nInliers < 50:
                  REJECT_3, else ACCEPT_3.
"""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64
REJECT_1, ACCEPT_1, REJECT_2, ACCEPT_2, REJECT_3, ACCEPT_3 = 1, 2, 3, 4, 5, 6
VERDICT_NAMES = {1: "REJECT_1", 2: "ACCEPT_1", 3: "REJECT_2", 4: "ACCEPT_2", 5: "REJECT_3", 6: "ACCEPT_3"}
DEFAULTS = dict(th_first=10.0, th_second=3.0, ratio=0.9, min_threshold=50, min_inliers=10, enough=50)


# ---- the two pose conversions (host/map_pb.hpp), fp64, one operation per line of the C++ ---------------------------------------------
def tcw_to_se3(R, t):
    m = np.asarray(R, F32).reshape(3, 3).astype(F64)
    t = np.asarray(t, F32).reshape(3)
    q = np.zeros(4, F64)
    half, one = F64(0.5), F64(1.0)
    tr = (m[0, 0] + m[1, 1]) + m[2, 2]
    if tr > 0.0:
        tr = np.sqrt(tr + one)
        q[3] = half * tr
        tr = half / tr
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * tr, (m[0, 2] - m[2, 0]) * tr, (m[1, 0] - m[0, 1]) * tr
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        tr = np.sqrt(((m[i, i] - m[j, j]) - m[k, k]) + one)
        q[i] = half * tr
        tr = half / tr
        q[3] = (m[k, j] - m[j, k]) * tr
        q[j] = (m[j, i] + m[i, j]) * tr
        q[k] = (m[k, i] + m[i, k]) * tr
    for _ in range(2):
        n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        if n > 0.0:
            q = q / n
    if q[3] < 0.0:
        q = -q
    return np.concatenate([q, t.astype(F64)])


def se3_to_tcw(p):
    x, y, z, w = (F64(v) for v in p[:4])
    two, one = F64(2.0), F64(1.0)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = np.array([one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx, one - (txx + tyy)], F64)
    return R.astype(F32), np.asarray(p[4:7], F64).astype(F32)


# ---- float pieces ---------------------------------------------------------------------------------------------------------------------
def row3(A, r, x):
    """(A[r][0] x0 + A[r][1] x1) + A[r][2] x2 in float; x (..., 3)"""
    A = np.asarray(A, F32).reshape(9)
    return (A[3 * r] * x[..., 0] + A[3 * r + 1] * x[..., 1]) + A[3 * r + 2] * x[..., 2]


def affine(R, X, t):
    """cv::gemm's R X + t: the float row sum, the translation added through double"""
    X, t = np.asarray(X, F32), np.asarray(t, F32).reshape(3)
    return np.stack([(row3(R, r, X).astype(F64) + F64(t[r])).astype(F32) for r in range(3)], -1)


def project(R, t, X, cam):
    """project2UV: (u, v, z) in float"""
    fx, fy, cx, cy = (F32(v) for v in cam[:4])
    pc = affine(R, X, t)
    with np.errstate(all="ignore"):
        z = pc[..., 2]
        return pc[..., 0] / z * fx + cx, pc[..., 1] / z * fy + cy, z


def tlc_z(Rcw, tcw, kf_Rcw, kf_tcw):
    """R5: the z of tlc = Rkf (-Rcw^T tcw) + tkf"""
    R, t = np.asarray(Rcw, F32).reshape(9), np.asarray(tcw, F32).reshape(3)
    twc = np.array([-((R[r] * t[0] + R[3 + r] * t[1]) + R[6 + r] * t[2]) for r in range(3)], F32)
    return affine(kf_Rcw, twc, kf_tcw)[2]


def window(octave, z, baseline):
    """R5: the octave window of every query -> (lo, hi) int8"""
    o = np.asarray(octave, np.int64)
    if abs(F32(z)) > F32(baseline):
        if z > 0:
            return o.astype(np.int8), np.full(len(o), 7, np.int8)
        return np.zeros(len(o), np.int8), o.astype(np.int8)
    return np.maximum(0, o - 1).astype(np.int8), np.minimum(o + 1, 7).astype(np.int8)


# ---- the stages -----------------------------------------------------------------------------------------------------------------------
def seed(s):
    """R1 -> cur [NF]: the keyframe feature whose point each frame feature holds"""
    held, good = np.asarray(s["held"], np.int64), np.asarray(s["good"], bool)
    cur = np.full(len(held), -1, np.int32)
    ok = held >= 0
    ok[ok] = good[held[ok]]
    ok[s["n_kp"]:] = False
    cur[ok] = held[ok]
    return cur


def edge_arrays(s, cur):
    """the edge list of OptimizePoseOnly on what the frame holds -> (features, Xw, meas, info, sigma2)"""
    ef = np.flatnonzero(cur >= 0)
    kp = s["kps"]
    ru = np.asarray(s["right_u"], F64)[ef] if s.get("right_u") is not None else np.full(len(ef), -1.0)
    meas = np.stack([kp["x"][ef].astype(F64), kp["y"][ef].astype(F64), np.where(ru < 0, -1.0, ru)], 1).reshape(-1, 3)
    oc = kp["octave"][ef]
    return ef, s["pos"][cur[ef]].astype(F64).reshape(-1, 3), meas, s["inv_sigma2"][oc].astype(F64), s["sigma2"][oc]


def optimise(orc, s, cur, p_init):
    """R2 -> (estimate [7], edge features, inlier per edge)"""
    ef, Xw, meas, info, sig = edge_arrays(s, cur)
    if len(ef) == 0:
        return np.array(p_init, F64), ef, np.zeros(0, bool)
    fx, fy, cx, cy, bf = (float(F32(v)) for v in s["cam"])
    _, pose, inl = orc.pose_only_optimize(Xw, meas, info, sig, p_init, fx, fy, cx, cy, bf)
    return pose, ef, inl


def post_check(s, cur, ef, edge_inl, pose, pose_before):
    """R3; pose_before = (R, t): the float pose the frame has during the check
    -> dict(Tcw (R, t), inlier [NF], cur [NF] after the nulling, n_inliers, u, v, z of the checked features)"""
    R, t = se3_to_tcw(pose)
    Rp, tp = pose_before
    NF = len(cur)
    inlier = np.zeros(NF, np.uint8)
    chk = ef[np.asarray(edge_inl, bool)]
    u, v, z = project(Rp, tp, s["pos"][cur[chk]].reshape(-1, 3), s["cam"])
    max_u, max_v = F32(s["bounds"][1]), F32(s["bounds"][3])
    with np.errstate(invalid="ignore"):
        drop = ~(z > 0) | (u > max_u) | (u < 0) | (v > max_v) | (v < 0)
    inlier[chk[~drop]] = 1
    out = cur.copy()
    out[inlier == 0] = -1
    return dict(R=R, t=t, inlier=inlier, cur=out, n_inliers=int(inlier.sum()), u=u, v=v, z=z)


def search(orc, s, cur, R, t, th, p):
    """R5 -> dict(tlc_z, lo, hi, assigned [NF], hits [NF], accepted [n], n_added)"""
    z = tlc_z(R, t, s["kf_Rcw"], s["kf_tcw"])
    q = np.flatnonzero(np.asarray(s["good"], bool))
    kk = s["kf_kps"]
    oc = kk["octave"][q].astype(np.int64)
    lo, hi = window(oc, z, s["baseline"])
    NF, n_kp = len(cur), s["n_kp"]
    rad = (F32(th) * s["sigma2"][oc]).astype(F32)
    qxy = np.stack([kk["x"][q], kk["y"][q]], 1).astype(F32).reshape(-1, 2)
    ex = (cur[:n_kp] >= 0).astype(np.uint8)
    bi, bd, sd, nc, eh = orc.search_in_area_ex(s["kps"][:n_kp], s["desc"][:n_kp], s["bounds"], qxy, rad, lo, hi, s["kf_desc"][q], ex)
    hits = np.zeros(NF, np.int32)
    hits[:n_kp] = eh
    acc = np.zeros(len(s["good"]), np.uint8)
    out = cur.copy()
    with np.errstate(all="ignore"):
        for k, i in enumerate(q):
            if nc[k] > 0 and F32(bd[k]) / F32(sd[k]) < F32(p["ratio"]) and bd[k] < p["min_threshold"]:
                out[bi[k]] = i                                    # setMapPoints: in query order, the last one stays
                acc[i] = 1
    return dict(tlc_z=F32(z), lo=lo, hi=hi, assigned=out, hits=hits, accepted=acc, n_added=int(acc.sum()))


def refine(orc, s, **kw):
    """R1-R8, free-running -> the outputs of orbfe_reloc_refine_stored (plus the post-check's projections per stage)"""
    p = dict(DEFAULTS, **kw)
    NF, n = len(s["held"]), len(s["good"])
    o = dict(verdict=0, n_edges=np.zeros(2, np.int32), n_inliers=np.zeros(2, np.int32), n_added=np.zeros(2, np.int32), tlc_z=np.zeros(2, F32),
             pose_se3=np.zeros((2, 7)), Tcw=np.zeros((2, 12), F32), inlier=np.zeros((2, NF), np.uint8), assigned=np.full((2, NF), -1, np.int32),
             excluded_hits=np.zeros((2, NF), np.int32), query_accepted=np.zeros((2, n), np.uint8), checked=[None, None])
    cur = seed(s)
    p_init = tcw_to_se3(s["Rcw"], s["tcw"])
    before = (np.asarray(s["Rcw"], F32).reshape(9), np.asarray(s["tcw"], F32).reshape(3))
    for st in range(2):
        pose, ef, inl = optimise(orc, s, cur, p_init)
        c = post_check(s, cur, ef, inl, pose, before)
        cur = c["cur"]
        o["n_edges"][st], o["n_inliers"][st], o["pose_se3"][st], o["inlier"][st] = len(ef), c["n_inliers"], pose, c["inlier"]
        o["Tcw"][st] = np.concatenate([c["R"], c["t"]])
        o["checked"][st] = (c["u"], c["v"], c["z"])
        n_in = c["n_inliers"]
        if st == 0 and n_in < p["min_inliers"]:
            o["verdict"] = REJECT_1
            break
        if n_in >= p["enough"]:
            o["verdict"] = ACCEPT_1 if st == 0 else ACCEPT_2
            break
        r = search(orc, s, cur, c["R"], c["t"], p["th_first"] if st == 0 else p["th_second"], p)
        cur = r["assigned"]
        o["tlc_z"][st], o["n_added"][st], o["assigned"][st] = r["tlc_z"], r["n_added"], cur
        o["excluded_hits"][st], o["query_accepted"][st] = r["hits"], r["accepted"]
        if r["n_added"] + n_in < p["enough"]:
            o["verdict"] = REJECT_2 if st == 0 else REJECT_3
            break
        if st == 1:
            o["verdict"] = ACCEPT_3
            break
        p_init, before = tcw_to_se3(c["R"], c["t"]), (c["R"], c["t"])
    o["final_assigned"] = cur
    o["verdict_name"] = VERDICT_NAMES[o["verdict"]]
    return o
