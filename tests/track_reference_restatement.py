"""Restatement of Tracking::trackReference (src/Tracking.cc:360-371): the reference for orbfe_track_reference_stored (include/orbfe.h,
DESIGN 4.29).  Put together from what the suite already has -- bow_restatement.transform, bow_search_scenes.oracle for one candidate,
reloc_refine_restatement's conversions and post-check, the oracle's pose-only optimiser -- stage by stage, so that a test can feed any
stage with the outputs another implementation gave for the stage before.

The rules:

  T1  bow         Frame::computeBow (Frame.h:224-229): bow_restatement.transform of the frame's descriptors at `levelsup`, or a
                  FeatureVector the frame already has.
  T2  matches     ORBMatcher::searchByBow(frame, keyframe, matches, false, false) (ORBMatcher.cc:170-253) with verifyAngle
                  (:1013-1051): keyframe features with a good point search among the node's frame features WITHOUT a good point.
  T3  assign      setMapPoints (:815-830) in match order: frame feature `query` takes keyframe feature `train`'s point; the last match
                  that names a frame feature keeps it.  One addMatchInTrack per match.
  T4  decide #1   Tracking.cc:365: fewer than min_matches (10) matches: false.  The frame has been written by then.
  T5  edges       Optimizer.cc:58-117: the features that hold a point, their own or an assigned one, in feature order.
  T6  optimise    from Converter::ConvertTcw2SE3 of the pose the frame has (:119), the four rounds (:122-178).
  T7  post-check  Optimizer.cc:179-203 with the pose the frame still has; edges - nBad; the nulling; ConvertSE32Tcw of the estimate.
  T8  decide #2   Tracking.cc:370: n_inliers >= min_inliers (10).
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_restatement as br  # noqa: E402
import bow_search_scenes as bs  # noqa: E402
import reloc_refine_restatement as rr  # noqa: E402

F32, F64 = np.float32, np.float64
REJECT_MATCHES, REJECT_INLIERS, ACCEPT = 1, 2, 3
VERDICT_NAMES = {1: "REJECT_MATCHES", 2: "REJECT_INLIERS", 3: "ACCEPT"}
OWN = -2
DEFAULTS = dict(levelsup=4, ratio=0.7, check_orientation=True, min_matches=10, min_inliers=10)


def frame_flags(s):
    """the frame's flag bytes: 1 where the feature came with a good point"""
    NF = s["nf"]
    fg = np.zeros(NF, np.uint8)
    if s.get("frame_good") is not None:
        fg[:] = np.asarray(s["frame_good"], np.uint8) != 0
    fg[s["n_kp"]:] = 0
    return fg


def frame_bow(s, voc, levelsup=4):
    """T1 -> (words, values, nodes, offsets, features) of the frame's n_kp descriptors"""
    return br.transform(voc, s["desc"][:s["n_kp"]], levelsup)


def search(s, fv, p):
    """T2 -> [(query, train, distance)] in the reference's order; fv = (nodes, offsets, features) of the frame"""
    n_kp = s["n_kp"]
    q = dict(desc=s["desc"][:n_kp], fv=fv, flags=frame_flags(s)[:n_kp], kps=s["kps"][:n_kp])
    kf = dict(desc=s["kf_desc"], fv=s["kf_fv"], flags=(np.asarray(s["good"], np.uint8) != 0).astype(np.uint8), kps=s["kf_kps"])
    return bs.oracle(q, kf, bs.TRACK, p["ratio"], bool(p["check_orientation"]))


def assign(s, matches):
    """T3 -> assigned [NF]: the keyframe feature whose point each frame feature holds after setMapPoints, -1 none, OWN its own"""
    a = np.where(frame_flags(s) != 0, OWN, -1).astype(np.int32)
    for (qi, ti, _) in matches:
        a[qi] = ti                                        # in match order: the last one stays
    return a


def edge_arrays(s, assigned):
    """T5 -> (features, Xw, meas, info, sigma2)"""
    ef = np.flatnonzero(assigned != -1)
    kp = s["kps"]
    a = assigned[ef]
    X = np.zeros((len(ef), 3), F32)
    X[a >= 0] = s["pos"][a[a >= 0]]
    if (a == OWN).any():
        X[a == OWN] = np.asarray(s["frame_pos"], F32)[ef[a == OWN]]
    ru = np.asarray(s["right_u"], F64)[ef] if s.get("right_u") is not None else np.full(len(ef), -1.0)
    meas = np.stack([kp["x"][ef].astype(F64), kp["y"][ef].astype(F64), np.where(ru < 0, -1.0, ru)], 1).reshape(-1, 3)
    oc = kp["octave"][ef]
    return ef, X.astype(F64).reshape(-1, 3), meas, s["inv_sigma2"][oc].astype(F64), s["sigma2"][oc]


def optimise(orc, s, assigned, p_init):
    """T6 -> (estimate [7], edge features, inlier per edge)"""
    ef, Xw, meas, info, sig = edge_arrays(s, assigned)
    if len(ef) == 0:
        return np.array(p_init, F64), ef, np.zeros(0, bool)
    fx, fy, cx, cy, bf = (float(F32(v)) for v in s["cam"])
    _, pose, inl = orc.pose_only_optimize(Xw, meas, info, sig, p_init, fx, fy, cx, cy, bf)
    return pose, ef, inl


def post_check(s, assigned, ef, edge_inl, pose):
    """T7: reloc_refine_restatement.post_check over the positions the held points have, with the input pose"""
    X = np.zeros((len(assigned), 3), F32)
    _, Xw, _, _, _ = edge_arrays(s, assigned)
    X[np.flatnonzero(assigned != -1)] = Xw.astype(F32)
    idx = np.arange(len(assigned), dtype=np.int32)        # `cur` indexes the positions: feature f's point sits at row f
    cur = np.where(assigned != -1, idx, -1).astype(np.int32)
    before = (np.asarray(s["Rcw"], F32).reshape(9), np.asarray(s["tcw"], F32).reshape(3))
    c = rr.post_check(dict(pos=X, cam=s["cam"], bounds=s["bounds"]), cur, ef, edge_inl, pose, before)
    final = assigned.copy()
    final[c["inlier"] == 0] = -1
    return dict(R=c["R"], t=c["t"], inlier=c["inlier"], final=final, n_inliers=c["n_inliers"], u=c["u"], v=c["v"], z=c["z"])


def chi2(s, assigned, pose):
    """the chi2 of every edge at an estimate, with its threshold 5.991 / 7.815 * sigma2 (for the scene builders' margins)"""
    ef, Xw, meas, info, sig = edge_arrays(s, assigned)
    fx, fy, cx, cy, bf = (float(F32(v)) for v in s["cam"])
    x, y, z, w = pose[:4]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    pc = Xw @ R.T + np.asarray(pose[4:7])
    u, v = fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy
    e2 = (meas[:, 0] - u) ** 2 + (meas[:, 1] - v) ** 2
    stereo = meas[:, 2] >= 0
    e2 = e2 + np.where(stereo, (meas[:, 2] - (u - bf / pc[:, 2])) ** 2, 0.0)
    return ef, e2 * info, np.where(stereo, 7.815, 5.991) * sig.astype(F64)


def track(orc, s, voc=None, fv=None, **kw):
    """T1-T8, free-running -> the outputs of orbfe_track_reference_stored (plus bow when the transform ran here)"""
    p = dict(DEFAULTS, **kw)
    NF = s["nf"]
    o = dict(verdict=0, n_matches=0, n_edges=0, n_inliers=0, inlier=np.zeros(NF, np.uint8), pose_se3=np.zeros(7), Tcw=np.zeros(12, F32))
    if fv is None:
        o["bow"] = frame_bow(s, voc, p["levelsup"])
        fv = o["bow"][2:]
    m = search(s, fv, p)
    o["matches"], o["n_matches"] = m, len(m)
    a = assign(s, m)
    o["assigned"] = a
    if len(m) < p["min_matches"]:
        o["verdict"], o["final_assigned"] = REJECT_MATCHES, a.copy()
    else:
        pose, ef, inl = optimise(orc, s, a, rr.tcw_to_se3(s["Rcw"], s["tcw"]))
        c = post_check(s, a, ef, inl, pose)
        o["n_edges"], o["n_inliers"], o["inlier"], o["pose_se3"], o["final_assigned"] = len(ef), c["n_inliers"], c["inlier"], pose, c["final"]
        o["Tcw"] = np.concatenate([c["R"], c["t"]])
        o["edge_inlier"] = (ef, np.asarray(inl, bool))
        o["verdict"] = ACCEPT if c["n_inliers"] >= p["min_inliers"] else REJECT_INLIERS
    o["verdict_name"] = VERDICT_NAMES[o["verdict"]]
    return o
