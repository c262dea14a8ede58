"""Restatement of Tracking::trackMotionModel from processLastFrame's unProject to its return (src/Tracking.cc:381-406): the reference for
orbfe_track_motion_model_slots (include/orbfe.h).  Composed from reloc_refine_restatement.py's float pieces (affine,
tcw_to_se3, se3_to_tcw, tlc_z, window, edge_arrays, optimise, post_check), the oracle's findFeaturesInArea + getBestMatch
(orc.search_in_area_ex), its pose-only optimiser (orc.pose_only_optimize) and numpy, stage by stage, so that a test can feed any stage with
the outputs another implementation gave for the stage before.

A scene s: the current frame (kps, desc, n_kp, right_u [NF] or None), the last frame (l_kps, l_desc, l_n, l_depth [NF] or None), the last
frame's map state (last_flags [NF], last_pos [NF, 3]), the poses (Rcw, tcw: the predicted one; last_Rcw, last_tcw, last_Rwc, last_twc),
cam, bounds, baseline, sigma2, inv_sigma2, nf.

The rules:

  M1  unProject   Frame::unProject (src/Frame.cc:179-202): a last-frame feature whose point is null or bad (flag bit 0 clear) and whose
                  depth is >= 0 gets a temporary point.  VirtualFrame::unProject (:262-275): x = (pt.x - cx) / fx, y = (pt.y - cy) / fy
                  in float; p3dC = (float)(depth x), (float)(depth y), (float)depth with depth a double; p3dW = mRwc p3dC + mtwc as
                  cv::gemm does it (:195).  MapPoint::create(p3dW) is good and not in the map.
  M2  direction   ORBMatcher.cc:270-280: twc1 = -Rcw1^T tcw1, tlc = Rcw2 twc1 + tcw2; up / down iff |tlc.z| > Camera::mfBl.
  M3  queries     :283-313: the last frame's features that hold a good point, in feature order; findFeaturesInArea(feature, th, lo, hi):
                  centre the feature's position, radius th * getScaledFactor2(octave), octaves [o, 7] (up), [0, o] (down) or
                  [max(0, o - 1), min(o + 1, 7)]; the descriptor is the last frame's.
  M4  search 1    :314-346 with bFuse == false: candidates that hold a good point are dropped, each occurrence counted by
                  addMatchInTrack; getBestMatch; accepted when ratio < mfRatio && best < mnMinThreshold; setMapPoints in query order:
                  the last query that names a feature keeps it, every match is one addMatchInTrack; the return value is the number of
                  accepted queries.
  M5  search 2    Tracking.cc:388-391: nMatches < 20: the same with th 30; what search 1 assigned is held now; nMatches is the sum.
  M6  decide #1   :392: nMatches < 20: false.  Both frames are written by then.
  M7  optimise    Optimizer.cc:58-178 on what the frame holds, from ConvertTcw2SE3 of the predicted pose (:119).
  M8  post-check  :179-203 with the pose the frame still has (the predicted one); a feature that is no inlier loses its point;
                  setPose(ConvertSE32Tcw(estimate)).
  M9  count       Tracking.cc:397-404: the features that hold a point that isInMap() -- never a temporary one.
  M10 decide #2   :405: inLiers >= 10.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reloc_refine_restatement as rr  # noqa: E402

F32, F64 = np.float32, np.float64
REJECT_MATCHES, REJECT_INLIERS, ACCEPT = 1, 2, 3
VERDICT_NAMES = {1: "REJECT_MATCHES", 2: "REJECT_INLIERS", 3: "ACCEPT"}
DEFAULTS = dict(th=15.0, th_second=30.0, ratio=0.9, min_threshold=50, min_matches=20, min_inliers=10)


def unproject(s):
    """M1 -> (temp [NF] uint8, temp_pos [NF, 3] float32, zero where no point was made)"""
    NF, n = s["nf"], s["l_n"]
    temp, pos = np.zeros(NF, np.uint8), np.zeros((NF, 3), F32)
    if s.get("l_depth") is None:
        return temp, pos
    fl = np.asarray(s["last_flags"], np.uint8)[:n]
    depth = np.asarray(s["l_depth"], F64)[:n]
    with np.errstate(invalid="ignore"):
        mk = ((fl & 1) == 0) & (depth >= 0)
    kp = s["l_kps"][:n]
    fx, fy, cx, cy = (F32(v) for v in s["cam"][:4])
    x, y = (kp["x"] - cx) / fx, (kp["y"] - cy) / fy
    pc = np.stack([(depth * x.astype(F64)).astype(F32), (depth * y.astype(F64)).astype(F32), depth.astype(F32)], 1)
    pw = rr.affine(s["last_Rwc"], pc, s["last_twc"])
    temp[:n][mk] = 1
    pos[:n][mk] = pw[mk]
    return temp, pos


def queries(s, temp, temp_pos):
    """M2, M3 -> dict(who [n_q]: the last-frame feature of every query, in feature order; z; lo, hi [n_q]; octave [n_q];
    pos [NF, 3]: the position of the point each last-frame feature holds (zero where none))"""
    NF, n = s["nf"], s["l_n"]
    good = np.zeros(NF, bool)
    good[:n] = (np.asarray(s["last_flags"], np.uint8)[:n] & 1) == 1
    pos = np.where(good[:, None], np.asarray(s["last_pos"], F32).reshape(NF, 3), temp_pos).astype(F32)
    pos[~(good | (temp == 1))] = 0
    who = np.flatnonzero(good | (temp == 1))
    z = rr.tlc_z(s["Rcw"], s["tcw"], s["last_Rcw"], s["last_tcw"])
    oc = s["l_kps"]["octave"][who].astype(np.int64)
    lo, hi = rr.window(oc, z, s["baseline"])
    return dict(who=who, z=F32(z), lo=lo, hi=hi, octave=oc, pos=pos)


def search(orc, s, q, held, th, p):
    """M4 / M5: one searchByProjection(frame, lastFrame, th); held [NF]: the last-frame feature whose point each frame feature holds
    -> dict(assigned [NF], hits [NF], accepted [NF] per last-frame feature, n_added)"""
    NF, n_kp = s["nf"], s["n_kp"]
    who = q["who"]
    lk = s["l_kps"]
    rad = (F32(th) * s["sigma2"][q["octave"]]).astype(F32)
    qxy = np.stack([lk["x"][who], lk["y"][who]], 1).astype(F32).reshape(-1, 2)
    ex = (held[:n_kp] >= 0).astype(np.uint8)
    hits, acc, out = np.zeros(NF, np.int32), np.zeros(NF, np.uint8), held.copy()
    if len(who):
        bi, bd, sd, nc, eh = orc.search_in_area_ex(s["kps"][:n_kp], s["desc"][:n_kp], s["bounds"], qxy, rad, q["lo"], q["hi"], s["l_desc"][who], ex)
        hits[:n_kp] = eh[:n_kp]
        with np.errstate(all="ignore"):
            for k, i in enumerate(who):
                if nc[k] > 0 and F32(bd[k]) / F32(sd[k]) < F32(p["ratio"]) and bd[k] < p["min_threshold"]:
                    out[bi[k]] = i                                    # setMapPoints: in query order, the last one stays
                    acc[i] = 1
    return dict(assigned=out, hits=hits, accepted=acc, n_added=int(acc.sum()))


def edge_scene(s, q):
    """the scene as reloc_refine_restatement's edge_arrays / optimise / post_check read it: pos indexed by last-frame feature"""
    return dict(s, pos=q["pos"])


def optimise(orc, s, q, assigned):
    """M7 -> (estimate [7], edge features, inlier per edge)"""
    return rr.optimise(orc, edge_scene(s, q), assigned, rr.tcw_to_se3(s["Rcw"], s["tcw"]))


def post_check(s, q, assigned, ef, edge_inl, pose):
    """M8 -> reloc_refine_restatement.post_check's dict (cur: final_assigned)"""
    before = (np.asarray(s["Rcw"], F32).reshape(9), np.asarray(s["tcw"], F32).reshape(3))
    return rr.post_check(edge_scene(s, q), assigned, ef, edge_inl, pose, before)


def count_in_map(s, final_assigned):
    """M9"""
    a = np.asarray(final_assigned)
    fl = np.asarray(s["last_flags"], np.uint8)
    return int(((fl[a[a >= 0]] & 3) == 3).sum())


def chi2(s, q, assigned, pose):
    """the chi2 of every edge at an estimate with its threshold (for the scene builders' margins) -> (edge features, chi2, threshold)"""
    import track_reference_restatement as tr
    e = edge_scene(s, q)
    return tr.chi2(dict(e, frame_pos=None), assigned, pose)


def track(orc, s, **kw):
    """M1-M10, free-running -> the outputs of orbfe_track_motion_model_slots (plus q, the queries, and edge_inlier)"""
    p = dict(DEFAULTS, **kw)
    NF = s["nf"]
    temp, temp_pos = unproject(s)
    q = queries(s, temp, temp_pos)
    o = dict(verdict=0, passes=1, n_edges=0, n_inliers=0, n_in_map=0, inlier=np.zeros(NF, np.uint8), pose_se3=np.zeros(7), Tcw=np.zeros(12, F32),
             temp=temp, temp_pos=temp_pos, q=q)
    r1 = search(orc, s, q, np.full(NF, -1, np.int32), p["th"], p)
    a, hits, qm, nm = r1["assigned"], r1["hits"].copy(), r1["accepted"].astype(np.int32), r1["n_added"]
    if nm < p["min_matches"] and p["th_second"] > 0:
        r2 = search(orc, s, q, a, p["th_second"], p)
        a, hits, qm, nm = r2["assigned"], hits + r2["hits"], qm + r2["accepted"], nm + r2["n_added"]
        o["passes"] = 2
    o.update(assigned=a, excluded_hits=hits, query_matches=qm, n_matches=nm)
    if nm < p["min_matches"]:
        o["verdict"], o["final_assigned"] = REJECT_MATCHES, a.copy()
    else:
        pose, ef, inl = optimise(orc, s, q, a)
        c = post_check(s, q, a, ef, inl, pose)
        o.update(n_edges=len(ef), n_inliers=c["n_inliers"], inlier=c["inlier"], pose_se3=pose, Tcw=np.concatenate([c["R"], c["t"]]),
                 final_assigned=c["cur"], edge_inlier=(ef, inl), n_in_map=count_in_map(s, c["cur"]))
        o["verdict"] = ACCEPT if o["n_in_map"] >= p["min_inliers"] else REJECT_INLIERS
    o["verdict_name"] = VERDICT_NAMES[o["verdict"]]
    return o


def array_call_inputs(s, q):
    """what orbfe_track_motion_model (the array call) takes for the queries of M1-M3 -> dict of its arrays; who maps a query to its feature"""
    who = q["who"]
    lk = s["l_kps"]
    return dict(qxy=np.stack([lk["x"][who], lk["y"][who]], 1).astype(F32).reshape(-1, 2), q_octave=q["octave"].astype(np.int8), q_min_level=q["lo"],
                q_max_level=q["hi"], desc=s["l_desc"][who], pos=q["pos"][who])
