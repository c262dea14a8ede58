"""Seeded scenes for the searchByBow-over-stored-keyframes tests (orbfe_search_by_bow_stored): one query frame and K
candidate keyframes on tri_scenes.make_kf, with keypoint angles and a skewed node function added, a scene whose special cases are placed
by hand, and the oracle: frontend.ORBMatcher.searchByBow per candidate with triangulation_restatement.best_match_numpy, on the CPU alone."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tri_scenes as ts  # noqa: E402
import triangulation_restatement as tr  # noqa: E402
from orb_slam2_ros2_amd._lib import KP_DTYPE  # noqa: E402
from orb_slam2_ros2_amd.frontend import ORBMatcher  # noqa: E402

F32 = np.float32
GOOD, INMAP = 1, 2
TRACK, LOOP, ADD = 0, 1, 2
MODES = {"track": TRACK, "loop": LOOP, "add": ADD}
INT_MAX = 2147483647
BIG_NODE = 5
ANGLE_OFFSETS = (0.0, 100.0, 359.9, 12.0)


def wrap_angle(a):
    """into (-180, 180], float32 (cv::KeyPoint::angle as the extractor leaves it)"""
    a = (np.asarray(a, np.float64) + 180.0) % 360.0 - 180.0
    a = np.where(a == -180.0, 180.0, a)
    return a.astype(F32)


def skewed_nodes(pid, n_nodes=23):
    """half of the points (the even ones) in ONE node, the rest spread over n_nodes"""
    pid = np.asarray(pid, np.int64)
    return np.where(pid % 2 == 0, BIG_NODE, 10 + (pid * 7919) % n_nodes)


def _points(rng, n_pts):
    z = rng.uniform(4, 14, n_pts)
    return np.stack([z * rng.uniform(-0.5, 0.5, n_pts), z * rng.uniform(-0.36, 0.36, n_pts), z], 1)


def _dress(rng, kf, base_ang, offset, good, skewed, outlier_frac=0.25):
    """angles (the point's own angle + the keyframe's offset + noise, a quarter of them a multiple of 30 degrees off), the flags of a
    frame / a keyframe, the skewed FeatureVector"""
    m = len(kf["pid"])
    step = np.where(rng.random(m) < outlier_frac, 30.0 * rng.integers(1, 12, m), 0.0)
    kf["kps"]["angle"] = wrap_angle(base_ang[kf["pid"]] + offset + rng.normal(0, 1.0, m) + step)
    r = rng.random(m)
    kf["flags"] = np.where(r < good, GOOD | INMAP, np.where(r < good + 0.1, GOOD, 0)).astype(np.uint8)
    if skewed:
        kf["fv"] = ts.csr_from_nodes(skewed_nodes(kf["pid"]))
    return kf


def scene(seed=0, K=4, n=300, n_pts=400, skewed=True):
    """-> (query, [K candidates]): the query has few good points (a frame being relocalised), the candidates many"""
    rng = np.random.default_rng(seed)
    pts = _points(rng, n_pts)
    base = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)
    base_ang = rng.uniform(-180, 180, n_pts)
    query = _dress(rng, ts.make_kf(rng, pts, base, (0, 0, 0), n=n), base_ang, 0.0, 0.15, skewed)
    cands = []
    for k in range(K):
        ang = rng.uniform(0, 2 * np.pi)
        c = (0.3 * np.cos(ang), 0.1 * np.sin(ang), 0.05 * rng.normal())
        cands.append(_dress(rng, ts.make_kf(rng, pts, base, c, ts.yaw(rng.normal(0, 0.02)), n=n), base_ang,
                            ANGLE_OFFSETS[k % len(ANGLE_OFFSETS)], 0.6, skewed))
    return query, cands


# ---- the hand-placed scene -------------------------------------------------------------------------------------------------------------
def _kf_from_rows(rows):
    """rows of (descriptor [32], node, angle, flag) -> a keyframe dict"""
    n = len(rows)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"], kps["y"] = 20 + 10 * np.arange(n), 30
    kps["size"], kps["class_id"] = 7.0, -1
    kps["angle"] = np.array([r[2] for r in rows], F32)
    return dict(kps=kps, desc=np.array([r[0] for r in rows], np.uint8).reshape(n, 32), fv=ts.csr_from_nodes([r[1] for r in rows]),
                flags=np.array([r[3] for r in rows], np.uint8))


def _flip(d, bits):
    d = np.array(d, np.uint8)
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def hand_scene():
    """-> (query, {name: candidate}).  Query features 0 .. 19 are unrelated random descriptors R_i in node 1 + i % 3 at angle 170 (feature
    0: angle 10); a candidate feature that copies R_i in that node matches i at distance 0, and its angle puts the pair into a chosen bin.
      bins      feature 0 against an angle one float above 10: diff a hair below zero, 360 + diff == 360.0f, bin 30 -> 0; with it the
                bins hold 5 (bin 0), 4 (bin 3), 2 (bin 7), 2 (bin 9), 1 (bin 12): 7 and 9 compete for third place, 7 wins
      fewbins   two non-empty bins
      dup       two keyframe features copy R_5: two matches with queryIdx 5
      edge      node 50 holds ONE query feature (second == INT_MAX); node 60 two query features identical to the keyframe's (0 / 0,
                accepted); node 61 two query features both 4 bits from the keyframe's (best == second, ratio 1, rejected)
      disjoint  shares no node with the query
      emptied   node 70's query features all carry a good point: in TRACK mode the candidate list is empty and the feature is skipped,
                in LOOP mode it matches"""
    rng = np.random.default_rng(77)
    R = rng.integers(0, 256, (27, 32), dtype=np.uint8)
    q_rows = [(R[i], 1 + i % 3, 10.0 if i == 0 else 170.0, 0) for i in range(20)]
    S, X, Z = R[20], R[21], R[23]
    q_rows.append((S, 50, 0.0, 0))
    q_rows += [(X, 60, 0.0, 0), (X, 60, 0.0, 0)]
    q_rows += [(_flip(Z, range(0, 4)), 61, 0.0, 0), (_flip(Z, range(8, 12)), 61, 0.0, 0)]
    q_rows += [(R[25], 70, 0.0, GOOD | INMAP), (R[26], 70, 0.0, GOOD | INMAP)]
    query = _kf_from_rows(q_rows)

    def partner(i, diff):
        return (R[i], 1 + i % 3, 170.0 - diff, GOOD)
    above_ten = float(np.nextafter(F32(10), F32(20)))
    bins = [(R[0], 1, above_ten, GOOD)] + [partner(i, 6) for i in (1, 2, 3, 4)] + [partner(i, 42) for i in (5, 6, 7, 8)] + \
        [partner(i, 90) for i in (9, 10)] + [partner(i, 114) for i in (11, 12)] + [partner(13, 150)]
    cands = dict(
        bins=_kf_from_rows(bins),
        fewbins=_kf_from_rows([partner(i, 6) for i in (1, 2, 3)] + [partner(i, 42) for i in (4, 5)]),
        dup=_kf_from_rows([partner(5, 6), partner(6, 6), partner(5, 6)]),
        edge=_kf_from_rows([(_flip(S, (1, 17, 200)), 50, 0.0, GOOD), (X, 60, 0.0, GOOD), (Z, 61, 0.0, GOOD)]),
        disjoint=_kf_from_rows([(R[i], 1000 + i, 0.0, GOOD) for i in range(5)]),
        emptied=_kf_from_rows([(R[25], 70, 0.0, GOOD), partner(1, 6)]))
    return query, cands


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
def raw_and_bins(query, kf, mode, ratio):
    """the matches before verifyAngle and each one's bin by the reference's own arithmetic (bin 30 NOT folded)"""
    raw = oracle(query, kf, mode, ratio, False)
    bins = []
    for (qi, ti, _) in raw:
        diff = F32(query["kps"]["angle"][qi]) - F32(kf["kps"]["angle"][ti])
        diff = diff if diff >= 0 else F32(360) + diff
        bins.append(int(diff / F32(12)))
    return raw, bins


def oracle(query, kf, mode, ratio, check, best_match=None):
    """ORBMatcher(ratio, check).searchByBow(query, kf): [(queryIdx, trainIdx, distance)] in the reference's order, on the CPU"""
    fq, fk = np.asarray(query["flags"], np.uint8), np.asarray(kf["flags"], np.uint8)
    return ORBMatcher(ratio, check).searchByBow(
        None, desc_f=query["desc"], desc_kf=kf["desc"], featvec_f=tr.featvec_dict(query["fv"]), featvec_kf=tr.featvec_dict(kf["fv"]),
        good_f=(fq & GOOD) != 0, inmap_f=(fq & INMAP) != 0, good_kf=(fk & GOOD) != 0, inmap_kf=(fk & INMAP) != 0,
        angles_f=query["kps"]["angle"], angles_kf=kf["kps"]["angle"], bAddMPs=mode == ADD, bLoop=mode == LOOP,
        best_match=best_match or tr.best_match_numpy)


def best_second(query, kf, t, mode=LOOP):
    """(best, second) of keyframe feature t over its node's query features (no filter but the mode's)"""
    fvq, fvk = tr.featvec_dict(query["fv"]), tr.featvec_dict(kf["fv"])
    node = next(nd for nd, fs in fvk.items() if t in fs)
    cand = [p for p in fvq.get(node, []) if mode == LOOP or not (query["flags"][p] & GOOD)]
    _, bd, sd = tr.best_match_numpy(kf["desc"][[t]], query["desc"], [0, len(cand)], cand)
    return int(bd[0]), int(sd[0]), len(cand)


def as_tuples(a):
    return [(int(m["query"]), int(m["train"]), int(m["distance"])) for m in a]


def host_query(q, with_flags=True):
    return dict(desc=q["desc"], fv=q["fv"], angle=q["kps"]["angle"], flags=q["flags"] if with_flags else None)


def fill_store(store, kfs, first_id=1):
    ids = []
    for i, kf in enumerate(kfs):
        store.add(first_id + i, kf["kps"], kf["desc"])
        store.set_bow(first_id + i, *kf["fv"])
        ids.append(first_id + i)
    return ids
