"""Restatement of LocalMapping::createNewMapPoints (src/LocalMapping.cc:165-285) for one current keyframe and an ordered list of
neighbours, under the numerical decisions of DESIGN 4.17: the reference for the device call (orbfe_create_new_map_points, k_tri.hip),
which must equal it bit for bit.

Pieces and the reference lines they follow:
  * matching      searchByBow(pkf1 = current, pkf2 = neighbour, matches, bAddMPs = true) with ORBMatcher(0.6f, false) -- no verifyAngle
                  (src/ORBMatcher.cc:170-253, mnMinThreshold 50): frontend.ORBMatcher.searchByBow itself, with a numpy getBestMatch
                  (ORBMatcher.cc:967-990) in place of the device brute force.
  * epipolar      the second half of searchForTriangulation (ORBMatcher.cc:736-793): MatcherExt.epipolarFilter itself.
  * per match     computeCosTheta (LocalMapping.cc:290-299), the three-way branch (:221-247), triangulate (:311-339),
                  VirtualFrame::unProject (src/Frame.cc:262-275, double depth x float x), MapPoint::checkMapPoint (src/MapPoint.cc:384-420).
  * resolution    loop 2 over all matches (:199-263) and the tail loop over the unprocessed points (:268-278).

Quirks:
  T1  checkMapPoint's second error uses kp1.pt.y, not kp2.pt.y (MapPoint.cc:410).
  T2  neighbours run in std::map<KeyFrame::SharedPtr, ..> order (pointer order): the call takes the order as input.
  T3  every neighbour is matched against the map-point state BEFORE any assignment (loop 1 matches, loop 2 assigns).
  T4  first accepted candidate wins a current feature, in neighbour order, then match order; one neighbour's list may hold a queryIdx
      more than once (searchByBow has no uniqueness check) and a rejected earlier candidate does not block a later one.
  T5  the own-stereo branch consumes the feature's unprocessed map point even when checkMapPoint then rejects it: the point is lost to
      later candidates and to the tail loop.
  T6  tail: an unprocessed point that was not consumed is put back exactly when the feature's slot is still empty (null or bad) after loop 2.
  T7  a neighbour is skipped when (float)cv::norm(Ow_cur - Ow_nb) < Camera::mfBl.
  T8  cos0 < min(cos1, cos2) && cos0 > 0 && (stereo1 || stereo2 || cos0 < 0.9998), else own stereo if stereo1 && cos1 < cos2, else
      neighbour stereo if stereo2 && cos2 < cos1; cos1 == cos2 gives no point.  depth > 0 decides stereo; right-u (double) is rounded
      to float for the second point.
  T9  triangulate gives nothing when w3 / w2 > 1e-3 or when the WORLD z of the normalised solution is < 0.

Arithmetic: float cv::Mat products summed left to right; `A x + t` is (float)((double)sum + (double)t) (matcher_ext._affine); Mat::dot
and cv::norm in double; std::pow(float, 2) in double; 5.991 * l2scale compared in double; `Mat / s` multiplies by 1.0 / s in double.
triangulate's rows `a * r0 + b * r2` are float products and a float sum.

The SVD decision: OpenCV's float 4x4 cv::SVD::compute is replaced by the eigen-decomposition of N = A^T A (double, sums sequential over
the rows) with the cyclic Jacobi of pnp_restatement.jacobi (k_pnp.hip's jacobi_small, shared through jacobi_dev.h).  The smallest
eigenvalue (first strict minimum in index order) gives the null vector, the next smallest (first strict minimum of the rest) w2;
w_i = (float)sqrt(max(lambda_i, 0)) and the test is (float)(w3 / w2) > 1e-3.  The point is v[0..2] rounded to float, each times
1.0 / (double)(float)v[3].
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_restatement as pr  # noqa: E402
from orb_slam2_ros2_amd.frontend import ORBMatcher  # noqa: E402
from orb_slam2_ros2_amd.matcher_ext import _affine, _matvec  # noqa: E402

F32, F64 = np.float32, np.float64
KIND_TRI, KIND_OWN, KIND_NB = 1, 2, 3
GOOD, INMAP = 1, 2  # flag bits: map point non-null and not bad | isInMap()
REC_DTYPE = np.dtype([("nb", "<i4"), ("q", "<i4"), ("t", "<i4"), ("kind", "<i4"), ("xyz", "<f4", (3,))])


def best_match_numpy(q, t, off, cand):
    """ORBMatcher::getBestMatch (ORBMatcher.cc:967-990) per query over its candidate list, in list order"""
    q, t = np.asarray(q, np.uint8), np.asarray(t, np.uint8)
    nq = len(q)
    bi, bd, sd = np.zeros(nq, np.int32), np.zeros(nq, np.int32), np.zeros(nq, np.int32)
    for i in range(nq):
        ids = np.asarray(cand[off[i]:off[i + 1]], np.int64)
        d = np.unpackbits(q[i][None, :] ^ t[ids], axis=1).sum(1)
        mn, sec, mi = 2147483647, 2147483647, 0
        for k in range(len(ids)):
            if d[k] < mn:
                mn, mi = int(d[k]), int(ids[k])
            elif d[k] < sec:
                sec = int(d[k])
        bi[i], bd[i], sd[i] = mi, mn, sec
    return bi, bd, sd


def featvec_dict(fv):
    nodes, offs, feats = fv
    return {int(nodes[i]): [int(f) for f in feats[offs[i]:offs[i + 1]]] for i in range(len(nodes))}


def match_neighbour(cur, nb, k_inv, scale_factors):
    """searchForTriangulation(current, neighbour): [(queryIdx, trainIdx, distance)] in the reference's order"""
    m = ORBMatcher(0.6, False)
    fc, fn = np.asarray(cur["flags"], np.uint8), np.asarray(nb["flags"], np.uint8)
    bow = dict(desc_f=cur["desc"], desc_kf=nb["desc"], featvec_f=featvec_dict(cur["fv"]), featvec_kf=featvec_dict(nb["fv"]),
               good_f=(fc & GOOD) != 0, inmap_f=(fc & INMAP) != 0, good_kf=(fn & GOOD) != 0, inmap_kf=(fn & INMAP) != 0)
    matches = m.searchByBow(None, bAddMPs=True, best_match=best_match_numpy, **bow)
    if not matches:
        return []
    return m.epipolarFilter(matches, cur["kps"], nb["kps"], cur["Tcw"], cur["Twc"], nb["Tcw"], nb["Twc"], k_inv, scale_factors)


def _norm(v):
    return np.sqrt(F64(v[0]) * F64(v[0]) + F64(v[1]) * F64(v[1]) + F64(v[2]) * F64(v[2]))


def _dot(a, b):
    return F64(a[0]) * F64(b[0]) + F64(a[1]) * F64(b[1]) + F64(a[2]) * F64(b[2])


def cos_theta(R1, R2, p1, p2, cam):
    """computeCosTheta (LocalMapping.cc:290-299): R^T (x, y, 1) in float, the dot and the norms in double"""
    fx, fy, cx, cy = cam
    v1 = np.array([F32(F32(p1[0] - cx) / fx), F32(F32(p1[1] - cy) / fy), F32(1)], F32)
    v2 = np.array([F32(F32(p2[0] - cx) / fx), F32(F32(p2[1] - cy) / fy), F32(1)], F32)
    w1, w2 = _matvec(np.asarray(R1, F32).T.copy(), v1), _matvec(np.asarray(R2, F32).T.copy(), v2)
    with np.errstate(all="ignore"):
        return F32(_dot(w1, w2) / (_norm(w1) * _norm(w2)))


def tri_matrix(T1, T2, k1, k2, cam):
    """triangulate's A (LocalMapping.cc:318-325)"""
    fx, fy, cx, cy = cam
    A = np.zeros((4, 4), F32)
    for r, (T, kp, f, c, row) in enumerate(((T1, k1, fx, cx, 0), (T1, k1, fy, cy, 1), (T2, k2, fx, cx, 0), (T2, k2, fy, cy, 1))):
        b = F32(c - F32(kp["x"] if row == 0 else kp["y"]))
        for j in range(4):
            A[r, j] = F32(F32(f * T[row, j]) + F32(b * T[2, j]))
    return A


def solve_null(As):
    """the SVD decision on a batch of A (H, 4, 4): (ok (H,), point (H, 3) float32) -- ok False when w3 / w2 > 1e-3 or world z < 0"""
    As = np.asarray(As, F32).reshape(-1, 4, 4)
    H = len(As)
    if H == 0:
        return np.zeros(0, bool), np.zeros((0, 3), F32)
    A = As.astype(F64)
    N = np.zeros((H, 4, 4), F64)
    for i in range(4):
        for j in range(4):
            acc = A[:, 0, i] * A[:, 0, j]
            for k in range(1, 4):
                acc = acc + A[:, k, i] * A[:, k, j]
            N[:, i, j] = acc
    w, V = pr.jacobi(N)
    ok = np.zeros(H, bool)
    pts = np.zeros((H, 3), F32)
    with np.errstate(all="ignore"):
        for h in range(H):
            m = 0
            for i in range(1, 4):
                if w[h, i] < w[h, m]:
                    m = i
            s = -1
            for i in range(4):
                if i != m and (s < 0 or w[h, i] < w[h, s]):
                    s = i
            sv3 = F32(np.sqrt(w[h, m] if w[h, m] > 0 else 0.0))
            sv2 = F32(np.sqrt(w[h, s] if w[h, s] > 0 else 0.0))
            if F64(F32(sv3 / sv2)) > 1e-3:
                continue
            v = V[h, :, m].astype(F32)
            inv = F64(1.0) / F64(v[3])
            p = np.array([F32(F64(v[i]) * inv) for i in range(3)], F32)
            if p[2] < 0:
                continue
            ok[h], pts[h] = True, p
    return ok, pts


def check_map_point(p, T1, T2, k1, k2, sf, cam):
    """MapPoint::checkMapPoint (MapPoint.cc:384-420) with quirk T1"""
    fx, fy, cx, cy = cam
    o1, o2 = int(k1["octave"]), int(k2["octave"])
    s1, s2 = F32(sf[o1]), F32(sf[o2])
    l21, l22 = F32(F64(s1) * F64(s1)), F32(F64(s2) * F64(s2))
    c1 = _affine(1.0, T1[:3, :3], p, T1[:3, 3])
    c2 = _affine(1.0, T2[:3, :3], p, T2[:3, 3])
    if c1[2] <= 0 or c2[2] <= 0:
        return False
    with np.errstate(all="ignore"):
        u1 = F32(F32(F32(c1[0] / c1[2]) * fx) + cx)
        v1 = F32(F32(F32(c1[1] / c1[2]) * fy) + cy)
        u2 = F32(F32(F32(c2[0] / c2[2]) * fx) + cx)
        v2 = F32(F32(F32(c2[1] / c2[2]) * fy) + cy)
        e1 = F32(F64(F32(F32(k1["x"]) - u1)) ** 2 + F64(F32(F32(k1["y"]) - v1)) ** 2)
        e2 = F32(F64(F32(F32(k2["x"]) - u2)) ** 2 + F64(F32(F32(k1["y"]) - v2)) ** 2)   # T1
        if F64(e1) > 5.991 * F64(l21) or F64(e2) > 5.991 * F64(l22):
            return False
        dis = F32(_norm(c1) / _norm(c2))
        py = F32(s1 / s2)
        if F64(dis) > F64(py) * 1.5 or F64(dis) < F64(py) / 1.5:
            return False
    return True


def candidate(cur, nb, q, t, cam, sf):
    """everything of one match that does not depend on the map state (T3): (kind, xyz, ok, tri_A or None)"""
    k1, k2 = cur["kps"][q], nb["kps"][t]
    T1, T2 = np.asarray(cur["Tcw"], F32), np.asarray(nb["Tcw"], F32)
    R1, R2 = T1[:3, :3], T2[:3, :3]
    eye = np.eye(3, dtype=F32)
    c0 = cos_theta(R1, R2, (k1["x"], k1["y"]), (k2["x"], k2["y"]), cam)
    c1 = c2 = F32(1)
    st1, st2 = bool(cur["depth"][q] > 0), bool(nb["depth"][t] > 0)
    if st1:
        c1 = cos_theta(eye, eye, (k1["x"], k1["y"]), (F32(cur["right_u"][q]), k1["y"]), cam)
    if st2:
        c2 = cos_theta(eye, eye, (k2["x"], k2["y"]), (F32(nb["right_u"][t]), k2["y"]), cam)
    cst = min(c1, c2)
    if c0 < cst and c0 > 0 and (st1 or st2 or F64(c0) < 0.9998):
        return KIND_TRI, None, None, tri_matrix(T1, T2, k1, k2, cam)
    if st1 and c1 < c2:
        p = np.asarray(cur["unproc_pos"], F32)[q]
        return KIND_OWN, p, check_map_point(p, T1, T2, k1, k2, sf, cam), None
    if st2 and c2 < c1:
        fx, fy, cx, cy = cam
        d = F64(nb["depth"][t])
        x, y = F32(F32(k2["x"] - cx) / fx), F32(F32(k2["y"] - cy) / fy)
        pc = np.array([F32(d * F64(x)), F32(d * F64(y)), F32(d)], F32)
        Twc = np.asarray(nb["Twc"], F32)
        p = _affine(1.0, Twc[:3, :3], pc, Twc[:3, 3])
        return KIND_NB, p, check_map_point(p, T1, T2, k1, k2, sf, cam), None
    return 0, None, False, None


def baseline_ok(cur, nb, bl):
    """T7: (float)cv::norm(Ow_cur - Ow_nb) >= mfBl"""
    d = (np.asarray(cur["Ow"], F32) - np.asarray(nb["Ow"], F32)).astype(F32)
    return not (F32(_norm(d)) < F32(bl))


def create_new_map_points(cur, nbs, cam, k_inv, bl, scale_factors, match=None):
    """(records REC_DTYPE in processing order, tail int32 ascending, per-neighbour match lists, consumed [n] bool -- the features whose
    unprocessed point an own-stereo candidate took, T5).  match(cur, nb) -> [(queryIdx, trainIdx, ..)] replaces searchForTriangulation
    (default: match_neighbour)."""
    cam = tuple(F32(v) for v in cam)
    k_inv = np.asarray(k_inv, F32).reshape(3, 3)
    sf = np.asarray(scale_factors, F32)
    match = match or (lambda c, nb: match_neighbour(c, nb, k_inv, sf))
    # loop 1 (T2, T3, T7): every neighbour is matched against the state before any assignment
    per_nb = [match(cur, nb) if baseline_ok(cur, nb, bl) else [] for nb in nbs]
    cands = []
    for ni, ms in enumerate(per_nb):
        for q, t, *_ in ms:
            k, p, ok, A = candidate(cur, nbs[ni], q, t, cam, sf)
            cands.append([ni, q, t, k, p, ok, A])
    tri = [c for c in cands if c[3] == KIND_TRI]
    ok, pts = solve_null(np.array([c[6] for c in tri], F32).reshape(-1, 4, 4))
    for c, o, p in zip(tri, ok, pts):
        if o:
            c[4], c[5] = p, check_map_point(p, np.asarray(cur["Tcw"], F32), np.asarray(nbs[c[0]]["Tcw"], F32), cur["kps"][c[1]],
                                            nbs[c[0]]["kps"][c[2]], sf, cam)
        else:
            c[3] = 0
    # loop 2 (T4, T5)
    n = len(cur["kps"])
    fl = np.asarray(cur["flags"], np.uint8)
    assigned = np.zeros(n, bool)
    unproc = np.asarray(cur["unproc"], bool).copy()
    recs = []
    for ni, q, t, k, p, ok, _ in cands:
        if assigned[q] or k == 0:
            continue
        if k == KIND_OWN:
            if not unproc[q]:
                continue
            unproc[q] = False       # consumed (T5)
        if ok:
            assigned[q] = True
            recs.append((ni, q, t, k, p))
    tail = np.array([q for q in range(n) if unproc[q] and not assigned[q] and not (fl[q] & GOOD)], np.int32)   # T6
    consumed = np.asarray(cur["unproc"], bool) & ~unproc
    out = np.zeros(len(recs), REC_DTYPE)
    for i, r in enumerate(recs):
        out[i] = r
    return out, tail, per_nb, consumed
