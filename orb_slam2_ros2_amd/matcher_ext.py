"""Host logic of the remaining callers of ORBMatcher::getBestMatch (include/ORB_SLAM2/ORBMatcher.h:41-75) around the batched device
search: searchBySim3 x2 (src/ORBMatcher.cc:370-559), fuse x2 / processFuseMps (:623-734) and searchForTriangulation (:736-787).

Map state enters as arrays and the side effects on the map come back as data, as in frontend.ORBMatcher.  Float arithmetic follows the
reference's expressions in float32.  Where the reference multiplies cv::Mat objects (un-vendored OpenCV, cv::gemm), the convention of
csrc/k_guided.hip is used, a decision that could not be checked against OpenCV here: a 3x3 / 4x4 product element is the float sum
a0 b0 + a1 b1 + a2 b2 (+ a3 b3) taken left to right, and `alpha * A * x + t` is (float)((double)alpha * (double)sum + (double)t).
"""
from __future__ import annotations

import numpy as np

F32 = np.float32


def _matvec(R, x):
    """rows of R (3x3 float32) times x (3,) in float32, left to right"""
    R = np.asarray(R, F32).reshape(3, 3)
    return np.array([F32(F32(F32(R[r, 0] * x[0]) + F32(R[r, 1] * x[1])) + F32(R[r, 2] * x[2])) for r in range(3)], F32)


def _affine(alpha, R, x, t):
    """(float)(alpha * (R x) + t) with the sum R x in float and the scale / shift in double (cv::gemm's alpha / beta)"""
    s = _matvec(R, x)
    return np.array([F32(np.float64(alpha) * np.float64(s[r]) + np.float64(np.asarray(t, F32).reshape(3)[r])) for r in range(3)], F32)


def _matmul(A, B):
    A, B = np.asarray(A, F32), np.asarray(B, F32)
    n, m, k = A.shape[0], B.shape[1], A.shape[1]
    out = np.zeros((n, m), F32)
    for i in range(n):
        for j in range(m):
            acc = F32(A[i, 0] * B[0, j])
            for q in range(1, k):
                acc = F32(acc + F32(A[i, q] * B[q, j]))
            out[i, j] = acc
    return out


def predict_level(max_dist, d, log_sf):
    """MapPoint::predictLevel (src/MapPoint.cc:188-199): cvRound(std::log(nMaxDis / distance) / std::log(mfScaledFactor)), clamped to [0, 7]"""
    lr = F32(np.log(np.float64(F32(F32(max_dist) / F32(d)))))
    lvl = int(np.rint(F32(lr / F32(log_sf))))
    return min(7, max(0, lvl))


def sim3_project(pos, max_dist, min_dist, Rcw, tcw, sim3, cam, bounds, log_sf):
    """The geometric half of ORBMatcher::SIM3Project (src/ORBMatcher.cc:370-392) for every point: world position -> source camera
    (Rcw, tcw; None: the point is already in the frame the similarity maps from) -> target camera through the similarity
    sim3 = (s, R, t) -> pixel.  Returns (ok [n], uv [n, 2], octave [n]): ok = in front, inside the image bounds (isInImage of mpCurr,
    :382-383), distance / s inside the map point's range (:388-390)."""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    n = len(pos)
    s, R, t = sim3
    fx, fy, cx, cy = (F32(v) for v in cam)
    min_u, max_u, min_v, max_v = (F32(v) for v in bounds)
    ok = np.zeros(n, bool)
    uv = np.zeros((n, 2), F32)
    octave = np.zeros(n, np.int32)
    for i in range(n):
        pc = pos[i] if Rcw is None else _affine(1.0, Rcw, pos[i], tcw)
        pm = _affine(F32(s), R, pc, t)
        if pm[2] <= 0:
            continue
        x, y = F32(pm[0] / pm[2]), F32(pm[1] / pm[2])                                     # Camera::project (src/Camera.cc:14-22)
        u, v = F32(F32(fx * x) + cx), F32(F32(fy * y) + cy)
        if not (u < max_u and v < max_v and u > min_u and v > min_v):
            continue
        d = F32(np.sqrt(F32(F32(F32(pm[0] * pm[0]) + F32(pm[1] * pm[1])) + F32(pm[2] * pm[2]))) / F32(s))
        if not (d < F32(max_dist[i]) and d > F32(min_dist[i])):
            continue
        ok[i], uv[i], octave[i] = True, (u, v), predict_level(max_dist[i], d, log_sf)
    return ok, uv, octave


def tlc_z(Rcw1, tcw1, Rcw2, tcw2):
    """tlc.z of ORBMatcher::searchByProjection(pFrame1, pFrame2, ..) (src/ORBMatcher.cc:274-276): twc1 = -Rcw1.t() * tcw1,
    tlc = Rcw2 * twc1 + tcw2 -- the products summed in float, alpha / beta applied in double (host/orbfe_dropin.hpp: motionDirection)"""
    R1, t1 = np.asarray(Rcw1, F32).reshape(3, 3), np.asarray(tcw1, F32).reshape(3)
    R2, t2 = np.asarray(Rcw2, F32).reshape(3, 3), np.asarray(tcw2, F32).reshape(3)
    twc1 = np.array([F32(-1.0 * np.float64(s)) for s in _matvec(R1.T, t1)], F32)
    return F32(np.float64(_matvec(R2, twc1)[2]) + np.float64(t2[2]))


def is_in_vision(pos, view_dir, max_dist, min_dist, Rcw, tcw, cam, bounds):
    """MapPoint::isInVision (src/MapPoint.cc:141-171) for one point in the float / double mix of csrc/k_guided.hip's k_project_map_points"""
    pc = _affine(1.0, Rcw, np.asarray(pos, F32).reshape(3), tcw)
    x, y, z = pc
    if z < 0:
        return False
    d = F32(np.sqrt(F32(F32(F32(x * x) + F32(y * y)) + F32(z * z))))
    if not (d < F32(max_dist) and d > F32(min_dist)):
        return False
    fx, fy, cx, cy = (F32(v) for v in cam[:4])
    u, v = F32(F32(F32(x / z) * fx) + cx), F32(F32(F32(y / z) * fy) + cy)
    min_u, max_u, min_v, max_v = (F32(b) for b in bounds)
    if not (u < max_u and v < max_v and u > min_u and v > min_v):
        return False
    vd = _matvec(Rcw, np.asarray(view_dir, F32).reshape(3)).astype(np.float64)
    vabs = F32(np.sqrt(vd[0] * vd[0] + vd[1] * vd[1] + vd[2] * vd[2]))
    dot = vd[0] * np.float64(x) + vd[1] * np.float64(y) + vd[2] * np.float64(z)
    with np.errstate(all="ignore"):
        cos_theta = F32(dot / np.float64(F32(d * vabs)))
    return not cos_theta < F32(0.5)


class MatcherExt:
    """mixed into frontend.ORBMatcher"""

    def _area_best(self, search, uv, octave, desc, th, scale_factors, exclude):
        """findFeaturesInArea(kp, th, octave - 1, octave + 1) + getBestMatch + `dist <= mnMinThreshold && ratio <= mfRatio` (:393-414)"""
        sf2 = np.asarray(scale_factors, F32) ** 2
        radius = (F32(th) * sf2[octave]).astype(F32)
        bi, bd, sd, nc = search(uv, radius, (octave - 1).astype(np.int8), (octave + 1).astype(np.int8), desc, exclude)
        ratio = bd.astype(F32) / sd.astype(F32)
        return bi, (nc > 0) & (bd <= self.mnMinThreshold) & (ratio <= F32(self.mfRatio))

    def searchBySim3Frames(self, ctx, matches, Scm, poseC, poseM, kfC, kfM, th, cam, bounds, scale_factors, search_in=None):
        """ORBMatcher::searchBySim3(mpCurr, mpMatch, matches, g2oScm, th) (src/ORBMatcher.cc:424-484).
        matches: [(queryIdx in C, trainIdx in M)] from the Sim3 solver; Scm = (s, R, t) with p_c = s R p_m + t; poseC / poseM = (Rcw, tcw).
        kfC / kfM: dict(kps [KP_DTYPE], desc [n, 32], pos [n, 3] world positions of the keyframe's map points (rows of features without one
        are ignored), good [n] = map point non-null and not bad, inmap [n], max_dist [n], min_dist [n]).
        Returns the extended match list [(queryIdx, trainIdx)]: the input followed by the new pairs in ascending queryIdx (std::map order)."""
        s, R, t = Scm
        R = np.asarray(R, F32).reshape(3, 3)
        s_inv = F32(F32(1.0) / F32(s))                                                      # Sim3Ret::inv (Sim3Solver.h:36-43)
        Rt = R.T.copy()
        Smc = (s_inv, Rt, (-s_inv * _matvec(Rt, np.asarray(t, F32).reshape(3))).astype(F32))
        log_sf = F32(np.log(F32(scale_factors[1])))
        nc, nm = len(kfC["kps"]), len(kfM["kps"])
        flagC, flagM = np.ones(nc, bool), np.ones(nm, bool)
        for q, tr in matches:
            flagC[q], flagM[tr] = False, False
        new = {}

        def direction(src, dst, flags, pose, sim3, need_inmap_src, forward, search):
            cand = np.flatnonzero(flags & np.asarray(src["good"], bool) & (np.asarray(src["inmap"], bool) if need_inmap_src else True))
            if cand.size == 0:
                return
            ok, uv, octave = sim3_project(np.asarray(src["pos"], F32)[cand], np.asarray(src["max_dist"], F32)[cand],
                                          np.asarray(src["min_dist"], F32)[cand], pose[0], pose[1], sim3, cam, bounds, log_sf)
            cand, uv, octave = cand[ok], uv[ok], octave[ok]
            if cand.size == 0:
                return
            usable_dst = np.asarray(dst["good"], bool) & np.asarray(dst["inmap"], bool)          # vGoodIndices (:396-405)
            bi, keep = self._area_best(search, uv, octave, np.asarray(src["desc"])[cand], th, scale_factors, (~usable_dst).astype(np.uint8))
            for k in np.flatnonzero(keep):
                key, val = (int(cand[k]), int(bi[k])) if forward else (int(bi[k]), int(cand[k]))
                new.setdefault(key, val)                                                           # std::map::insert keeps the first

        def target(dst, tag):   # search_in(tag, ...) lets the logic be exercised without a device
            if search_in is not None:
                return lambda *a: search_in(tag, *a)
            return lambda *a: ctx.search_in_area_features(dst["kps"], dst["desc"], *a)
        # C's map points into M (:448-462), then M's into C (:464-476)
        direction(kfC, kfM, flagC, poseC, Smc, True, True, target(kfM, "M"))
        direction(kfM, kfC, flagM, poseM, (F32(s), R, np.asarray(t, F32).reshape(3)), False, False, target(kfC, "C"))
        return list(matches) + sorted(new.items())

    def searchBySim3MapPoints(self, ctx, kf, loop_mps, matched, Scw, th, cam, bounds, scale_factors, search_in=None):
        """ORBMatcher::searchBySim3(pCurr, vLoopGroupMps, vMatchedMps, g2oScw, th) (src/ORBMatcher.cc:501-559).
        kf: dict(kps, desc) of pCurr; loop_mps: dict(pos [n, 3], view_dir [n, 3], desc [n, 32], max_dist, min_dist, usable [n] = non-null, not
        bad, in map, id [n] = identity of the map point); matched: [nKF] identity of the map point each feature of pCurr is matched
        with, -1 for none (vMatchedMps; entries whose map point is no longer usable do not count, the caller passes -1 for them).
        Returns (assignments [(featIdx, loop map point index)] in loop order -- vMatchedMps[bestMatch.first] = pMp --, nMatches)."""
        s, R, t = Scw
        R = np.asarray(R, F32).reshape(3, 3)
        t = np.asarray(t, F32).reshape(3)
        matched = np.asarray(matched, np.int64)
        already = set(int(v) for v in matched if v >= 0)
        n_matches = int((matched >= 0).sum())
        ids = np.asarray(loop_mps["id"], np.int64)
        cand = np.array([i for i in range(len(ids)) if loop_mps["usable"][i] and int(ids[i]) not in already], np.int64)
        if cand.size == 0:
            return [], n_matches
        log_sf = F32(np.log(F32(scale_factors[1])))
        pos = np.asarray(loop_mps["pos"], F32)[cand]
        ok, uv, octave = sim3_project(pos, np.asarray(loop_mps["max_dist"], F32)[cand], np.asarray(loop_mps["min_dist"], F32)[cand], None, None,
                                      (F32(s), R, t), cam, bounds, log_sf)
        # the viewing-angle test (:534-536): (Rqp * viewDirection) . p3dC >= 0.5 * |p3dC|, dot and norm accumulated in double (cv::Mat::dot, cv::norm)
        vd = np.asarray(loop_mps["view_dir"], F32)[cand]
        for j in np.flatnonzero(ok):
            pc = _affine(F32(s), R, pos[j], t)
            d_with_s = F32(np.sqrt(np.float64(pc[0]) ** 2 + np.float64(pc[1]) ** 2 + np.float64(pc[2]) ** 2))
            rv = _matvec(R, vd[j])
            dot = np.float64(rv[0]) * np.float64(pc[0]) + np.float64(rv[1]) * np.float64(pc[1]) + np.float64(rv[2]) * np.float64(pc[2])
            if dot < 0.5 * np.float64(d_with_s):
                ok[j] = False
        cand, uv, octave = cand[ok], uv[ok], octave[ok]
        if cand.size == 0:
            return [], n_matches
        search = search_in or (lambda *a: ctx.search_in_area_features(kf["kps"], kf["desc"], *a))
        bi, keep = self._area_best(search, uv, octave, np.asarray(loop_mps["desc"])[cand], th, scale_factors, None)
        out = [(int(bi[k]), int(cand[k])) for k in np.flatnonzero(keep)]
        return out, n_matches + len(out)

    def fuseMapPoints(self, ctx, kf, kf_state, mps, th=3.0, bLoop=False, scale_factors=None, search_in=None):
        """ORBMatcher::fuse(pkf1, mapPoints, map, bLoop, th) (src/ORBMatcher.cc:682-707): the map points already held by the keyframe are
        dropped (:687-701), the rest go through searchByProjection(pkf1, vMapPoints, th, matches, true) against the keyframe's features,
        then processFuseMps.  kf: dict(kps, desc); kf_state: dict(good [n], id [n], obs [n]) of the keyframe's map points; mps: dict(id,
        good, obs, usable [m] = in map, not bad, in vision of pkf1, uv [m, 2], level [m], cos_theta [m], desc [m, 32]) -- uv / level /
        cos_theta from ORBMatcher.projectMapPoints.  Returns (actions, nFuse) of processFuseMps; action indices refer to `mps`."""
        held = set(int(i) for i, g in zip(kf_state["id"], kf_state["good"]) if g)
        sel = np.array([i for i in range(len(mps["id"])) if int(mps["id"][i]) not in held], np.int64)
        if sel.size == 0:
            return [], 0
        search = search_in or (lambda *a: ctx.search_in_area_features(kf["kps"], kf["desc"], *a))
        matches, _ = self.searchByProjectionMapPoints(ctx, 0, np.asarray(mps["uv"], F32)[sel], np.asarray(mps["level"])[sel],
                                                      np.asarray(mps["cos_theta"], F32)[sel], np.asarray(mps["desc"])[sel],
                                                      np.asarray(mps["usable"], bool)[sel], th, np.zeros(len(kf["kps"]), bool), True,
                                                      scale_factors=scale_factors, area_search=search)
        matches = [(f, int(sel[m]), d) for f, m, d in matches]
        return self.processFuseMps(matches, kf_state["good"], kf_state["id"], mps["good"], mps["id"], kf_state["obs"], mps["obs"], bLoop)

    def fuseFrames(self, ctx, kf1, kf1_state, kf2_kps, kf2_desc, kf2_state, in_vision2, z, bl, scale_factors, search_in=None):
        """ORBMatcher::fuse(pkf1, pkf2, map) (src/ORBMatcher.cc:716-724): searchByProjection(pkf1, pkf2, matches, 3.0f, true) + processFuseMps.
        kf2_state: dict(good, id, obs) per feature of pkf2; in_vision2 [n2]: the map point of feature idx is in vision of pkf1 (:283-288)."""
        search = search_in or (lambda *a: ctx.search_in_area_features(kf1["kps"], kf1["desc"], *a))
        matches = self.searchByProjectionFrames(ctx, 0, scale_factors, kf2_kps, kf2_desc, kf2_state["good"], np.zeros(len(kf1["kps"]), bool), 3.0,
                                                z, bl, True, in_vision2, area_search=search)
        return self.processFuseMps(matches, kf1_state["good"], kf1_state["id"], kf2_state["good"], kf2_state["id"], kf1_state["obs"],
                                   kf2_state["obs"], False)

    def fuseIntoKeyframes(self, ctx, model, cur_kf, target_kfs, cur, pts, targets, z, cam, bl, scale_factors, th=3.0, search_in=None,
                          reevaluate=True):
        """The loop `for pkf in sTargetKfs: matcher.fuse(pkf, cur, map)` of LocalMapping::fuseMapPoints (src/LocalMapping.cc:401-402) from
        ONE batch call (Context.fuse_into_keyframes; search_in(cur, pts, targets, z, cam, bl, scale_factors, th, ratio, dist_threshold)
        replaces it without a device) and a sequential replay on `model`, a small mutable map:
            model.slot(kf, i) -> point id or -1        model.is_bad(pid)        model.n_obs(pid)        model.in_vision(pid, kf)
            model.set_slot(kf, i, pid)                 model.add_observation(pid, kf, i)                model.replace(keep, drop)
        cur_kf / target_kfs name the keyframes in the model; cur / pts / targets / z are their arrays as the binding takes them, pts
        describing the points model.slot(cur_kf, i) at call time.
        Why one batch is enough: with bFuse the search of (target k, feature i) uses cur's feature position and descriptor only
        (src/ORBMatcher.cc:297-313), so no MapPoint::replace of an earlier fuse can change it.  Only isInVision depends on the map, and the
        batch's visible[k][i] is used iff slot i still holds the point it held at call time AND that point has not survived a replace
        since (its view direction is recomputed there, src/MapPoint.cc:229-230); otherwise the live point is re-evaluated (counted).
        Per target, in the caller's order: the match list in ascending i from the live slots (point present and not bad, visible,
        best_idx >= 0), then processFuseMps (:623-663) on the snapshots of both keyframes' slots with isBad / getObsNum read live, as the
        reference's objects give them.
        reevaluate = False uses the batch flag everywhere (what a stale flag would do; for tests).
        Returns (nFuse per target, dict(device_flags, reevaluated))."""
        if search_in is not None:
            bi, bd, vis = search_in(cur, pts, targets, z, cam, bl, scale_factors, th, self.mfRatio, self.mnMinThreshold)
        else:
            bi, bd, vis = ctx.fuse_into_keyframes(cur, pts, targets, z, cam, bl, scale_factors, th, self.mfRatio, self.mnMinThreshold)
        n = len(cur["kps"])
        at_call = [model.slot(cur_kf, i) for i in range(n)]
        survived = set()
        stats = dict(device_flags=0, reevaluated=0)
        n_fuse = []
        for k, kf in enumerate(target_kfs):
            v_ids = [model.slot(cur_kf, i) for i in range(n)]                                     # mps2 / vMapPoints (:282, :721)
            matches = []
            for i in range(n):
                pid = v_ids[i]
                if pid < 0 or model.is_bad(pid):
                    continue
                if not reevaluate or (pid == at_call[i] and pid not in survived):
                    visible = bool(vis[k][i])
                    stats["device_flags"] += 1
                else:
                    visible = model.in_vision(pid, kf)
                    stats["reevaluated"] += 1
                if visible and bi[k][i] >= 0:
                    matches.append((int(bi[k][i]), i, int(bd[k][i])))
            f_ids = {q: model.slot(kf, q) for q in set(m[0] for m in matches)}                    # fMapPoints (:720): the slots the loop reads
            nf = 0
            for q, tr, _ in matches:
                p1, p2 = f_ids[q], v_ids[tr]
                if p2 < 0 or model.is_bad(p2):
                    continue
                if p1 < 0 or model.is_bad(p1):
                    model.set_slot(kf, q, p2)
                    model.add_observation(p2, kf, q)
                    nf += 1
                elif p1 != p2:
                    keep, drop = (p1, p2) if model.n_obs(p1) >= model.n_obs(p2) else (p2, p1)
                    model.replace(keep, drop)
                    survived.add(keep)
                    nf += 1
            n_fuse.append(nf)
        return n_fuse, stats

    def fusePointsIntoKeyframes(self, ctx, model, target_kfs, point_ids, store, cam, scale_factors, th=4.0, bLoop=True, search_in=None,
                                reevaluate=True, max_kf=64, max_pairs=1 << 22):
        """The loop `for pkf in target_kfs: matcher.fuse(pkf, points, map, bLoop, th)` of LoopClosing::correctLoop (src/LoopClosing.cc:515-517;
        ORBMatcher::fuse, src/ORBMatcher.cc:682-707) from ONE device call (Context.fuse_points_into_keyframes_stored over the keyframes
        target_kfs of `store`; search_in(target_kfs, poses, pts, cam, scale_factors, th, ratio, dist_threshold) -> (best_idx, best_dist)
        replaces it without a device) and a sequential replay on `model`, the small mutable map of fuseIntoKeyframes with, besides:
            model.in_map(pid)      model.pose(kf) -> (Rcw, tcw)      model.held(kf) -> the good points in kf's slots
            model.point_arrays(pids) -> the arrays of the call for the points as they are NOW (-1: a null pointer)
        point_ids: the map points in the caller's order.  More than max_kf keyframes or max_pairs pairs go in several calls, all issued
        before the replay starts.
        Why one call is enough: entry (k, j) is a function of point j's position, view direction, distance range and descriptor and of
        keyframe k's pose, bounds and features.  The poses are fixed before the loop, addObservation changes none of the point's fields,
        and MapPoint::replace(keep, drop) recomputes only `keep`'s descriptor, normal and depth (src/MapPoint.cc:229-230): an entry is
        valid exactly while point j has not been the `keep` of a replace since the call.  Per target, in order: vMapPoints = the points
        the keyframe does not hold NOW (:687-701); those of them that are live-good, in the map and have survived a replace are searched
        again (one further call with that keyframe alone and their live arrays); the match list in ascending position in vMapPoints;
        processFuseMps (:623-663) on a snapshot of the keyframe's slots with isBad / getObsNum read live.
        reevaluate = False uses the stale entries (for tests).
        Returns (nFuse per target, dict(device_entries, reevaluated, extra_calls))."""
        def search(kfs, pts):
            poses = [model.pose(kf) for kf in kfs]
            if search_in is not None:
                return search_in(kfs, poses, pts, cam, scale_factors, th, self.mfRatio, self.mnMinThreshold)
            return ctx.fuse_points_into_keyframes_stored(store, kfs, poses, pts, cam, scale_factors, th, self.mfRatio, self.mnMinThreshold)

        m = len(point_ids)
        at_call = model.point_arrays(point_ids)
        per_call = max(1, min(max_kf, max_pairs // max(m, 1)))
        bi, bd = [], []
        for k0 in range(0, len(target_kfs), per_call):
            a, b = search(list(target_kfs[k0:k0 + per_call]), at_call)
            bi.extend(a)
            bd.extend(b)
        survived = set()
        stats = dict(device_entries=0, reevaluated=0, extra_calls=0)
        n_fuse = []
        for k, kf in enumerate(target_kfs):
            held = model.held(kf)
            v = [j for j in range(m) if point_ids[j] not in held]                                  # vMapPoints (:695-701), as positions in the list
            live = [j for j in v if point_ids[j] >= 0 and not model.is_bad(point_ids[j]) and model.in_map(point_ids[j])]
            again = [j for j in live if point_ids[j] in survived] if reevaluate else []
            fresh = {}
            if again:
                a, b = search([kf], model.point_arrays([point_ids[j] for j in again]))
                fresh = {j: (int(a[0][q]), int(b[0][q])) for q, j in enumerate(again)}
                stats["extra_calls"] += 1
                stats["reevaluated"] += len(again)
            stats["device_entries"] += len(live) - len(again)
            where = {j: p for p, j in enumerate(v)}
            matches = []
            for j in live:
                f, d = fresh[j] if j in fresh else (int(bi[k][j]), int(bd[k][j]))
                if f >= 0:
                    matches.append((f, where[j], d))
            f_ids = {q: model.slot(kf, q) for q in set(mt[0] for mt in matches)}                    # fMapPoints (:703): the slots the loop reads
            nf = 0
            for q, p, _ in matches:
                p1, p2 = f_ids[q], point_ids[v[p]]
                if p2 < 0 or model.is_bad(p2):
                    continue
                if p1 < 0 or model.is_bad(p1):
                    model.set_slot(kf, q, p2)
                    model.add_observation(p2, kf, q)
                    nf += 1
                elif p1 != p2:
                    keep, drop = (p2, p1) if bLoop or model.n_obs(p1) < model.n_obs(p2) else (p1, p2)
                    model.replace(keep, drop)
                    survived.add(keep)
                    nf += 1
            n_fuse.append(nf)
        return n_fuse, stats

    def searchForTriangulation(self, ctx, bow_args, kps1, kps2, pose1, pose1_inv, pose2, pose2_inv, k_inv, scale_factors):
        """ORBMatcher::searchForTriangulation (src/ORBMatcher.cc:736-787): searchByBow(pkf1, pkf2, matches, true) -- bow_args are the
        keyword arguments of ORBMatcher.searchByBow for (frame = pkf1, keyframe = pkf2) -- then the mutual epipolar test."""
        matches = self.searchByBow(ctx, bAddMPs=True, **bow_args)
        if not matches:
            return []
        return self.epipolarFilter(matches, kps1, kps2, pose1, pose1_inv, pose2, pose2_inv, k_inv, scale_factors)

    @staticmethod
    def processFuseMps(matches, f_good, f_id, v_good, v_id, f_obs, v_obs, bLoop=False):
        """ORBMatcher::processFuseMps (src/ORBMatcher.cc:623-661): what to do with every match (queryIdx = feature of pkf1, trainIdx = map
        point index) given which features of pkf1 carry a good map point (f_good, identity f_id, observation count f_obs) and the same for
        the projected map points.  Returns (actions, nFuse): ("add", featIdx, mpIdx) = setMapPoint + addObservation,
        ("replace", keep_id, drop_id) = MapPoint::replace(keep, drop, map).  Within one call the map changes are NOT fed back into later
        decisions, exactly like the reference, which works on the copies taken before the loop (:705-706, :727-729)."""
        actions, n = [], 0
        for q, tr, *_ in matches:
            if not v_good[tr]:
                continue
            if not f_good[q]:
                actions.append(("add", int(q), int(tr)))
                n += 1
            elif f_id[q] != v_id[tr]:
                if bLoop:
                    actions.append(("replace", int(v_id[tr]), int(f_id[q])))
                elif f_obs[q] >= v_obs[tr]:
                    actions.append(("replace", int(f_id[q]), int(v_id[tr])))
                else:
                    actions.append(("replace", int(v_id[tr]), int(f_id[q])))
                n += 1
        return actions, n

    @staticmethod
    def epipolarFilter(matches, kps1, kps2, pose1, pose1_inv, pose2, pose2_inv, k_inv, scale_factors):
        """The second half of ORBMatcher::searchForTriangulation (src/ORBMatcher.cc:739-786): F21 = KInv^T [t21]x R21 KInv from the 4x4
        float poses (T21 = Tcw2 * Twc1), keep a match iff both point-to-epipolar-line distances are within 5.991 * scale^2 of the octave.
        matches: [(queryIdx in kf1, trainIdx in kf2, ...)] from searchByBow(pkf1, pkf2, matches, true)."""
        T21, T12 = _matmul(pose2, pose1_inv), _matmul(pose1, pose2_inv)
        K = np.asarray(k_inv, F32).reshape(3, 3)

        def fundamental(T):
            Rm, tv = T[:3, :3], T[:3, 3]
            ssm = np.array([[0, -tv[2], tv[1]], [tv[2], 0, -tv[0]], [-tv[1], tv[0], 0]], F32)
            return _matmul(_matmul(_matmul(K.T.copy(), ssm), Rm), K)
        F21, F12 = fundamental(T21), fundamental(T12)
        sf2 = np.asarray(scale_factors, F32) ** 2

        def dist(p_line, Fm, p):
            """point2LineDistance(pt_line^T * F, p) (:789-795): |param . point| / sqrt(a^2 + b^2), the dot in double (cv::Mat::dot)"""
            prm = _matmul(np.asarray(p_line, F32).reshape(1, 3), Fm)[0]
            dot = np.float64(prm[0]) * np.float64(p[0]) + np.float64(prm[1]) * np.float64(p[1]) + np.float64(prm[2]) * np.float64(p[2])
            return F32(F32(abs(dot)) / F32(np.sqrt(F32(F32(prm[0] * prm[0]) + F32(prm[1] * prm[1])))))
        out = []
        for m in matches:
            k1, k2 = kps1[m[0]], kps2[m[1]]
            p1, p2 = np.array([k1["x"], k1["y"], 1], F32), np.array([k2["x"], k2["y"], 1], F32)
            if dist(p2, F21, p1) > F32(5.991 * np.float64(sf2[k1["octave"]])):
                continue
            if dist(p1, F12, p2) > F32(5.991 * np.float64(sf2[k2["octave"]])):
                continue
            out.append(m)
        return out
