"""LocalMapping::createNewMapPoints restated (tests/triangulation_restatement.py): known answers, one case per quirk T1-T9, agreement
with the existing matcher code, the SVD decision, and the C-ABI's behaviour without a device.  No GPU needed."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tri_scenes as ts  # noqa: E402
import triangulation_restatement as tr  # noqa: E402
from orb_slam2_ros2_amd._lib import KP_DTYPE, OrbfeError  # noqa: E402
from orb_slam2_ros2_amd.frontend import ORBMatcher  # noqa: E402

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cur, nbs, bl=ts.BL):
    return tr.create_new_map_points(cur, nbs, ts.CAM, ts.k_inv(), bl, ts.SF)[:3]


def proj(T, P):
    fx, fy, cx, cy = (float(v) for v in ts.CAM)
    pc = T[:3, :3].astype(np.float64) @ P + T[:3, 3]
    return fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy


def hand_kf(T, feats, unproc=None):
    """a keyframe from [(x, y, desc byte, node, depth, right_u, flags)]; feature i sits in node feats[i][3]"""
    Tcw, Twc, Ow = T
    n = len(feats)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = [f[0] for f in feats]
    kps["y"] = [f[1] for f in feats]
    kps["size"], kps["class_id"] = 7.0, -1
    desc = np.zeros((n, 32), np.uint8)
    for i, f in enumerate(feats):
        desc[i, :] = f[2]
    kf = dict(kps=kps, desc=desc, fv=ts.csr_from_nodes([f[3] for f in feats]), depth=np.array([f[4] for f in feats], np.float64),
              right_u=np.array([f[5] for f in feats], np.float64), flags=np.array([f[6] for f in feats], np.uint8), Tcw=Tcw, Twc=Twc, Ow=Ow)
    kf["unproc"] = np.zeros(n, bool) if unproc is None else np.array([u is not None for u in unproc])
    kf["unproc_pos"] = np.array([u if u is not None else (0, 0, 0) for u in (unproc or [None] * n)], F32)
    return kf


P0 = np.array([0.3, -0.2, 8.0])


def t4_scene():
    """one neighbour, two of its features match the same current feature: the first (a wrong stereo depth) is rejected, the second
    (triangulated) accepted"""
    C, N = ts.pose((0, 0, 0)), ts.pose((0.5, 0, 0))
    u1, v1 = proj(C[0], P0)
    u2, v2 = proj(N[0], P0)
    cur = hand_kf(C, [(u1, v1, 7, 5, -1, -1, 0), (100, 100, 200, 9, -1, -1, 0)])
    nb = hand_kf(N, [(u2, v2, 7, 5, 4.0, u2 - 60, 0), (u2, v2, 7, 5, -1, -1, 0), (400, 300, 99, 9, -1, -1, 0)])
    return cur, [nb]


def t5_scene(second=True):
    """the current feature's own stereo branch takes its unprocessed point (placed wrong, so rejected); a later neighbour-stereo
    candidate still wins, and the tail does not restore the point"""
    C, A, B = ts.pose((0, 0, 0)), ts.pose((0.5, 0, 0)), ts.pose((-0.5, 0, 0))
    u1, v1 = proj(C[0], P0)
    ua, va = proj(A[0], P0)
    ub, vb = proj(B[0], P0)
    cur = hand_kf(C, [(u1, v1, 7, 5, 8.0, u1 - 60, 0)], unproc=[tuple(P0 + (0.5, 0, 0))])
    na = hand_kf(A, [(ua, va, 7, 5, -1, -1, 0)])
    nb = hand_kf(B, [(ub, vb, 7, 5, 8.0, ub - 80, 0)])
    return cur, ([na, nb] if second else [na])


# ---- known answers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nb", [1, 4])
def test_known_answers(n_nb):
    cur, nbs, pts = ts.scene(11, n_nb=n_nb, n=400, n_pts=1200, baselines=[0.8, 1.0, 0.6, 0.9][:n_nb], px_noise=0.0, flip_bits=2)
    recs, _, _ = run(cur, nbs)
    tri = recs[recs["kind"] == tr.KIND_TRI]
    assert len(tri) > 50
    truth = pts[cur["pid"][tri["q"]]]
    rel = np.abs(tri["xyz"] - truth).max(1) / np.linalg.norm(truth, axis=1)
    assert np.all(rel < 1e-3)
    # first wins: one record per current feature, records in neighbour order
    assert len(np.unique(recs["q"])) == len(recs) and np.all(np.diff(recs["nb"]) >= 0)


# ---- one case per quirk ---------------------------------------------------------------------------------------------------------
def _kp(x, y, o=0):
    k = np.zeros(1, KP_DTYPE)[0]
    k["x"], k["y"], k["octave"] = x, y, o
    return k


def test_t1_second_error_uses_kp1_y():
    C, N = ts.pose((0, 0, 0)), ts.pose((0, 0.5, 0))
    u1, v1 = proj(C[0], P0)
    u2, v2 = proj(N[0], P0)
    assert abs(v1 - v2) > 10
    chk = lambda k1, k2: tr.check_map_point(P0.astype(F32), C[0], N[0], k1, k2, ts.SF, ts.CAM)   # noqa: E731
    assert not chk(_kp(u1, v1), _kp(u2, v2))           # kp2.y would accept: consistent views, rejected through kp1.y
    C2 = ts.pose((0.5, 0, 0))
    u3, v3 = proj(C2[0], P0)
    assert abs(v3 - v1) < 1e-3
    assert tr.check_map_point(P0.astype(F32), C[0], C2[0], _kp(u1, v1), _kp(u3, v3 + 10), ts.SF, ts.CAM)   # kp2.y would reject


def test_t4_rejected_repeat_does_not_block():
    cur, nbs = t4_scene()
    per = tr.match_neighbour(cur, nbs[0], ts.k_inv(), ts.SF)
    assert [(m[0], m[1]) for m in per] == [(0, 0), (0, 1)]
    recs, tail, _ = run(cur, nbs)
    assert len(recs) == 1 and (recs[0]["q"], recs[0]["t"], recs[0]["kind"]) == (0, 1, tr.KIND_TRI)


def test_t5_consume_and_reject():
    cur, nbs = t5_scene()
    recs, tail, _, consumed = tr.create_new_map_points(cur, nbs, ts.CAM, ts.k_inv(), ts.BL, ts.SF)
    assert len(recs) == 1 and (recs[0]["nb"], recs[0]["kind"]) == (1, tr.KIND_NB) and len(tail) == 0 and list(consumed) == [True]
    cur, nbs = t5_scene(second=False)
    recs, tail, _ = run(cur, nbs)
    assert len(recs) == 0 and len(tail) == 0                    # consumed: not restored although the slot stays empty
    recs, tail, _ = run(cur, [])
    assert list(tail) == [0]                                    # T6: not consumed, slot empty -> restored


def test_t7_baseline():
    cur, nbs, _ = ts.scene(2, n_nb=2, n=500, n_pts=1500, baselines=[0.3, 0.3])
    assert len(run(cur, nbs)[0]) > 0
    d = float(np.linalg.norm(cur["Ow"] - nbs[0]["Ow"]))
    assert all(len(p) == 0 for p in run(cur, nbs[:1], bl=F32(d * 1.01))[2])
    assert len(run(cur, nbs[:1], bl=F32(d * 0.99))[2][0]) > 0


def test_t8_branches():
    C, R = ts.pose((0, 0, 0)), ts.pose((0, 0, 0), ts.yaw(0.05))
    u1, v1 = proj(C[0], P0)
    u2, v2 = proj(R[0], P0)
    cur = hand_kf(C, [(u1, v1, 7, 5, -1, -1, 0)])
    nb = hand_kf(R, [(u2, v2, 7, 5, -1, -1, 0)])
    cam = ts.CAM
    c = cur
    assert tr.cos_theta(C[0][:3, :3], R[0][:3, :3], (cur["kps"][0]["x"], cur["kps"][0]["y"]), (nb["kps"][0]["x"], nb["kps"][0]["y"]), cam) >= 0.9998
    assert tr.candidate(c, nb, 0, 0, cam, ts.SF)[0] == 0                      # pure rotation, no stereo: no point
    cur2 = hand_kf(C, [(u1, v1, 7, 5, 8.0, u1 - 30, 0)])
    nb2 = hand_kf(R, [(u1, v1, 7, 5, 8.0, u1 - 30, 0)])
    assert tr.candidate(cur2, nb2, 0, 0, cam, ts.SF)[0] == 0   # cos1 == cos2: no point


def test_t9_negative_world_z():
    C, N = ts.pose((0, 0, 0), ts.yaw(np.pi)), ts.pose((0.5, 0, 0), ts.yaw(np.pi))
    P = np.array([0.3, -0.2, -8.0])
    k1, k2 = _kp(*proj(C[0], P)), _kp(*proj(N[0], P))
    ok, pts = tr.solve_null(tr.tri_matrix(C[0], N[0], k1, k2, ts.CAM)[None])
    assert not ok[0]
    ok, pts = tr.solve_null(tr.tri_matrix(ts.pose((0, 0, 0))[0], ts.pose((0.5, 0, 0))[0], _kp(*proj(ts.pose((0, 0, 0))[0], P0)),
                                          _kp(*proj(ts.pose((0.5, 0, 0))[0], P0)), ts.CAM)[None])
    assert ok[0] and np.allclose(pts[0], P0, rtol=1e-4)


# ---- agreement with the existing matcher code ------------------------------------------------------------------------------------
def test_matching_equals_search_by_bow_and_epipolar_filter():
    cur, nbs, _ = ts.scene(9, n_nb=2, n=500, n_pts=1500)
    m = ORBMatcher(0.6, False)
    for nb in nbs:
        bow = dict(desc_f=cur["desc"], desc_kf=nb["desc"], featvec_f=tr.featvec_dict(cur["fv"]), featvec_kf=tr.featvec_dict(nb["fv"]),
                   good_f=(cur["flags"] & 1) != 0, inmap_f=(cur["flags"] & 2) != 0, good_kf=(nb["flags"] & 1) != 0, inmap_kf=(nb["flags"] & 2) != 0)
        raw = m.searchByBow(None, bAddMPs=True, best_match=tr.best_match_numpy, **bow)
        # the numpy getBestMatch is the plain loop over the candidates
        for q, t, d in raw[:50]:
            assert d == ORBMatcher.descDistance(cur["desc"][q], nb["desc"][t]) and d <= 50
        want = m.epipolarFilter(raw, cur["kps"], nb["kps"], cur["Tcw"], cur["Twc"], nb["Tcw"], nb["Twc"], ts.k_inv(), ts.SF)
        assert tr.match_neighbour(cur, nb, ts.k_inv(), ts.SF) == want and 0 < len(want) < len(raw) + 1


# ---- the SVD decision ------------------------------------------------------------------------------------------------------------
def test_svd_decision_against_numpy():
    rng = np.random.default_rng(3)
    As = []
    for _ in range(200):
        U, _ = np.linalg.qr(rng.normal(size=(4, 4)))
        V, _ = np.linalg.qr(rng.normal(size=(4, 4)))
        s = np.array([rng.uniform(500, 1000), rng.uniform(100, 400), rng.uniform(10, 90), rng.uniform(0, 1e-3)])
        As.append((U * s) @ V.T)
    As = np.array(As, F32)
    w, V = tr.pr.jacobi(np.einsum("hki,hkj->hij", As.astype(np.float64), As.astype(np.float64)))
    for h in range(len(As)):
        _, sv, vt = np.linalg.svd(As[h].astype(np.float64))
        m = int(np.argmin(w[h]))
        got = V[h, :, m] / V[h, 3, m]
        assert np.allclose(got, vt[3] / vt[3, 3], rtol=1e-4, atol=1e-5)
        s2 = np.sort(w[h])[1]
        assert np.isclose(np.sqrt(max(w[h, m], 0)) / np.sqrt(s2), sv[3] / sv[2], rtol=1e-2, atol=1e-6)


# ---- no device --------------------------------------------------------------------------------------------------------------------
def test_create_new_map_points_fails_loudly_without_device():
    """the new entry point itself: without a context (none can be made without a device) it refuses with EBADARG and its own message,
    and Context.create_new_map_points is never reached because the context raises EDEVICE"""
    import ctypes as C
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    from orb_slam2_ros2_amd import _lib
    L = _lib.load()
    nr, nt = C.c_int64(-1), C.c_int64(-1)
    st = L.orbfe_create_new_map_points(None, None, 0, None, None, None, 0.0, None, 8, None, 0, C.byref(nr), None, 0, C.byref(nt), None)
    assert st == 1 and b"create_new_map_points" in L.orbfe_last_error(None)
    with pytest.raises(OrbfeError) as ei:
        _lib.Context(640, 480, n_features=500, n_levels=4, device_id=0, max_images=1)
    assert ei.value.status == 3


# ---- the drop-in through the compiler ---------------------------------------------------------------------------------------------
REF = "/root/reference/src/ORB_SLAM2"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "ORB_SLAM2")) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++")
def test_dropin_compiles_against_the_reference_headers(tmp_path):
    """g++ -fsyntax-only of orbfe_mapping_dropin.hpp with the reference's LocalMapping.h / KeyFrame.h / MapPoint.h / Map.h (symlinks; Frame.h /
    KeyFrame.h as temporary copies with INTEGRATION section 3's friend line) and LocalMapping::createNewMapPoints as its one-line body"""
    from test_reference_compile import _include_dir
    inc = _include_dir(str(tmp_path / "inc"), friend_line=True)
    tu = tmp_path / "tu.cpp"
    tu.write_text(r"""
#include <string>
#include <opencv2/opencv.hpp>
namespace cv {
inline void destroyWindow(const std::string&) {}
}
#include "ORB_SLAM2/Camera.h"
#include "ORB_SLAM2/Frame.h"
#include "ORB_SLAM2/KeyFrame.h"
#include "ORB_SLAM2/Map.h"
#include "ORB_SLAM2/MapPoint.h"
#include "ORB_SLAM2/LocalMapping.h"
#include "orbfe_mapping_dropin.hpp"
namespace ORB_SLAM2_ROS2 {
void LocalMapping::createNewMapPoints() { orbfe::dropin::createNewMapPoints<Camera, Frame>(mpCurrKeyFrame, mmUnprocessMps, mpMap, mlpAddedMPs); }
}  // namespace ORB_SLAM2_ROS2
""")
    stubs = os.path.join(ROOT, "tests", "cpp", "stubs")
    host = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + inc, "-I" + stubs, "-I" + os.path.join(stubs, "refgen"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + host, str(tu)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
