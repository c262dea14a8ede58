"""trackReference over a stored keyframe (orbfe_track_reference_stored) without a device: the restatement of
track_reference_restatement.py on a hand-made scene with answers worked out by hand, the scene builders' claims (every verdict, the
boundary counts with their chi-square margins, what each shape scene is there for), the surface -- header, export, binding, ABI version,
the C layout of the two records -- and the drop-in body against the reference's real class declarations."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_reference_restatement as tr  # noqa: E402
import track_reference_scenes as sc  # noqa: E402
import tri_scenes as ts  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN = tr.OWN


# ---- a dozen features, by hand ---------------------------------------------------------------------------------------------------------
def hand_scene(own_off=False):
    """Twelve frame features with unrelated random descriptors R_f, feature f in node 1 + f % 3, at the pixel its point projects to under
    the identity pose.  Features 5, 10 and 11 arrive holding points of their own.  Six keyframe features:
      0, 1  both copy R_3 (node 1): two matches name frame feature 3, the later one keeps it
      2     copies R_5 (node 3): feature 5 holds a point and is no candidate; the node's other features are far: no match
      3, 4  copy R_7 (node 2) and R_8 (node 3)
      5     copies R_9 (node 1) but its point is bad: it does not search
    so the list is (3, 0), (3, 1) of node 1, then (7, 3) of node 2, then (8, 4) of node 3: four matches, distance 0."""
    from orb_slam2_ros2_amd._lib import KP_DTYPE
    rng = np.random.default_rng(12)
    R = rng.integers(0, 256, (12, 32), dtype=np.uint8)
    kps = np.zeros(12, KP_DTYPE)
    kps["x"], kps["y"] = 200 + 70 * np.arange(12), 100 + 15 * np.arange(12)
    kps["size"], kps["class_id"] = 31.0, -1
    z = 8.0 + np.arange(12) % 4
    X = np.stack([(kps["x"] - sc.CX) / sc.FX * z, (kps["y"] - sc.CY) / sc.FY * z, z], 1).astype(np.float32)
    src = np.array([3, 3, 5, 7, 8, 9])
    kf_kps = kps[src].copy()
    frame_good = np.zeros(12, np.uint8)
    frame_good[[5, 10, 11]] = 1
    frame_pos = np.zeros((12, 3), np.float32)
    frame_pos[[5, 10, 11]] = X[[5, 10, 11]]
    if own_off:
        frame_pos[5] += np.float32(4.0)
    node = lambda f: 1 + np.asarray(f) % 3
    return dict(nf=12, n_kp=12, kps=kps, desc=R, right_u=None, kf_kps=kf_kps, kf_desc=R[src].copy(), kf_fv=ts.csr_from_nodes(node(src)),
                good=np.array([1, 1, 1, 1, 1, 0], np.uint8), pos=X[src].copy(), frame_good=frame_good, frame_pos=frame_pos,
                Rcw=np.eye(3, dtype=np.float32).reshape(9), tcw=np.zeros(3, np.float32), cam=sc.CAM, bounds=sc.BOUNDS, sigma2=sc.SIGMA2,
                inv_sigma2=sc.INV_SIGMA2), ts.csr_from_nodes(node(np.arange(12)))


def test_the_restatement_on_a_scene_worked_out_by_hand(orc):
    s, fv = hand_scene()
    want_matches = [(3, 0, 0), (3, 1, 0), (7, 3, 0), (8, 4, 0)]
    want_assigned = [-1, -1, -1, 1, -1, OWN, -1, 3, 4, -1, OWN, OWN]
    # the decision of Tracking.cc:365 falls after the frame was written: four matches are too few, and the frame has them all the same
    o = tr.track(orc, s, fv=fv)
    assert o["verdict_name"] == "REJECT_MATCHES" and o["matches"] == want_matches and o["assigned"].tolist() == want_assigned
    assert o["final_assigned"].tolist() == want_assigned and o["n_edges"] == 0 and o["n_inliers"] == 0
    assert not o["inlier"].any() and not o["pose_se3"].any() and not o["Tcw"].any()
    # with a minimum of four the optimisation runs on six edges in feature order, the frame's own points among them; every point is exact
    o = tr.track(orc, s, fv=fv, min_matches=4, min_inliers=6)
    assert o["verdict_name"] == "ACCEPT" and o["n_edges"] == 6 and o["n_inliers"] == 6 and np.flatnonzero(o["inlier"]).tolist() == [3, 5, 7, 8, 10, 11]
    assert o["final_assigned"].tolist() == want_assigned and np.abs(o["pose_se3"] - [0, 0, 0, 1, 0, 0, 0]).max() < 1e-6
    ef, X, meas, _, _ = tr.edge_arrays(s, o["assigned"])
    assert ef.tolist() == [3, 5, 7, 8, 10, 11] and np.array_equal(X[0], s["pos"][1].astype(np.float64)) and np.array_equal(X[1], s["frame_pos"][5].astype(np.float64))
    assert (meas[:, 2] == -1).all()
    o = tr.track(orc, s, fv=fv, min_matches=4, min_inliers=7)
    assert o["verdict_name"] == "REJECT_INLIERS" and o["n_inliers"] == 6
    # the frame's own point metres off: it is an edge, the optimisation throws it out, the feature comes back empty
    s2, _ = hand_scene(own_off=True)
    o = tr.track(orc, s2, fv=fv, min_matches=4, min_inliers=5)
    assert o["n_edges"] == 6 and o["n_inliers"] == 5 and o["assigned"][5] == OWN and o["final_assigned"][5] == -1 and o["verdict_name"] == "ACCEPT"
    # without the orientation check the list is the raw one, in the same order (every pair has the same angle)
    assert tr.track(orc, s, fv=fv, check_orientation=False)["matches"] == want_matches


# ---- the scenes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.VERDICT_SCENES))
def test_the_restatement_reaches_every_verdict(orc, name):
    s, o = sc.restated(orc, name)
    assert o["verdict_name"] == name
    if name == "REJECT_MATCHES":
        assert o["n_matches"] == 9 and (o["assigned"] >= 0).sum() > 0 and np.array_equal(o["assigned"], o["final_assigned"]) and o["n_edges"] == 0
    if name == "REJECT_INLIERS":
        assert o["n_matches"] >= 10 and o["n_inliers"] == 9 and o["n_edges"] >= 20       # the points moved metres off were matched and thrown out
    if name == "ACCEPT":
        assert o["n_inliers"] > 100 and o["n_edges"] > o["n_inliers"] + 5 and len(s["good"]) > 300 and len(s["kf_fv"][0]) > 50
    assert sc.margins(orc, s, o) > 0.01


@pytest.mark.parametrize("name", list(sc.BOUNDARY_SCENES))
def test_boundary_scenes(orc, name):
    """the builder has asserted the count and the 1 % chi-square margin; both once more, and the verdict"""
    s, o = sc.restated(orc, name)
    kind, want = name.split("_")
    assert (o["n_matches"] if kind == "matches" else o["n_inliers"]) == int(want)
    assert o["verdict_name"] == sc.BOUNDARY_SCENES[name][1]
    assert sc.margins(orc, s, o) > 0.01
    if kind == "inliers":
        assert o["n_matches"] >= 10
    # no post-checked projection near a bound
    if o["n_edges"]:
        ef, inl = o["edge_inlier"]
        c = tr.post_check(s, o["assigned"], ef, inl, o["pose_se3"])
        d = np.concatenate([np.abs(c["u"]), np.abs(c["u"] - np.float32(sc.W)), np.abs(c["v"]), np.abs(c["v"] - np.float32(sc.H)), np.abs(c["z"])])
        assert d.min() > 1e-3


def test_shape_scenes_are_what_they_claim(orc):
    s, o, _ = sc.shape(orc, "dup")
    qs = [m[0] for m in o["matches"]]
    twice = [f for f in set(qs) if qs.count(f) == 2]
    assert len(twice) >= 3 and all(o["assigned"][f] == [m[1] for m in o["matches"] if m[0] == f][-1] for f in twice)
    nodes = {int(t): int(nd) for nd, a, b in zip(s["kf_fv"][0], s["kf_fv"][1][:-1], s["kf_fv"][1][1:]) for t in s["kf_fv"][2][a:b]}
    assert all(len({nodes[m[1]] for m in o["matches"] if m[0] == f}) == 1 for f in twice)     # both of one node
    s, o, _ = sc.shape(orc, "angles")
    raw = tr.search(s, o["bow"][2:], dict(tr.DEFAULTS, check_orientation=False))
    assert len(o["matches"]) <= 0.8 * len(raw)
    diff = s["kps"]["angle"][[m[0] for m in o["matches"]]] - s["kf_kps"]["angle"][[m[1] for m in o["matches"]]]
    bins = (np.where(diff < 0, np.float32(360) + diff, diff) / np.float32(12)).astype(int) % 30
    assert len(set(bins.tolist())) == 3 and 0 in bins
    s, o, _ = sc.shape(orc, "own")
    had = np.flatnonzero(s["frame_good"])
    assert len(had) == 100 and not np.isin([m[0] for m in o["matches"]], had).any() and (o["assigned"][had] == OWN).all()
    assert set(o["final_assigned"][had].tolist()) == {OWN, -1} and (o["final_assigned"][had] == -1).sum() >= 10
    assert np.isin(s["src"][s["good"] == 1], had).sum() >= 10                                 # keyframe features whose own feature is taken
    s, o, _ = sc.shape(orc, "mono")
    assert s["right_u"] is None and o["verdict"] == tr.ACCEPT
    s, o, _ = sc.shape(orc, "no_good")
    assert o["n_matches"] == 0 and o["verdict"] == tr.REJECT_MATCHES and (o["assigned"] == -1).all() and not o["pose_se3"].any()
    s, o, _ = sc.shape(orc, "root")
    assert len(o["bow"][2]) == 1 and len(s["kf_fv"][0]) == 1 and o["verdict"] == tr.ACCEPT
    s, o, kw = sc.shape(orc, "one")
    assert len(s["good"]) == 1 and kw == dict(min_matches=0) and o["n_matches"] == 1 and o["n_edges"] == 1 and o["verdict"] == tr.REJECT_INLIERS


# ---- surface ---------------------------------------------------------------------------------------------------------------------------
_LAYOUT = r"""
#include <cstddef>
#include <cstdio>
#include "orbfe.h"
#define F(T, m) std::printf(#m " %zu\n", offsetof(T, m));
int main() {
  F(orbfe_trackref_input, kf_id) F(orbfe_trackref_input, n) F(orbfe_trackref_input, good) F(orbfe_trackref_input, pos)
  F(orbfe_trackref_input, frame_good) F(orbfe_trackref_input, frame_pos) F(orbfe_trackref_input, right_u) F(orbfe_trackref_input, Rcw)
  F(orbfe_trackref_input, tcw) F(orbfe_trackref_input, bounds) F(orbfe_trackref_input, level_sigma2) F(orbfe_trackref_input, level_inv_sigma2)
  F(orbfe_trackref_input, cam) F(orbfe_trackref_input, levelsup) F(orbfe_trackref_input, ratio) F(orbfe_trackref_input, dist_threshold)
  F(orbfe_trackref_input, check_orientation) F(orbfe_trackref_input, min_matches) F(orbfe_trackref_input, min_inliers)
  F(orbfe_trackref_input, n_nodes) F(orbfe_trackref_input, nodes) F(orbfe_trackref_input, node_offsets) F(orbfe_trackref_input, features)
  std::printf("sizeof_in %zu\nsizeof_out %zu\nown %d\n", sizeof(orbfe_trackref_input), sizeof(orbfe_trackref_output), ORBFE_TRACKREF_OWN);
  F(orbfe_trackref_output, verdict) F(orbfe_trackref_output, n_matches) F(orbfe_trackref_output, matches) F(orbfe_trackref_output, assigned)
  F(orbfe_trackref_output, n_edges) F(orbfe_trackref_output, n_inliers) F(orbfe_trackref_output, inlier) F(orbfe_trackref_output, final_assigned)
  F(orbfe_trackref_output, pose_se3) F(orbfe_trackref_output, Tcw) F(orbfe_trackref_output, bow)
}
"""


def test_header_declares_and_library_exports_the_entry_point():
    from orb_slam2_ros2_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)                       # loading must not need a GPU
    assert re.search(r"\borbfe_status\s+orbfe_track_reference_stored\s*\(", hdr)
    assert hasattr(lib, "orbfe_track_reference_stored") and "orbfe_track_reference_stored" in _lib.EXPORTS
    for typ in ("orbfe_trackref_input", "orbfe_trackref_output", "orbfe_trackref_verdict"):
        assert re.search(r"\}\s*" + typ + r"\s*;", hdr), typ
    for name, val in tr.VERDICT_NAMES.items():
        assert re.search(r"ORBFE_TRACKREF_" + val + r"\s*=\s*" + str(name) + r"\b", hdr) and _lib.TRACKREF_VERDICTS[name] == val
    assert "#define ORBFE_ABI_VERSION 4" in hdr and lib.orbfe_abi_version() == 4
    assert callable(_lib.Context.track_reference_stored) and _lib.TRACKREF_OWN == OWN
    # the header's comment cites what it restates and lists the rules
    block = hdr[hdr.index("trackReference over a stored keyframe"):hdr.index("orbfe_trackref_verdict")]
    for cite in ("src/Tracking.cc:360-371", "src/ORBMatcher.cc:170-253, 815-830, 1013-1051", "src/Optimizer.cc:33-203", "Frame.h:224-229"):
        assert cite in block, cite
    for k in range(1, 9):
        assert f"T{k} " in block


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_binding_has_the_c_layout_of_the_two_records(tmp_path):
    from orb_slam2_ros2_amd import _lib
    src, exe = str(tmp_path / "layout.cpp"), str(tmp_path / "layout")
    open(src, "w").write(_LAYOUT)
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, src], timeout=300)
    rows = dict(r.split() for r in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.strip().split("\n"))
    ti, to = _lib.TrackRefInput, _lib.TrackRefOutput
    assert int(rows.pop("sizeof_in")) == ctypes.sizeof(ti) and int(rows.pop("sizeof_out")) == ctypes.sizeof(to) and int(rows.pop("own")) == OWN
    names_in, names_out = [k for k, _ in ti._fields_], [k for k, _ in to._fields_]
    assert list(rows) == names_in + names_out               # the same fields in the same order
    for k in names_in:
        assert getattr(ti, k).offset == int(rows[k]), k
    for k in names_out:
        assert getattr(to, k).offset == int(rows[k]), k


def test_nm_exports_equal_the_headers_declarations():
    if shutil.which("nm") is None:
        pytest.skip("needs nm")
    from orb_slam2_ros2_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    declared = set(re.findall(r"\b(orbfe_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, timeout=60).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T orbfe_" in ln}
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    assert "orbfe_track_reference_stored" in exported


from test_reference_compile import REF  # noqa: E402


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "ORB_SLAM2")) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++")
def test_dropin_compiles_against_the_reference_headers(tmp_path):
    """g++ -fsyntax-only of tests/cpp/ref_trackref_body.cpp: orbfe::dropin::trackReference as the whole body of Tracking::trackReference, with
    the reference's Tracking.h / KeyFrame.h / Frame.h / MapPoint.h (symlinks; Frame.h / KeyFrame.h as temporary copies with INTEGRATION
    section 3's friend line) and host/compat's DBoW3.h in DBoW3's place"""
    from test_reference_compile import _include_dir
    inc = _include_dir(str(tmp_path / "inc"), friend_line=True)
    stubs = os.path.join(ROOT, "tests", "cpp", "stubs")
    host = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(host, "compat"), "-I" + inc, "-I" + stubs,
                        "-I" + os.path.join(stubs, "refgen"), "-I" + os.path.join(ROOT, "include"), "-I" + host,
                        os.path.join(ROOT, "tests", "cpp", "ref_trackref_body.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_dropin_body_over_stand_ins_with_a_stub_for_the_device_call(tmp_path):
    """tests/cpp/test_trackref_gather.cpp: Bodies::trackReference runs over stand-in classes up to the device call, which the program
    defines itself; the gathered arrays bit for bit, the replayed side effects for each verdict, the host-FeatureVector form, and every
    fallback condition"""
    pkg = os.path.join(ROOT, "orb_slam2_ros2_amd")
    exe = str(tmp_path / "test_trackref_gather")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_trackref_gather.cpp"), "-L" + pkg, "-lorbfe_hip", "-pthread",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "GATHER_OK", r.stdout + r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_dropin_program_builds_on_the_stand_in_classes(tmp_path):
    """tests/cpp/test_trackref_dropin.cpp (run by tests/test_gpu_track_reference.py) compiles and links without a device"""
    pkg = os.path.join(ROOT, "orb_slam2_ros2_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), "-o",
                           str(tmp_path / "test_trackref_dropin"), os.path.join(ROOT, "tests", "cpp", "test_trackref_dropin.cpp"), "-L" + pkg,
                           "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=600)
