"""trackMotionModel over two frame slots (orbfe_track_motion_model_slots) without a device: the restatement of
track_motion_restatement.py on a dozen hand-made features with answers worked out by hand, the scene builders' claims (every verdict, the
directions, the second search, the boundary counts with their chi-square margins), and the surface -- header, export, binding, ABI
version, the C layout of the two records."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reloc_refine_restatement as rr  # noqa: E402
import track_motion_restatement as tm  # noqa: E402
import track_motion_scenes as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = sc.GEOM["kitti"]
FX, FY, CX, CY = G["cam"][:4]


# ---- a dozen features, by hand ---------------------------------------------------------------------------------------------------------
def hand_scene():
    """Twelve frame features with unrelated random descriptors R_f in two rows, 192 pixels (three grid cells) apart, so that no search
    box of th <= 30 reaches a neighbour; every pose is the identity, every octave 0; the point of feature f lies at depth 8 + f % 4 on
    its pixel's ray.  Twelve last-frame features, each at the pixel of a frame feature:
      0, 1     both copy R_3 with in-map points: two queries name frame feature 3, the later one keeps it
      2        copies R_5, holds nothing, depth 9: a temporary point on the ray of feature 5
      3        copies R_7, its point is bad, no depth: no query
      4        copies R_8 with a point that is not in the map
      5        copies R_9 with an in-map point four metres off
      6 .. 9   copy R_0, R_1, R_2, R_4 with exact in-map points
      10       copies R_6, holds nothing, no depth: no query
      11       an in-map point at the pixel of feature 10 with a descriptor that matches nothing"""
    from orb_slam2_ros2_amd._lib import KP_DTYPE
    rng = np.random.default_rng(31)
    R = rng.integers(0, 256, (13, 32), dtype=np.uint8)
    kps = np.zeros(12, KP_DTYPE)
    f = np.arange(12)
    kps["x"], kps["y"] = 100 + 192 * (f % 6), np.where(f < 6, 60, 300)
    kps["size"], kps["class_id"] = 31.0, -1
    z = 8.0 + f % 4
    X = np.stack([(kps["x"] - CX) / FX * z, (kps["y"] - CY) / FY * z, z], 1).astype(np.float32)
    src = np.array([3, 3, 5, 7, 8, 9, 0, 1, 2, 4, 6, 10])
    l_desc = R[src].copy()
    l_desc[11] = R[12]
    flags = np.array([3, 3, 0, 0, 1, 3, 3, 3, 3, 3, 0, 3], np.uint8)
    pos = X[src].copy()
    pos[5] += np.float32(4.0)
    pos[[2, 3, 10]] = np.float32(1e6)                       # not read
    depth = np.full(12, -1.0)
    depth[2] = 9.0
    eye, zero = np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32)
    return dict(nf=12, n_kp=12, kps=kps, desc=R[:12], right_u=None, l_kps=kps[src].copy(), l_desc=l_desc, l_n=12, l_depth=depth, last_flags=flags,
                last_pos=pos, Rcw=eye, tcw=zero, last_Rcw=eye, last_tcw=zero, last_Rwc=eye, last_twc=zero, cam=G["cam"], bounds=(0.0, 1241.0, 0.0, 376.0),
                baseline=sc.BASELINE, sigma2=sc.SIGMA2, inv_sigma2=sc.INV_SIGMA2), X


def test_the_restatement_on_a_scene_worked_out_by_hand(orc):
    s, X = hand_scene()
    want_assigned = [6, 7, 8, 1, 9, 2, -1, -1, 4, 5, -1, -1]
    want_qm = [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 0, 0]
    # M1: one temporary point, on the ray of frame feature 5 at depth 9, computed as the reference computes it
    temp, tpos = tm.unproject(s)
    assert temp.tolist() == [0, 0, 1] + [0] * 9
    x, y = (np.float32(100 + 192 * 5) - np.float32(CX)) / np.float32(FX), (np.float32(60) - np.float32(CY)) / np.float32(FY)
    by_hand = np.array([np.float32(9.0 * np.float64(x)), np.float32(9.0 * np.float64(y)), np.float32(9.0)], np.float32)
    assert np.array_equal(tpos[2], by_hand) and not tpos[[0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11]].any()
    # M2, M3: ten queries in feature order, no motion: the window is the octave +- 1
    q = tm.queries(s, temp, tpos)
    assert q["who"].tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9, 11] and q["z"] == 0 and set(q["lo"].tolist()) == {0} and set(q["hi"].tolist()) == {1}
    assert np.array_equal(q["pos"][2], by_hand) and np.array_equal(q["pos"][0], s["last_pos"][0]) and not q["pos"][[3, 10]].any()
    # nine matches are too few for 20: the second search runs, meets every feature it assigned -- feature 3 twice -- and adds nothing;
    # both frames are written all the same
    o = tm.track(orc, s)
    assert o["verdict_name"] == "REJECT_MATCHES" and o["passes"] == 2 and o["n_matches"] == 9
    assert o["assigned"].tolist() == want_assigned and o["final_assigned"].tolist() == want_assigned and o["query_matches"].tolist() == want_qm
    assert o["excluded_hits"].tolist() == [1, 1, 1, 2, 1, 1, 0, 0, 1, 1, 0, 0]
    assert o["n_edges"] == 0 and o["n_inliers"] == 0 and o["n_in_map"] == 0 and not o["inlier"].any() and not o["pose_se3"].any() and not o["Tcw"].any()
    # with a minimum of nine: one search, no excluded candidate; eight edges in feature order; the point four metres off is thrown out;
    # of the seven inliers the temporary point (feature 5) and the local one (feature 8) are not in the map
    o = tm.track(orc, s, min_matches=9, min_inliers=5)
    assert o["passes"] == 1 and o["n_matches"] == 9 and not o["excluded_hits"].any() and o["assigned"].tolist() == want_assigned
    assert o["n_edges"] == 8 and o["edge_inlier"][0].tolist() == [0, 1, 2, 3, 4, 5, 8, 9]
    assert np.flatnonzero(o["inlier"]).tolist() == [0, 1, 2, 3, 4, 5, 8] and o["n_inliers"] == 7
    assert o["final_assigned"].tolist() == [6, 7, 8, 1, 9, 2, -1, -1, 4, -1, -1, -1]
    assert o["n_in_map"] == 5 and o["verdict_name"] == "ACCEPT" and np.abs(o["pose_se3"] - [0, 0, 0, 1, 0, 0, 0]).max() < 1e-6
    R, t = rr.se3_to_tcw(o["pose_se3"])
    assert np.array_equal(o["Tcw"], np.concatenate([R, t]))
    o = tm.track(orc, s, min_matches=9, min_inliers=6)
    assert o["verdict_name"] == "REJECT_INLIERS" and o["n_inliers"] == 7 and o["n_in_map"] == 5
    # no second search when th_second is not positive
    o = tm.track(orc, s, th_second=0.0)
    assert o["passes"] == 1 and o["verdict_name"] == "REJECT_MATCHES" and not o["excluded_hits"].any()
    # without depth there is no temporary point: feature 5 stays empty
    o = tm.track(orc, dict(s, l_depth=None), min_matches=8, min_inliers=5)
    assert not o["temp"].any() and o["n_matches"] == 8 and o["assigned"][5] == -1 and o["n_in_map"] == 5


# ---- the scenes -------------------------------------------------------------------------------------------------------------------------
def test_the_two_frames_really_move(orc):
    last, cur = sc.frames(orc, "kitti")
    assert sc.SHIFT == (2, 1) and not np.array_equal(last["lk"], cur["lk"])
    # most level-0 features of the last frame reappear (2, 1) pixels further left / up
    l0, c0 = last["lk"][last["lk"]["octave"] == 0], cur["lk"][cur["lk"]["octave"] == 0]
    moved = {(float(x) - 2, float(y) - 1) for x, y in zip(l0["x"], l0["y"])}
    again = sum((float(x), float(y)) in moved for x, y in zip(c0["x"], c0["y"]))
    assert again > 0.5 * len(l0)


@pytest.mark.parametrize("name", sc.SCENES)
def test_every_scene_is_what_it_claims(orc, name):
    s, o, kw = sc.scene(orc, name)
    want = dict(forward="ACCEPT", backward="ACCEPT", neither="ACCEPT", second="ACCEPT", few="REJECT_MATCHES", temp_inliers="REJECT_INLIERS",
                mono="ACCEPT", zero="REJECT_MATCHES", one="ACCEPT", all_temp="REJECT_INLIERS")[name]
    assert o["verdict_name"] == want
    q, oc = o["q"], o["q"]["octave"]
    if name == "forward":
        assert q["z"] > sc.BASELINE and np.array_equal(q["lo"], oc) and (q["hi"] == 7).all()
    if name == "backward":
        assert q["z"] < -sc.BASELINE and (q["lo"] == 0).all() and np.array_equal(q["hi"], oc)
    if name == "neither":
        assert abs(q["z"]) < sc.BASELINE and np.array_equal(q["lo"], np.maximum(oc - 1, 0)) and np.array_equal(q["hi"], np.minimum(oc + 1, 7))
    if name in ("forward", "backward", "neither"):
        # points of their own, temporaries, points metres off that the optimisation throws out, bad points that became temporaries
        assert o["passes"] == 1 and o["temp"].sum() > 100 and o["n_edges"] - o["n_inliers"] >= 20 and o["n_in_map"] > 100
        bad = np.flatnonzero((s["last_pos"] == np.float32(1e6)).all(1))
        assert len(bad) > 20 and (o["temp"][bad] == (s["l_depth"][bad] >= 0)).all() and o["temp"][bad].any()
    if name == "second":
        r1 = tm.search(orc, s, q, np.full(s["nf"], -1, np.int32), kw["th"], tm.DEFAULTS)
        assert r1["n_added"] == 12 and o["passes"] == 2 and o["n_matches"] >= 40 and o["excluded_hits"].sum() >= 12
        assert (o["assigned"][r1["assigned"] >= 0] == r1["assigned"][r1["assigned"] >= 0]).all()      # the matches of the first search stay
    if name == "few":
        assert o["passes"] == 2 and o["n_matches"] < 20 and (o["assigned"] >= 0).sum() >= 8 and np.array_equal(o["assigned"], o["final_assigned"])
        assert o["n_edges"] == 0 and not o["pose_se3"].any()
    if name == "temp_inliers":
        assert o["n_inliers"] > 100 and o["n_in_map"] < 10 and o["temp"].sum() > 100
    if name == "mono":
        assert s["right_u"] is None and s["pair"] == -1 and o["temp"].sum() > 50
    if name == "zero":
        assert len(q["who"]) == 0 and o["n_matches"] == 0 and o["passes"] == 2 and (o["assigned"] == -1).all()
    if name == "one":
        assert len(q["who"]) == 1 and o["n_matches"] == 1 and o["n_edges"] == 1
    if name == "all_temp":
        assert not s["last_flags"].any() and np.array_equal(np.flatnonzero(o["temp"]), q["who"]) and o["n_in_map"] == 0 and o["n_inliers"] > 100
    assert sc.margins(orc, s, o) > 0.01


@pytest.mark.parametrize("name", list(sc.BOUNDARY))
def test_boundary_scenes(orc, name):
    """the builder has asserted the count and the 1 % chi-square margin; both once more, the verdict, and that the query count is exact"""
    s, o, _ = sc.scene(orc, name)
    kind, want = name.rsplit("_", 1)
    assert (o["n_matches"] if kind == "matches" else o["n_in_map"]) == int(want) and o["verdict_name"] == sc.BOUNDARY[name]
    assert s["last_pair"] == -1 and not o["temp"].any() and len(o["q"]["who"]) == int((s["last_flags"] & 1).sum())
    assert o["passes"] == (2 if name == "matches_19" else 1)
    assert sc.margins(orc, s, o) > 0.01
    if o["n_edges"]:            # no post-checked projection near a bound
        ef, inl = o["edge_inlier"]
        c = tm.post_check(s, o["q"], o["assigned"], ef, inl, o["pose_se3"])
        d = np.concatenate([np.abs(c["u"]), np.abs(c["u"] - np.float32(G["W"])), np.abs(c["v"]), np.abs(c["v"] - np.float32(G["H"])), np.abs(c["z"])])
        assert d.min() > 1e-3


def test_the_small_geometry(orc):
    s, o, _ = sc.scene(orc, "small")
    assert s["nf"] == 500 and s["n_kp"] <= 500 and o["verdict_name"] == "ACCEPT" and o["temp"].sum() > 10


# ---- surface ---------------------------------------------------------------------------------------------------------------------------
_IN = ("last_flags", "last_ids", "last_pos", "Rcw", "tcw", "last_Rcw", "last_tcw", "last_Rwc", "last_twc", "bounds", "cam", "baseline", "level_sigma2",
       "level_inv_sigma2", "th", "th_second", "ratio", "min_threshold", "min_matches", "min_inliers")
_OUT = ("verdict", "passes", "n_matches", "n_edges", "n_inliers", "n_in_map", "assigned", "final_assigned", "inlier", "excluded_hits", "query_matches",
        "temp", "temp_pos", "pose_se3", "Tcw")
_LAYOUT = ("#include <cstddef>\n#include <cstdio>\n#include \"orbfe.h\"\n#define F(T, m) std::printf(#m \" %zu\\n\", offsetof(T, m));\nint main() {\n"
           + "".join(f"  F(orbfe_motion_slots_input, {m})\n" for m in _IN)
           + "  std::printf(\"sizeof_in %zu\\nsizeof_out %zu\\n\", sizeof(orbfe_motion_slots_input), sizeof(orbfe_motion_slots_output));\n"
           + "".join(f"  F(orbfe_motion_slots_output, {m})\n" for m in _OUT) + "}\n")


def test_header_declares_and_library_exports_the_entry_point():
    from orb_slam2_ros2_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)                       # loading must not need a GPU
    assert re.search(r"\borbfe_status\s+orbfe_track_motion_model_slots\s*\(", hdr)
    assert hasattr(lib, "orbfe_track_motion_model_slots") and "orbfe_track_motion_model_slots" in _lib.EXPORTS
    for typ in ("orbfe_motion_slots_input", "orbfe_motion_slots_output", "orbfe_motion_verdict"):
        assert re.search(r"\}\s*" + typ + r"\s*;", hdr), typ
    for name, val in tm.VERDICT_NAMES.items():
        assert re.search(r"ORBFE_MOTION_" + val + r"\s*=\s*" + str(name) + r"\b", hdr) and _lib.MOTION_VERDICTS[name] == val
    assert "#define ORBFE_ABI_VERSION 4" in hdr and lib.orbfe_abi_version() == 4
    assert callable(_lib.Context.track_motion_model_slots)
    # the header's comment cites what it restates and lists the rules
    block = hdr[hdr.index("trackMotionModel over two frame slots"):hdr.index("orbfe_motion_verdict")]
    for cite in ("src/Tracking.cc:381-406", "src/Frame.cc:179-202", "src/ORBMatcher.cc:265-347, 815-830", "src/Optimizer.cc:33-203"):
        assert cite in block, cite
    for k in range(1, 11):
        assert f"M{k} " in block


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_binding_has_the_c_layout_of_the_two_records(tmp_path):
    from orb_slam2_ros2_amd import _lib
    src, exe = str(tmp_path / "layout.cpp"), str(tmp_path / "layout")
    open(src, "w").write(_LAYOUT)
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, src], timeout=300)
    rows = dict(r.split() for r in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.strip().split("\n"))
    ti, to = _lib.MotionSlotsInput, _lib.MotionSlotsOutput
    assert int(rows.pop("sizeof_in")) == ctypes.sizeof(ti) and int(rows.pop("sizeof_out")) == ctypes.sizeof(to)
    names_in, names_out = [k for k, _ in ti._fields_], [k for k, _ in to._fields_]
    assert list(rows) == names_in + names_out == list(_IN + _OUT)              # the same fields in the same order
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
    assert "orbfe_track_motion_model_slots" in exported


from test_reference_compile import REF  # noqa: E402


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "ORB_SLAM2")) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++")
def test_dropin_compiles_against_the_reference_headers(tmp_path):
    """g++ -fsyntax-only of tests/cpp/ref_motion_body.cpp: orbfe::dropin::trackMotionModel as the body of Tracking::trackMotionModel after
    its two setPose calls, with the reference's Tracking.h / Frame.h / MapPoint.h (symlinks; Frame.h / KeyFrame.h as temporary copies with
    INTEGRATION section 3's friend line)"""
    from test_reference_compile import _include_dir
    inc = _include_dir(str(tmp_path / "inc"), friend_line=True)
    stubs = os.path.join(ROOT, "tests", "cpp", "stubs")
    host = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(host, "compat"), "-I" + inc, "-I" + stubs,
                        "-I" + os.path.join(stubs, "refgen"), "-I" + os.path.join(ROOT, "include"), "-I" + host,
                        os.path.join(ROOT, "tests", "cpp", "ref_motion_body.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


def _build(tmp_path, name, opt):
    pkg = os.path.join(ROOT, "orb_slam2_ros2_amd")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", opt, "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-L" + pkg, "-lorbfe_hip", "-pthread",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=600)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_dropin_body_over_stand_ins_with_a_stub_for_the_device_call(tmp_path):
    """tests/cpp/test_motion_gather.cpp: Bodies::trackMotionModelSlots runs over stand-in classes up to the device call, which the program
    defines itself; the gathered flags, ids and poses bit for bit, the replayed side effects for each verdict, every fallback condition"""
    r = subprocess.run([_build(tmp_path, "test_motion_gather", "-O1")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "MOTION_GATHER_OK", r.stdout + r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_dropin_program_builds_on_the_stand_in_classes(tmp_path):
    """tests/cpp/test_motion_dropin.cpp (run by tests/test_gpu_track_motion.py) compiles and links without a device"""
    _build(tmp_path, "test_motion_dropin", "-O0")
