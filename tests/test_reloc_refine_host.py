"""The relocalisation refine (orbfe_reloc_refine_stored) without a device: the restatement of reloc_refine_restatement.py
reaches every verdict on the scenes of reloc_refine_scenes.py with margins that make the verdicts robust, the boundary scenes sit where
they claim, the numpy pose conversions are host/map_pb.hpp's bit for bit (through a small C++ program), and the surface: header, export,
binding, ABI version."""
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
import reloc_refine_scenes as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
result = sc.restated


def _conditions(s, o):
    """what makes a scene's verdict independent of the last bit: no post-checked projection within 1e-3 px of a bound, tlc.z not within
    1e-3 of the baseline"""
    for st in range(2):
        if o["checked"][st] is None:
            continue
        u, v, z = o["checked"][st]
        d = np.concatenate([np.abs(u), np.abs(u - np.float32(s["bounds"][1])), np.abs(v), np.abs(v - np.float32(s["bounds"][3])), np.abs(z)])
        assert d.size == 0 or d.min() > 1e-3, (st, d.min())
    for st in range(2):
        if o["n_added"][st] or o["excluded_hits"][st].any():
            assert abs(abs(float(o["tlc_z"][st])) - s["baseline"]) > 1e-3


@pytest.mark.parametrize("name", list(sc.VERDICT_SCENES))
def test_the_restatement_reaches_every_verdict_with_margins(orc, name):
    s, o = result(orc, name)
    assert o["verdict_name"] == name, (o["verdict_name"], o["n_inliers"], o["n_added"])
    # every count a decision reads is at least 3 away from 10 and 50
    read = [int(o["n_inliers"][0])]
    if name not in ("REJECT_1", "ACCEPT_1"):
        read.append(int(o["n_inliers"][0] + o["n_added"][0]))
    if name in ("ACCEPT_2", "REJECT_3", "ACCEPT_3"):
        read.append(int(o["n_inliers"][1]))
    if name in ("REJECT_3", "ACCEPT_3"):
        read.append(int(o["n_inliers"][1] + o["n_added"][1]))
    for c in read:
        assert abs(c - 10) >= 3 and abs(c - 50) >= 3, (name, read)
    _conditions(s, o)
    # the three bad seeds never became edges; a stage that did not run left nothing
    assert o["n_edges"][0] == sc.VERDICT_SCENES[name]["n_seed"]
    if name in ("REJECT_1", "ACCEPT_1"):
        assert o["n_edges"][1] == 0 and not o["n_added"].any() and (o["assigned"] == -1).all() and not o["Tcw"][1].any()
    if name in ("ACCEPT_2",):
        # some features were picked by two queries (the later one stays), queries met features that hold a point, every window mode
        # but this scene's is covered by the others
        picked = o["query_accepted"][0].sum()
        assert picked > (o["assigned"][0] >= 0).sum() - o["n_inliers"][0] and o["excluded_hits"][0].sum() > 50
    if name in ("REJECT_3", "ACCEPT_3"):
        assert o["n_edges"][1] > o["n_inliers"][1] + 5            # the second optimisation threw the bad points out again


def test_the_scenes_cover_every_window_mode(orc):
    modes = {}
    for name in ("REJECT_2", "REJECT_3", "ACCEPT_3"):
        s, o = result(orc, name)
        modes[s["mode"]] = float(o["tlc_z"][0])
    assert modes["up"] > sc.BASELINE and modes["down"] < -sc.BASELINE and abs(modes["same"]) < sc.BASELINE


def test_far_queries_are_found_by_the_first_search_only(orc):
    s, o = result(orc, "REJECT_3")
    assert o["n_added"][0] >= 20 and o["n_added"][1] <= 3


def test_zero_edges_is_reject_1(orc):
    s = sc.build(orc, n_seed=0)
    s["held"][:] = -1
    o = rr.refine(orc, s)
    assert o["verdict"] == rr.REJECT_1 and o["n_edges"][0] == 0 and o["n_inliers"][0] == 0
    assert np.array_equal(o["pose_se3"][0], rr.tcw_to_se3(s["Rcw"], s["tcw"]))


@pytest.mark.parametrize("n_seed", list(sc.BOUNDARY_SCENES))
def test_boundary_scenes(orc, n_seed):
    """noise-free points: every seed edge is an inlier with chi2 ~ 0, so 9 / 10 / 49 / 50 seeds are 9 / 10 / 49 / 50 inliers"""
    s, o = result(orc, n_seed)
    assert o["n_edges"][0] == n_seed and o["n_inliers"][0] == n_seed
    assert o["verdict_name"] == sc.BOUNDARY_SCENES[n_seed]
    searched = o["verdict"] not in (rr.REJECT_1, rr.ACCEPT_1)
    assert searched == (n_seed in (10, 49))
    # no edge near a threshold: the reprojection error at the optimum is far below a pixel
    R, t = o["Tcw"][0][:9], o["Tcw"][0][9:]
    f = np.flatnonzero(o["inlier"][0])
    u, v, _ = rr.project(R, t, s["pos"][s["held"][f]], s["cam"])
    assert np.abs(u - s["kps"]["x"][f]).max() < 0.05 and np.abs(v - s["kps"]["y"][f]).max() < 0.05
    _conditions(s, o)


# ---- the pose conversions against host/map_pb.hpp ---------------------------------------------------------------------------------------
_CPP = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "map_pb.hpp"
int main() {
  uint32_t w[12];
  for (;;) {
    for (int k = 0; k < 12; ++k)
      if (std::scanf("%" SCNx32, &w[k]) != 1) return 0;
    float R[9], t[3], R2[9], t2[3];
    std::memcpy(R, w, 36), std::memcpy(t, w + 9, 12);
    double p[7];
    orbfe::mappb::tcw_to_se3(R, t, p);
    orbfe::mappb::se3_to_tcw(p, R2, t2);
    for (int k = 0; k < 7; ++k) { uint64_t b; std::memcpy(&b, &p[k], 8); std::printf("%016" PRIx64 " ", b); }
    for (int k = 0; k < 9; ++k) { uint32_t b; std::memcpy(&b, &R2[k], 4); std::printf("%08" PRIx32 " ", b); }
    for (int k = 0; k < 3; ++k) { uint32_t b; std::memcpy(&b, &t2[k], 4); std::printf("%08" PRIx32 " ", b); }
    std::printf("\n");
  }
}
"""


def _rotations():
    rng = np.random.default_rng(7)
    out = []
    for _ in range(40):                                   # the trace branch
        q = rng.normal(size=4); q[3] = abs(q[3]) + 1.0; q /= np.linalg.norm(q)
        out.append(sc.quat_to_R(q))
    for axis in range(3):                                 # half turns and near half turns: each largest-diagonal branch
        for _ in range(15):
            q = rng.normal(0, 0.05, 4); q[axis] = 1.0; q /= np.linalg.norm(q)
            out.append(sc.quat_to_R(q))
    for _ in range(20):                                   # anything, w of either sign
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        out.append(sc.quat_to_R(q))
    return [(R.astype(np.float32).reshape(9), rng.uniform(-30, 30, 3).astype(np.float32)) for R in out]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pose_conversions_are_map_pb_hpp_bit_for_bit(tmp_path):
    src, exe = str(tmp_path / "conv.cpp"), str(tmp_path / "conv")
    open(src, "w").write(_CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "orb_slam2_ros2_amd", "host"), "-o", exe, src],
                          timeout=300)
    cases = _rotations()
    text = "\n".join(" ".join(f"{int(w):08x}" for w in np.concatenate([R, t]).view(np.uint32)) for R, t in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    rows = r.stdout.strip().split("\n")
    assert len(rows) == len(cases)
    branches = set()
    for (R, t), row in zip(cases, rows):
        w = row.split()
        p_ref = np.array([int(x, 16) for x in w[:7]], np.uint64).view(np.float64)
        T_ref = np.array([int(x, 16) for x in w[7:]], np.uint32)
        p = rr.tcw_to_se3(R, t)
        assert np.array_equal(p.view(np.uint64), p_ref.view(np.uint64)), (R, p, p_ref)
        R2, t2 = rr.se3_to_tcw(p)
        assert np.array_equal(np.concatenate([R2, t2]).view(np.uint32), T_ref)
        m = R.reshape(3, 3).astype(np.float64)
        branches.add("trace" if m.trace() > 0 else int(np.argmax(np.diag(m))))
    assert branches == {"trace", 0, 1, 2}


# ---- surface --------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    from orb_slam2_ros2_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)                       # loading must not need a GPU
    assert re.search(r"\borbfe_status\s+orbfe_reloc_refine_stored\s*\(", hdr)
    assert hasattr(lib, "orbfe_reloc_refine_stored") and "orbfe_reloc_refine_stored" in _lib.EXPORTS
    for typ in ("orbfe_reloc_input", "orbfe_reloc_output", "orbfe_reloc_verdict"):
        assert re.search(r"\}\s*" + typ + r"\s*;", hdr), typ
    for name, val in rr.VERDICT_NAMES.items():
        assert re.search(r"ORBFE_RELOC_" + val + r"\s*=\s*" + str(name) + r"\b", hdr) and _lib.RELOC_VERDICTS[name] == val
    assert "#define ORBFE_ABI_VERSION 4" in hdr and lib.orbfe_abi_version() == 4
    assert callable(_lib.Context.reloc_refine_stored)
    # the C layout (x86-64 / LP64) of the two records
    ri, ro = _lib.RelocInput, _lib.RelocOutput
    assert ri.good.offset == 16 and ri.kf_Rcw.offset == 32 and ri.held.offset == 80 and ri.Rcw.offset == 96 and ri.bounds.offset == 144
    assert ri.level_sigma2.offset == 160 and ri.cam.offset == 176 and ri.baseline.offset == 184 and ctypes.sizeof(ri) == 216
    assert ctypes.sizeof(ro) == 12 * 8


REF = "/root/reference/src/ORB_SLAM2"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "ORB_SLAM2")) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++")
def test_dropin_compiles_against_the_reference_headers(tmp_path):
    """g++ -fsyntax-only of tests/cpp/ref_reloc_refine_body.cpp: orbfe::dropin::relocRefine with the reference's Tracking.h / KeyFrame.h /
    Frame.h / MapPoint.h / PnPSolver.h (symlinks; Frame.h / KeyFrame.h as temporary copies with INTEGRATION section 3's friend line)"""
    from test_reference_compile import _include_dir
    inc = _include_dir(str(tmp_path / "inc"), friend_line=True)
    stubs = os.path.join(ROOT, "tests", "cpp", "stubs")
    host = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + inc, "-I" + stubs, "-I" + os.path.join(stubs, "refgen"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "cpp", "ref_reloc_refine_body.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
