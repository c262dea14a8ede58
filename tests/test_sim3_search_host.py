"""searchBySim3 over stored keyframes without a device: the restatement the GPU tests compare with equals the existing host
logic (MatcherExt.searchBySim3Frames / searchBySim3MapPoints with the oracle's search injected), the scenes really contain every case the
rules distinguish (a condition on the inputs, computed by the restatement alone), and the surface: header, exports, bindings, ctypes
mirrors, ABI version."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_search_restatement as rs  # noqa: E402
import sim3_search_scenes as sc  # noqa: E402
from orb_slam2_ros2_amd.frontend import ORBMatcher  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("s", [1.0, 0.5, 2.0])
def test_restatement_equals_the_matcher_on_the_seeded_scene(orc, s):
    """searchBySim3Frames knows one set of bounds: both keyframes get the image's here (the per-direction rule is pinned by the scenes
    below).  The two differ in one expression, the points overload's distance (cv::norm in double here, as host/orbfe_dropin.hpp has it):
    asserted not to matter on this scene."""
    S = sc.seeded(3, s, bounds_c=sc.IMAGE, bounds_m=sc.IMAGE)
    C, M = S["C"], S["M"]
    m = ORBMatcher(0.75)

    def inject(tag, *a):
        t = M if tag == "M" else C
        return orc.search_in_area_ex(t["kps"], t["desc"], sc.IMAGE, *a)[:4]
    got = m.searchBySim3Frames(None, S["matches"], S["Scm"], (C["Rcw"], C["tcw"]), (M["Rcw"], M["tcw"]), sc.frames_kf(C), sc.frames_kf(M), 7.5, sc.CAM,
                               sc.IMAGE, sc.SF, search_in=inject)
    w = rs.pair(orc, C, M, S["Scm"], S["matches"], sc.CAM, sc.SF, 7.5, 0.75)
    assert got == list(S["matches"]) + w["new"] and len(w["new"]) > 40
    loop = S["loop"]
    matched = np.full(len(C["kps"]), -1, np.int64)
    matched[[4, 8, 15]] = loop["id"][[1, 2, 3]]
    got, n = m.searchBySim3MapPoints(None, C, loop, matched, S["Scw"], 10.0, sc.CAM, sc.IMAGE, sc.SF,
                                     search_in=lambda *a: orc.search_in_area_ex(C["kps"], C["desc"], sc.IMAGE, *a)[:4])
    usable = loop["usable"] & ~np.isin(loop["id"], matched)
    bi = rs.points(orc, C, dict(loop, usable=usable), S["Scw"], sc.CAM, sc.SF, 10.0, 0.75)[0]
    assert got == [(int(bi[j]), int(j)) for j in np.flatnonzero(bi >= 0)] and n == 3 + len(got) and len(got) > 40


def test_the_scenes_cover_every_case(orc):
    """every rejection reason in both directions and for the points, at least 20 accepted per direction, the merge's collisions, the
    octave windows -1 .. 1 and 6 .. 8, the source-bounds rule"""
    seen = {"A": set(), "B": set(), "P": set()}
    accepted = {"A": 0, "B": 0, "P": 0}
    octaves = {"A": set(), "B": set(), "P": set()}
    held = shared = repeat = 0
    for S in [sc.seeded(1, s) for s in (1.0, 0.5, 2.0)] + [sc.hand()]:
        ratio = S.get("ratio", 0.75)
        w = rs.pair(orc, S["C"], S["M"], S["Scm"], S["matches"], sc.CAM, sc.SF, S["th"], ratio)
        p = rs.points(orc, S[S.get("loop_target", "C")], S["loop"], S["Scw"], sc.CAM, sc.SF, S["th"], ratio)
        for d, why, best, octs in (("A", w["reasons_a"], w["a"], w["oct_a"]), ("B", w["reasons_b"], w["b"], w["oct_b"]), ("P", p[2], p[0], p[3])):
            seen[d] |= set(why)
            octaves[d] |= set(int(o) for o in octs if o >= 0)
            if "notes" not in S:
                accepted[d] = max(accepted[d], int((best >= 0).sum()))
        keys_a = set(np.flatnonzero(w["a"] >= 0).tolist())
        keys_b = [int(k) for k in w["b"] if k >= 0]
        held += sum(k in keys_a for k in keys_b)                                        # a direction-B key that direction A already holds
        shared += len(keys_b) - len(set(keys_b))                                        # two direction-B sources with one key
        repeat += len({q for q, _ in w["new"]} & {q for q, _ in S["matches"]})           # a new key equal to an input match's queryIdx
    print(seen, accepted, octaves, held, shared, repeat)
    pair_reasons = {"source", "z", "u_max", "v_max", "u_min", "v_min", "d_max", "d_min", "no_candidate", "flags", "threshold", "ratio", "nan", "accepted"}
    assert seen["A"] == pair_reasons and seen["B"] == pair_reasons
    assert seen["P"] == (pair_reasons - {"flags"}) | {"view"}                           # (no flag filter on the target there)
    assert min(accepted.values()) >= 20
    assert held > 0 and shared > 0 and repeat > 0
    assert all({0, 7} <= o for o in octaves.values())


def test_the_hand_placed_cases_are_what_they_claim(orc):
    S = sc.hand()
    w = rs.pair(orc, S["C"], S["M"], S["Scm"], S["matches"], sc.CAM, sc.SF, S["th"], S["ratio"])
    for d in ("A", "B"):
        why, best, cand, n = w["reasons_" + d.lower()], w[d.lower()], w["cand_" + d.lower()], S["notes"][d]
        for name in ("z", "u_max", "u_min", "v_max", "v_min", "d_max", "d_min", "no_candidate", "flags", "threshold", "ratio", "nan"):
            assert why[n[name]] == name, (d, name, why[n[name]])
        assert why[n["no_candidate_octave"]] == "no_candidate" and why[n["threshold_plus_one"]] == "threshold"
        for name in ("threshold_equal", "ratio_equal", "record_order", "single", "octave0", "octave7"):      # both comparisons are <=
            assert why[n[name]] == "accepted", (d, name, why[n[name]])
        assert best[n["single"]] == n["single_target"] and cand[n["single"]] == 1 and cand[n["nan"]] == 2
        oc = w["oct_" + d.lower()]
        assert oc[n["octave0"]] == 0 and oc[n["octave7"]] == 7
    # isInImage asks the SOURCE keyframe: a point between the image and M's wide bounds
    assert w["reasons_b"][S["notes"]["B"]["between_bounds"]] == "accepted" and w["reasons_a"][S["notes"]["A"]["between_bounds"]] == "u_max"
    assert w["a"][S["notes"]["A"]["outside"]] == S["notes"]["A"]["outside_target"]      # a feature outside the image, in a border cell
    new = dict(w["new"])
    ic, im = S["notes"]["mutual"]
    assert w["a"][ic] == im and w["b"][im] == ic and new[ic] == im
    k, im1, im2 = S["notes"]["shared_key"]
    assert w["b"][im1] == k and w["b"][im2] == k and w["a"][k] < 0 and new[k] == im1 < im2      # first wins
    q0, t0, im3 = S["notes"]["repeat_query"]
    assert S["matches"] == [(q0, t0)] and w["b"][im3] == q0 and new[q0] == im3
    assert [q for q, _ in w["new"]] == sorted(new)
    # the points: a later point overwrites an earlier one
    bi, bd, why, octs, cand = rs.points(orc, S["M"], S["loop"], S["Scw"], sc.CAM, sc.SF, S["th"], S["ratio"])
    pn = S["point_notes"]
    for name in ("z", "u_max", "u_min", "v_max", "v_min", "d_max", "d_min", "view", "no_candidate", "threshold", "ratio", "nan"):
        assert why[pn[name]] == name, (name, why[pn[name]])
    assert why[pn["unusable"]] == "source" and bi[pn["accepted"]] == bi[pn["accepted_again"]] >= 0 and bd[pn["accepted"]] == 2 and bd[pn["accepted_again"]] == 1
    assert octs[pn["octave0"]] == 0 and octs[pn["octave7"]] == 7 and bi[pn["octave0"]] >= 0 and bi[pn["octave7"]] >= 0


@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 127, 128, 129])
def test_the_window_scenes_have_the_list_lengths_they_claim(orc, n_cand):
    S = sc.window(n_cand)
    w = rs.pair(orc, S["C"], S["M"], S["Scm"], [], sc.CAM, sc.SF, 7.5, 1.0)
    assert w["cand_a"][0] == n_cand and w["oct_a"][0] == 1
    cells = {(int(k["x"] // 64), int(k["y"] // 48)) for k in S["M"]["kps"]}
    assert len(cells) == 1                                                             # one cell: list order is index order


# ---- surface -------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from orb_slam2_ros2_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)                       # loading must not need a GPU
    for fn in ("orbfe_search_by_sim3_stored", "orbfe_search_by_sim3_points_stored"):
        assert re.search(r"\borbfe_status\s+" + fn + r"\s*\(", hdr) and hasattr(lib, fn) and fn in _lib.EXPORTS
    for typ in ("orbfe_sim3_side", "orbfe_sim3_points"):
        assert re.search(r"\}\s*" + typ + r"\s*;", hdr), typ
    assert "#define ORBFE_ABI_VERSION 4" in hdr and lib.orbfe_abi_version() == 4


def test_bindings_exist_and_mirror_the_structures():
    from orb_slam2_ros2_amd import _lib
    assert callable(_lib.Context.search_by_sim3_stored) and callable(_lib.Context.search_by_sim3_points_stored)
    assert callable(ORBMatcher.searchBySim3Stored) and callable(ORBMatcher.searchBySim3PointsStored)
    # the C layout (x86-64 / LP64): uint64 | int32 (+4) | 4 pointers | 12 floats; int32 (+4) | 6 pointers
    assert ctypes.sizeof(_lib.Sim3Side) == 8 + 8 + 32 + 48 and _lib.Sim3Side.flags.offset == 16 and _lib.Sim3Side.Rcw.offset == 48
    assert ctypes.sizeof(_lib.Sim3Points) == 8 + 48 and _lib.Sim3Points.usable.offset == 8 and _lib.Sim3Points.desc.offset == 48


REF = "/root/reference/src/ORB_SLAM2"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "ORB_SLAM2")) or __import__("shutil").which("g++") is None,
                    reason="needs the reference tree and g++")
def test_dropin_compiles_against_the_reference_headers(tmp_path):
    """g++ -fsyntax-only of tests/cpp/ref_sim3search_body.cpp: orbfe_reloc_dropin.hpp with the reference's ORBMatcher.h / KeyFrame.h /
    MapPoint.h / Sim3Solver.h (symlinks; Frame.h / KeyFrame.h as temporary copies with INTEGRATION section 3's friend line) and the two
    one-line bodies of INTEGRATION section 16"""
    import subprocess
    from test_reference_compile import _include_dir
    inc = _include_dir(str(tmp_path / "inc"), friend_line=True)
    stubs = os.path.join(ROOT, "tests", "cpp", "stubs")
    host = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + inc, "-I" + stubs, "-I" + os.path.join(stubs, "refgen"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "cpp", "ref_sim3search_body.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
