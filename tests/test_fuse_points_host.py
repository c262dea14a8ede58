"""The forward fuse over stored keyframes without a device: the restatement the GPU tests compare with equals the matcher's
own searchByProjectionMapPoints / fuseMapPoints keyframe by keyframe, the scenes contain what they are for, the replay of
MatcherExt.fusePointsIntoKeyframes on the one call's tables equals the plain sequential loop on the live map (and a stale entry gives
another map), the one-line bodies compile against the reference's class declarations, and the surface is there."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_points_restatement as fr  # noqa: E402
import fuse_points_scenes as sc  # noqa: E402
from orb_slam2_ros2_amd.frontend import ORBMatcher  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def tables(orc, S, th=None, ratio=sc.RATIO):
    return fr.tables(orc, S["kfs"], S["pts"], sc.CAM, S["sf"], th or S.get("th", sc.TH), ratio)


# ---- 1. the restatement is the matcher's ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["seeded8", "seeded4", "hand"])
def test_restatement_equals_the_matcher_keyframe_by_keyframe(orc, scene):
    S = {"seeded8": lambda: sc.seeded(1), "seeded4": lambda: sc.seeded(2, n_levels=4), "hand": sc.hand}[scene]()
    t = tables(orc, S)
    pts, sf, n_levels = S["pts"], S["sf"], len(S["sf"])
    m = ORBMatcher(sc.RATIO, True)
    total = 0
    for k, kf in enumerate(S["kfs"]):
        pr = orc.project_map_points(pts["pos"], pts["view_dir"], pts["max_dist"], pts["min_dist"], kf["Rcw"], kf["tcw"], sc.CAM, kf["bounds"])
        level = np.minimum(pr["level"].astype(np.int32), n_levels - 1)
        usable = pts["usable"].astype(bool) & pr["visible"].astype(bool)
        search = lambda *a, kf=kf: orc.search_in_area_ex(kf["kps"], kf["desc"], kf["bounds"], *a)[:4]  # noqa: E731
        got, n = m.searchByProjectionMapPoints(None, 0, pr["uv"], level, pr["cos_theta"], pts["desc"], usable, sc.TH, np.zeros(len(kf["kps"]), bool),
                                               True, n_levels=n_levels, scale_factors=sf, area_search=search)
        want = [(int(t["best_idx"][k][j]), int(j), int(t["best_dist"][k][j])) for j in np.flatnonzero(t["best_idx"][k] >= 0)]
        assert got == want and n == len(want)
        total += n
        if n_levels == 8:   # ORBMatcher::fuse on a keyframe without map points: every match is an "add"
            state = dict(good=np.zeros(len(kf["kps"]), bool), id=np.full(len(kf["kps"]), -1), obs=np.zeros(len(kf["kps"]), int))
            mps = dict(id=np.arange(len(usable)), good=np.ones(len(usable), bool), obs=np.ones(len(usable), int), usable=usable, uv=pr["uv"], level=level,
                       cos_theta=pr["cos_theta"], desc=pts["desc"])
            actions, nf = m.fuseMapPoints(None, kf, state, mps, th=sc.TH, bLoop=True, scale_factors=sf, search_in=search)
            assert actions == [("add", f, j) for f, j, _ in want] and nf == len(want)
    assert total >= 8


# ---- 2. the scenes contain what they are for -----------------------------------------------------------------------------------------------
def test_hand_scene_has_every_reason_both_radius_classes_and_levels_0_and_7(orc):
    S = sc.hand()
    t = tables(orc, S)
    why, n, f = t["reasons"][0], S["notes"], S["feats"]
    want = dict(unusable="unusable", behind="behind", distance_max="distance", distance_min="distance", outside_u_max="outside", outside_u_min="outside",
                outside_v_max="outside", outside_v_min="outside", angle="angle", angle_inside="accepted", empty="empty", empty_octave="empty",
                threshold="threshold", threshold_minus_one="accepted", ratio="ratio", ratio_inside="accepted", single="accepted", level0="accepted",
                level7="accepted", narrow="empty", wide="accepted", outside_image="accepted")
    for name, reason in want.items():
        assert why[n[name]] == reason, (name, why[n[name]])
    assert set(why) == set(fr.REASONS) | {"accepted"}
    for name in ("threshold_minus_one", "ratio_inside", "single", "level0", "level7", "wide", "outside_image"):
        assert t["best_idx"][0][n[name]] == f[name], name
    assert t["best_dist"][0][n["threshold_minus_one"]] == 49 and t["best_dist"][0][n["ratio_inside"]] == 7
    assert t["level"][0][n["level0"]] == 0 and t["level"][0][n["level7"]] == 7
    # cosTheta just on either side of 0.998f, and the radius it selects (level 0: the scale factor is 1)
    c_narrow, c_wide = t["cos_theta"][0][n["narrow"]], t["cos_theta"][0][n["wide"]]
    assert F32(0.998) < c_narrow < F32(0.99801) and F32(0.99799) < c_wide <= F32(0.998)
    assert t["radius"][0][n["narrow"]] == F32(10.0) and t["radius"][0][n["wide"]] == F32(16.0)


@pytest.mark.parametrize("n_levels", [8, 4])
def test_seeded_scene_is_not_vacuous(orc, n_levels):
    S = sc.seeded(1 if n_levels == 8 else 2, n_levels=n_levels)
    t = tables(orc, S)
    K, m = t["best_idx"].shape
    assert (K, m) == (4, 300) and all(len(kf["kps"]) == 300 for kf in S["kfs"])
    assert len({kf["bounds"] for kf in S["kfs"]}) == 4 and sc.IMAGE in {kf["bounds"] for kf in S["kfs"]}
    why = {r for row in t["reasons"] for r in row}
    assert why >= {"unusable", "distance", "outside", "angle", "empty", "accepted"}
    assert all((t["best_idx"][k] >= 0).sum() >= 10 for k in range(K))
    vis = t["level"] >= 0
    assert (vis.sum(0) == 1).sum() >= 10 and (vis.sum(0) == K).sum() >= 1 and (vis.sum(0) == 0).sum() >= 10    # visible in exactly one keyframe, ..
    assert set(np.unique(t["level"][vis])) == set(range(n_levels))
    base = t["radius"][vis] / (F32(sc.TH) * (S["sf"][t["level"][vis]] ** 2).astype(F32))
    assert (np.abs(base - 2.5) < 1e-5).sum() >= 10 and (np.abs(base - 4.0) < 1e-5).sum() >= 10              # both radius classes
    assert np.all(t["best_dist"][t["best_idx"] < 0] == 0)


@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 127, 128, 129])
def test_the_window_scenes_have_the_list_lengths_they_claim(orc, n_cand):
    S = sc.window(n_cand)
    t = tables(orc, S, ratio=1.5)                            # (the two best may tie: the ratio test is strict)
    assert t["cand"][0][0] == n_cand and t["level"][0][0] == 1 and t["best_idx"][0][0] >= 0
    assert len({(int(k["x"] // 64), int(k["y"] // 48)) for k in S["kfs"][0]["kps"]}) == 1        # one cell: list order is index order


# ---- 3. the replay -------------------------------------------------------------------------------------------------------------------------
def test_replay_equals_the_sequential_loop_and_a_stale_entry_does_not(orc):
    S = sc.loop_scene()
    a, b, c = S["model"].copy(), S["model"].copy(), S["model"].copy()
    for k, pid in S["held"]:
        assert pid in a.held(k)                                                  # a point held by the target from the start
    assert -1 in S["point_ids"] and any(a.is_bad(p) for p in S["point_ids"] if p >= 0) and any(not a.in_map(p) for p in S["point_ids"] if p >= 0)
    m = ORBMatcher(sc.RATIO, True)
    args = (S["target_kfs"], S["point_ids"], None, sc.CAM, sc.SF)
    n_fuse, stats = m.fusePointsIntoKeyframes(None, a, *args, th=sc.TH, search_in=sc.restated(orc, S))
    want = sc.sequential_loop(orc, S, b)
    assert n_fuse == want and all(n > 10 for n in want)
    assert a.state() == b.state()                                                # slots of every keyframe, observations, bad flags
    assert stats["device_entries"] > 0 and stats["reevaluated"] > 0 and stats["extra_calls"] == len(S["target_kfs"]) - 1
    # the replace in target 1 changed loop points that later targets match: both kinds occur
    near = [i for i in range(len(S["kind"])) if S["kind"][i] == "near"]
    far = [i for i in range(len(S["kind"])) if S["kind"][i] == "far"]
    before, after = S["model"], a
    assert any(not np.array_equal(before.pt[i]["desc"], after.pt[i]["desc"]) and before.in_vision(i, 2) and after.in_vision(i, 2) for i in near)
    assert any(before.in_vision(i, 2) and not after.in_vision(i, 2) for i in far)
    assert any(after.slots[2].get(2 * i + 1) == i for i in near)                  # ... the side descriptor's feature took the point
    # stale entries: another map
    stale, st2 = m.fusePointsIntoKeyframes(None, c, *args, th=sc.TH, search_in=sc.restated(orc, S), reevaluate=False)
    assert st2["reevaluated"] == 0 and st2["extra_calls"] == 0
    assert c.state() != b.state()
    # several calls (two keyframes each, then a pair limit that allows one): the same map
    for kw in (dict(max_kf=2), dict(max_pairs=len(S["point_ids"]))):
        d = S["model"].copy()
        n2, _ = m.fusePointsIntoKeyframes(None, d, *args, th=sc.TH, search_in=sc.restated(orc, S), **kw)
        assert n2 == want and d.state() == b.state()


def test_replay_without_the_loop_policy_keeps_the_point_with_more_observations(orc):
    S = sc.loop_scene(seed=4, K=2)
    a, b = S["model"].copy(), S["model"].copy()
    m = ORBMatcher(sc.RATIO, True)
    n_fuse, _ = m.fusePointsIntoKeyframes(None, a, S["target_kfs"], S["point_ids"], None, sc.CAM, sc.SF, th=3.0, bLoop=False, search_in=sc.restated(orc, S))
    want = sc.sequential_loop(orc, S, b, th=3.0, bLoop=False)
    assert n_fuse == want and sum(want) > 0 and a.state() == b.state()
    assert any(a.is_bad(i) for i in range(len(S["kind"])) if S["kind"][i] != "plain")      # a duplicate with six observations won


# ---- 4. the surface ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    from orb_slam2_ros2_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)                       # loading must not need a GPU
    for fn in ("orbfe_fuse_points_into_keyframes_stored", "orbfe_debug_fuse_points_kernels"):
        assert re.search(r"\borbfe_status\s+" + fn + r"\s*\(", hdr) and hasattr(lib, fn) and fn in _lib.EXPORTS
    assert re.search(r"#define\s+ORBFE_FUSE_POINTS_MAX_PAIRS\s+\(1 << 22\)", hdr) and _lib.FUSE_POINTS_MAX_PAIRS == 1 << 22
    assert "#define ORBFE_ABI_VERSION 4" in hdr and lib.orbfe_abi_version() == 4
    assert callable(_lib.Context.fuse_points_into_keyframes_stored) and callable(ORBMatcher.fusePointsIntoKeyframes)


def test_sources_are_in_the_makefile_and_the_file_list():
    mk = open(os.path.join(ROOT, "orb_slam2_ros2_amd", "csrc", "Makefile")).read()
    assert "orbfe_fusepoints.hip" in mk and "k_fusepoints.hip" in mk
    assert "orbfe_fusepoints.hip" in open(os.path.join(ROOT, "orb_slam2_ros2_amd", "csrc", "orbfe_ctx.h")).read()


from test_reference_compile import REF  # noqa: E402  (where the reference's headers are, when they are there)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "ORB_SLAM2")) or shutil.which("g++") is None, reason="needs the reference tree and g++")
def test_dropin_compiles_against_the_reference_headers(tmp_path):
    """g++ -fsyntax-only of tests/cpp/ref_loopfuse_body.cpp: orbfe_loopfuse_dropin.hpp with the reference's LoopClosing.h / KeyFrame.h /
    MapPoint.h / Map.h (symlinks; Frame.h / KeyFrame.h as temporary copies with INTEGRATION section 3's friend line) and the one-line
    bodies of INTEGRATION section 19"""
    from test_reference_compile import _include_dir
    inc = _include_dir(str(tmp_path / "inc"), friend_line=True)
    stubs = os.path.join(ROOT, "tests", "cpp", "stubs")
    host = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + inc, "-I" + stubs, "-I" + os.path.join(stubs, "refgen"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "cpp", "ref_loopfuse_body.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
