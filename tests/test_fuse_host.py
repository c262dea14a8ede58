"""fuseMapPoints without a device: the expected tables of the scenes the GPU tests use are not vacuous, the replay of
MatcherExt.fuseIntoKeyframes on the batch tables equals the plain sequential chain on the live map, and the C++ drop-in compiles against
the reference's class declarations."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_restatement as fr  # noqa: E402
import fuse_scenes as fs  # noqa: E402
from orb_slam2_ros2_amd.frontend import ORBMatcher  # noqa: E402
from orb_slam2_ros2_amd.matcher_ext import tlc_z  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def expected(orc, sc):
    return fr.fuse_into_keyframes(orc, sc["cur"], sc["pts"], sc["targets"], sc["z"], fs.CAM, fs.BL, fs.SF)


@pytest.mark.parametrize("name", fs.GPU_SCENES)
def test_expected_tables_are_not_vacuous(orc, name):
    sc = fs.gpu_scene(name)
    bi, bd, vis = expected(orc, sc)
    K = len(sc["targets"])
    has = sc["pts"]["has_point"].astype(bool)
    assert int(((bi >= 0).sum(1) > 0).sum()) * 2 >= K                       # accepted matches in at least half of the targets
    assert set(np.unique(vis[:, has])) == {0, 1}                            # both values of `visible` among slots that hold a point
    assert {fr.window_case(z, fs.BL) for z in sc["z"]} == {0, 1, 2}         # all three octave-window cases
    assert np.all(bd[bi < 0] == 0) and np.all(vis[:, ~has] == 0)
    if len(has) >= 63:
        assert set(sc["cur"]["kps"]["octave"]) == set(range(8)) and not has.all()   # every octave, and slots without a point


@pytest.mark.parametrize("count", [63, 64, 65, 200])
def test_dense_cell_construction(orc, count):
    sc = fs.dense_cell_scene(count)
    t, q = sc["targets"][0], sc["cur"]
    n = len(q["kps"])
    rad = np.full(n, F32(3.0) * (fs.SF[2] * fs.SF[2]), F32)
    nc = orc.search_in_area_ex(t["kps"], t["desc"], t["bounds"], np.stack([q["kps"]["x"], q["kps"]["y"]], 1), rad, np.full(n, 1, np.int8),
                               np.full(n, 3, np.int8), q["desc"])[3]
    assert np.all(nc == count)                                               # every query sees the whole cell, and only the window's octaves
    bi, _, _ = expected(orc, sc)
    assert np.all(bi >= 0) and len(set(bi[0])) >= 4                          # matches early, late and across the 64-candidate boundary


def test_border_construction(orc):
    sc = fs.border_scene()
    bi, _, vis = expected(orc, sc)
    x = sc["cur"]["kps"]["x"]
    assert (x == fs.W).sum() >= 3 and fs.W % 64 == 0 and (bi >= 0).any() and {fr.window_case(z, fs.BL) for z in sc["z"]} == {0, 1, 2}


def test_in_vision_and_tlc_z_equal_the_oracle(orc):
    sc = fs.gpu_scene("mid")
    m, n = sc["model"], len(sc["cur"]["kps"])
    _, _, vis = expected(orc, sc)
    for k, kf in enumerate(sc["target_kfs"]):
        for i in range(n):
            if sc["pts"]["has_point"][i]:
                assert m.in_vision(m.slot(fs.CUR, i), kf) == bool(vis[k][i]), (k, i)
    # cur at the origin looking down +z: tlc.z is the target centre's z
    R = np.eye(3, dtype=F32)
    assert tlc_z(R, -np.array([0.1, 0.2, 0.3], F32), R, np.zeros(3, F32)) == F32(0.3)


@pytest.mark.parametrize("name", ["k3", "mid", "k64"])
def test_replay_equals_sequential_chain(orc, name):
    sc = fs.gpu_scene(name)
    a, b, c = sc["model"].copy(), sc["model"].copy(), sc["model"].copy()
    args = (sc["target_kfs"], sc["cur"], sc["pts"], sc["targets"], sc["z"], fs.CAM, fs.BL, fs.SF)
    n_fuse, stats = ORBMatcher(0.6, True).fuseIntoKeyframes(None, a, fs.CUR, *args, search_in=fs.restated(orc))
    want = fs.sequential_chain(orc, sc, b)
    assert n_fuse == want and sum(want) > 0
    assert a.state() == b.state()                                            # slots of every keyframe, observations, bad flags
    assert stats["device_flags"] > 0
    if name != "k3":
        # a replace changed a later target's visibility: the live re-evaluation is needed, a stale device flag gives another map
        assert stats["reevaluated"] > 0
        stale, _ = ORBMatcher(0.6, True).fuseIntoKeyframes(None, c, fs.CUR, *args, search_in=fs.restated(orc), reevaluate=False)
        assert stale != want or c.state() != b.state()
        assert c.state() != b.state()


# ---- the drop-in through the compiler ---------------------------------------------------------------------------------------------
REF = "/root/reference/src/ORB_SLAM2"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "ORB_SLAM2")) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++")
def test_dropin_compiles_against_the_reference_headers(tmp_path):
    """g++ -fsyntax-only of tests/cpp/ref_fuse_body.cpp: orbfe_fuse_dropin.hpp with the reference's LocalMapping.h / KeyFrame.h / MapPoint.h /
    Map.h (symlinks; Frame.h / KeyFrame.h as temporary copies with INTEGRATION section 3's friend line) and LocalMapping::fuseMapPoints as
    its one-line body"""
    from test_reference_compile import _include_dir
    inc = _include_dir(str(tmp_path / "inc"), friend_line=True)
    stubs = os.path.join(ROOT, "tests", "cpp", "stubs")
    host = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + inc, "-I" + stubs, "-I" + os.path.join(stubs, "refgen"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "cpp", "ref_fuse_body.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
