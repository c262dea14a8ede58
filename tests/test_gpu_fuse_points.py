"""The forward fuse over stored keyframes (orbfe_fuse_points_into_keyframes_stored) on the device against the CPU restatement
(fuse_points_restatement.py: the oracle's isInVision / predictLevel and findFeaturesInArea + getBestMatch).  Indices and Hamming distances
are integers: every comparison is exact, element for element.  640 x 480 throughout."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_points_restatement as fr  # noqa: E402
import fuse_points_scenes as sc  # noqa: E402
from orb_slam2_ros2_amd import _lib  # noqa: E402
from orb_slam2_ros2_amd._lib import Context, KeyframeStore, OrbfeError  # noqa: E402

pytestmark = pytest.mark.gpu
ID0 = (1 << 40) + 5          # ids are 64 bit


@pytest.fixture(scope="module")
def ctx():
    c = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
    yield c
    c.close()


class Stored:
    """a scene's keyframes in a store of their own, keyframe k under id ID0 + k"""

    def __init__(self, scene, n_levels=8):
        self.scene, self.st = scene, KeyframeStore(sc.W, sc.H, n_levels)
        self.ids = [ID0 + k for k in range(len(scene["kfs"]))]
        for i, kf in zip(self.ids, scene["kfs"]):
            self.st.add(i, kf["kps"], kf["desc"], bounds=kf["bounds"])

    def run(self, ctx, which=None, pts=None, th=None, ratio=sc.RATIO, kfs=None, **kw):
        S = self.scene
        which = range(len(S["kfs"])) if which is None else which
        kfs = [S["kfs"][k] for k in which] if kfs is None else kfs
        return ctx.fuse_points_into_keyframes_stored(self.st, [self.ids[k] for k in which], sc.poses(kfs), S["pts"] if pts is None else pts, sc.CAM, S["sf"],
                                                     th or S.get("th", sc.TH), ratio, 50, **kw)

    def want(self, orc, which=None, pts=None, th=None, ratio=sc.RATIO, kfs=None):
        S = self.scene
        kfs = [S["kfs"][k] for k in (range(len(S["kfs"])) if which is None else which)] if kfs is None else kfs
        return fr.tables(orc, kfs, S["pts"] if pts is None else pts, sc.CAM, S["sf"], th or S.get("th", sc.TH), ratio)

    def check(self, ctx, orc, **kw):
        t = self.want(orc, **kw)
        bi, bd = self.run(ctx, **kw)
        assert np.array_equal(bi, t["best_idx"]) and np.array_equal(bd, t["best_dist"])
        return t

    def close(self):
        self.st.close()


@pytest.fixture(scope="module")
def small(ctx):
    s = Stored(sc.seeded(1))
    yield s
    s.close()


@pytest.fixture(scope="module")
def small_tables(orc, small):
    """the restatement of the small scene, computed once"""
    return small.want(orc)


# ---- 1. seeded scenes ----------------------------------------------------------------------------------------------------------------------
def test_seeded_scene_equals_the_restatement(ctx, orc, small, small_tables):
    bi, bd = small.run(ctx)
    assert bi.shape == (4, 300) and np.array_equal(bi, small_tables["best_idx"]) and np.array_equal(bd, small_tables["best_dist"])
    assert (bi >= 0).sum() >= 40
    small.check(ctx, orc, th=3.0, ratio=0.6)                     # LocalMapping::fuseMapPoints' forward fuse


def test_four_levels(ctx, orc):
    S = Stored(sc.seeded(2, n_levels=4), n_levels=4)
    t = S.check(ctx, orc)
    assert set(np.unique(t["level"])) == {-1, 0, 1, 2, 3} and (t["best_idx"] >= 0).sum() >= 40
    S.close()


def test_hand_placed_scene_equals_the_restatement(ctx, orc):
    S = Stored(sc.hand())
    t = S.check(ctx, orc)
    assert set(t["reasons"][0]) == set(fr.REASONS) | {"accepted"}
    S.close()


# ---- 2. the candidate list -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 127, 128, 129])
def test_candidate_counts_at_the_fold_boundaries(ctx, orc, n_cand):
    S = Stored(sc.window(n_cand))
    t = S.check(ctx, orc, ratio=1.5)
    assert t["cand"][0][0] == n_cand and t["best_idx"][0][0] >= 0
    S.close()


@pytest.mark.parametrize("where", [(5, 9), (10, 70), (63, 64), (0, 128)])
def test_first_minimum_tied_inside_a_chunk_and_across_chunks(ctx, orc, where):
    dists = np.full(130, 30)
    dists[list(where)] = 4
    S = Stored(sc.window(130, dists=dists, n_decoys=20))
    t = S.check(ctx, orc, ratio=1.5)
    first = np.flatnonzero(S.scene["kfs"][0]["kps"]["octave"] <= 2)[where[0]]
    assert t["cand"][0][0] == 130 and t["best_idx"][0][0] == first and t["best_dist"][0][0] == 4
    bi, bd = S.run(ctx, ratio=1.0)                              # best / second = 1: rejected, the test is strict
    assert bi[0][0] == -1 and bd[0][0] == 0
    S.close()


@pytest.mark.parametrize("at", [(3.0, 200.0), (637.0, 200.0), (300.0, 2.5), (300.0, 477.5), (2.0, 478.0)])
def test_window_clipped_at_an_image_edge(ctx, orc, at):
    S = Stored(sc.window(20, at=at))
    t = S.check(ctx, orc, ratio=1.5)
    assert t["cand"][0][0] == 20 and t["best_idx"][0][0] >= 0
    S.close()


def test_window_over_the_whole_grid(ctx, orc, small):
    t = small.check(ctx, orc, th=2000.0, ratio=0.9)
    octs = [np.bincount(kf["kps"]["octave"], minlength=10) for kf in small.scene["kfs"]]
    whole = max(int(o[max(0, lv - 1):lv + 2].sum()) for o in octs for lv in range(8))      # every feature of an octave window
    assert t["cand"].max() == whole > 64


# ---- 3. the compaction ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 63), (2, 32), (5, 13), (3, 85), (1, 257), (17, 241)])
def test_total_pairs_around_the_wave_and_block_sizes(ctx, orc, small, shape):
    """1, 63, 64, 65, 255, 257 and 4097 pairs; beyond four keyframes the ids repeat, each time with another pose"""
    K, m = shape
    assert K * m in (1, 63, 64, 65, 255, 257, 4097)
    S = small.scene
    which = [k % 4 for k in range(K)]
    kfs = [dict(S["kfs"][k % 4], tcw=(S["kfs"][k % 4]["tcw"] + np.float32(0.02 * (k // 4))).astype(np.float32)) for k in range(K)]
    vis = np.flatnonzero(S["pts"]["usable"])
    pts = sc.take(S["pts"], np.resize(np.concatenate([vis[:3], np.arange(300)]), m))     # (m = 1: a usable point)
    t = small.check(ctx, orc, which=which, pts=pts, kfs=kfs)
    assert K * m < 64 or (t["best_idx"] >= 0).any()


def test_no_survivor_one_survivor_and_a_full_list(ctx, orc, small, small_tables):
    S = small.scene
    vis = small_tables["level"] >= 0
    none = np.flatnonzero(vis.sum(0) == 0)[:70]
    t = small.check(ctx, orc, pts=sc.take(S["pts"], none))
    assert (t["level"] < 0).all() and len(none) == 70
    one = np.concatenate([none[:40], np.flatnonzero(vis.sum(0) == 1)[:1], none[40:]])
    t = small.check(ctx, orc, pts=sc.take(S["pts"], one))
    assert (t["level"] >= 0).sum() == 1
    # every pair survives: the list is full to its capacity
    both = np.flatnonzero(vis[1] & vis[2])
    assert len(both) >= 20
    t = small.check(ctx, orc, which=[1, 2, 1], pts=sc.take(S["pts"], np.resize(both, 130)))
    assert (t["level"] >= 0).all() and t["level"].size == 390


def test_points_visible_in_exactly_one_keyframe(ctx, orc, small, small_tables):
    vis = small_tables["level"] >= 0
    only = np.flatnonzero(vis.sum(0) == 1)
    t = small.check(ctx, orc, pts=sc.take(small.scene["pts"], only))
    assert len(only) >= 10 and ((t["level"] >= 0).sum(0) == 1).all() and (t["best_idx"] >= 0).any()


# ---- 4. what the call promises -------------------------------------------------------------------------------------------------------------
def test_three_calls_return_identical_arrays_and_equal_single_keyframe_calls(ctx, small, small_tables):
    runs = [small.run(ctx) for _ in range(3)]
    for bi, bd in runs:
        assert np.array_equal(bi, small_tables["best_idx"]) and np.array_equal(bd, small_tables["best_dist"])
    for k in range(4):
        bi, bd = small.run(ctx, which=[k])
        assert np.array_equal(bi[0], runs[0][0][k]) and np.array_equal(bd[0], runs[0][1][k])


def test_an_id_appears_twice(ctx, small, small_tables):
    bi, bd = small.run(ctx, which=[2, 0, 2, 2])
    for row, k in enumerate([2, 0, 2, 2]):
        assert np.array_equal(bi[row], small_tables["best_idx"][k]) and np.array_equal(bd[row], small_tables["best_dist"][k])


def test_equals_the_chain_of_existing_calls_per_keyframe(ctx, small, small_tables):
    """project_map_points + search_in_area_features_ex per keyframe, with the radius, the window and the acceptance in numpy as
    frontend.ORBMatcher.searchByProjectionMapPoints does them: what the one call replaces"""
    S = small.scene
    pts, sf = S["pts"], np.asarray(S["sf"], np.float32)
    for k, kf in enumerate(S["kfs"]):
        pr = ctx.project_map_points(pts["pos"], pts["view_dir"], pts["max_dist"], pts["min_dist"], kf["Rcw"], kf["tcw"], sc.CAM, kf["bounds"])
        rows = np.flatnonzero(pts["usable"].astype(bool) & pr["visible"].astype(bool))
        lvl = pr["level"][rows].astype(np.int32)
        base = np.where(pr["cos_theta"][rows] > np.float32(0.998), np.float32(2.5), np.float32(4.0))
        radius = ((base * np.float32(sc.TH)).astype(np.float32) * (sf[lvl] * sf[lvl])).astype(np.float32)
        bi, bd, sd, nc = ctx.search_in_area_features(kf["kps"], kf["desc"], pr["uv"][rows], radius, np.maximum(0, lvl - 1).astype(np.int8),
                                                     np.minimum(7, lvl + 1).astype(np.int8), pts["desc"][rows], None, bounds=kf["bounds"])[:4]
        ok = (nc > 0) & (bd < 50) & (bd.astype(np.float32) / sd.astype(np.float32) < np.float32(sc.RATIO))
        want_i, want_d = np.full(300, -1, np.int32), np.zeros(300, np.int32)
        want_i[rows[ok]], want_d[rows[ok]] = bi[ok], bd[ok]
        assert np.array_equal(want_i, small_tables["best_idx"][k]) and np.array_equal(want_d, small_tables["best_dist"][k])


# ---- 5. degenerate inputs and refusals -----------------------------------------------------------------------------------------------------
def test_degenerate_inputs(ctx, orc, small):
    S, st = small.scene, small.st
    mark = lambda K, m: (np.full((K, m), -7, np.int32), np.full((K, m), -7, np.int32))  # noqa: E731
    # n_kf = 0, m = 0: OK, nothing written
    out = mark(1, 300)
    ctx.fuse_points_into_keyframes_stored(st, [], [], S["pts"], sc.CAM, S["sf"], sc.TH, sc.RATIO, 50, out=out)
    assert (out[0] == -7).all() and (out[1] == -7).all()
    bi, bd = small.run(ctx, pts=sc.take(S["pts"], []))
    assert bi.shape == (4, 0) and bd.shape == (4, 0)
    # a keyframe without features, and one with a single feature
    kf0 = S["kfs"][0]
    st.add(900, kf0["kps"][:0], kf0["desc"][:0], bounds=kf0["bounds"])
    st.add(901, kf0["kps"][:1], kf0["desc"][:1], bounds=kf0["bounds"])
    bi, bd = ctx.fuse_points_into_keyframes_stored(st, [900, 901, small.ids[0]], sc.poses([kf0] * 3), S["pts"], sc.CAM, S["sf"], sc.TH, sc.RATIO, 50)
    t = fr.tables(orc, [dict(kf0, kps=kf0["kps"][:1], desc=kf0["desc"][:1]), kf0], S["pts"], sc.CAM, S["sf"], sc.TH, sc.RATIO)
    assert (bi[0] == -1).all() and (bd[0] == 0).all() and np.array_equal(bi[1:], t["best_idx"]) and np.array_equal(bd[1:], t["best_dist"])
    st.erase([900, 901])
    # no usable point
    t = small.check(ctx, orc, pts=dict(S["pts"], usable=np.zeros(300, np.uint8)))
    assert (t["best_idx"] == -1).all()


def test_refusals_leave_the_outputs_untouched(ctx, orc, small):
    import ctypes
    S, st = small.scene, small.st
    nan_pose = [(S["kfs"][0]["Rcw"], np.array([0, np.nan, 0], np.float32))] + sc.poses(S["kfs"][1:])
    inf_pose = sc.poses(S["kfs"][:3]) + [(np.full((3, 3), np.inf, np.float32), S["kfs"][3]["tcw"])]
    bad = [dict(ids=[small.ids[0], 12345, small.ids[2], small.ids[3]]),           # an unknown id
           dict(sf=S["sf"][:7]),                                                   # n_levels below the store's
           dict(poses=nan_pose), dict(poses=inf_pose),                             # a pose entry
           dict(th=np.nan), dict(th=np.inf), dict(ratio=np.nan), dict(ratio=-np.inf)]
    for kw in bad:
        out = (np.full((4, 300), -7, np.int32), np.full((4, 300), -7, np.int32))
        with pytest.raises(OrbfeError) as ei:
            ctx.fuse_points_into_keyframes_stored(st, kw.get("ids", small.ids), kw.get("poses", sc.poses(S["kfs"])), S["pts"], sc.CAM, kw.get("sf", S["sf"]),
                                                  kw.get("th", sc.TH), kw.get("ratio", sc.RATIO), 50, out=out)
        assert ei.value.status == 1, kw
        assert (out[0] == -7).all() and (out[1] == -7).all(), kw
    # more than ORBFE_FUSE_MAX_KF keyframes: EBADARG; more than ORBFE_FUSE_POINTS_MAX_PAIRS pairs: EBADSIZE; more than 2^20 points: EBADARG
    with pytest.raises(OrbfeError) as ei:
        small.run(ctx, which=[0] * 65, kfs=[S["kfs"][0]] * 65)
    assert ei.value.status == 1
    many = {k: np.resize(v, ((1 << 16) + 1,) + v.shape[1:]) for k, v in S["pts"].items()}
    with pytest.raises(OrbfeError) as ei:
        small.run(ctx, which=[0] * 64, kfs=[S["kfs"][0]] * 64, pts=many)
    assert ei.value.status == 2                                   # ORBFE_EBADSIZE
    # NULL arrays with a non-zero count, through the C call itself
    ids = np.array(small.ids, np.uint64)
    ps = (_lib.FusePose * 4)()
    for k, (R, t) in enumerate(sc.poses(S["kfs"])):
        ps[k].Rcw[:], ps[k].tcw[:] = R.reshape(9).tolist(), t.reshape(3).tolist()
    cam = _lib.Camera(*[float(v) for v in sc.CAM], 0.0)
    sf = np.ascontiguousarray(S["sf"], np.float32)
    bi = np.full((4, 300), -7, np.int32)
    call = lambda p, idp, pp, o1, o2, m=300: ctx.lib.orbfe_fuse_points_into_keyframes_stored(  # noqa: E731
        ctx.h, st.h, 4, idp, pp, ctypes.byref(p), ctypes.byref(cam), _lib.ptr(sf), 8, sc.TH, sc.RATIO, 50, o1, o2)
    null_pts = _lib.Sim3Points(300, None, None, None, None, None, None)
    arrs = [np.ascontiguousarray(S["pts"][k]) for k in sc.POINT_KEYS]
    full = _lib.Sim3Points(300, *[_lib.ptr(a).value for a in arrs])
    pp = ctypes.cast(ps, ctypes.c_void_p)
    assert call(null_pts, _lib.ptr(ids), pp, _lib.ptr(bi), _lib.ptr(bi)) == 1
    assert call(full, None, pp, _lib.ptr(bi), _lib.ptr(bi)) == 1 and call(full, _lib.ptr(ids), None, _lib.ptr(bi), _lib.ptr(bi)) == 1
    assert call(full, _lib.ptr(ids), pp, None, _lib.ptr(bi)) == 1 and call(full, _lib.ptr(ids), pp, _lib.ptr(bi), None) == 1
    assert (bi == -7).all()
    # a context on another device (where the machine has one)
    import torch
    if torch.cuda.device_count() > 1:
        far = Context(640, 480, n_features=2000, n_levels=8, device_id=1, max_images=1)
        with pytest.raises(OrbfeError) as ei:
            far.fuse_points_into_keyframes_stored(st, small.ids, sc.poses(S["kfs"]), S["pts"], sc.CAM, S["sf"], sc.TH, sc.RATIO, 50)
        assert ei.value.status == 1
        far.close()
    # afterwards the same context and store still answer
    small.check(ctx, orc, which=[1])


# ---- 6. larger shapes ----------------------------------------------------------------------------------------------------------------------
def test_eight_keyframes_fifteen_hundred_points(ctx, orc):
    S = Stored(sc.seeded(6, K=8, m=1500, n=500, n_pts=1200))
    assert all(len(kf["kps"]) == 500 for kf in S.scene["kfs"])
    t = S.check(ctx, orc)
    assert t["best_idx"].shape == (8, 1500) and (t["best_idx"] >= 0).sum() > 500
    S.close()


def test_a_point_list_too_large_for_the_staging_buffer(ctx, small, small_tables):
    """past 8 MB the arrays are copied directly instead of through the page-locked buffer: the small scene's points 534 times over
    (160200 points, 10 MB) against one keyframe must give the small list's answer 534 times over"""
    S = small.scene
    big = {k: np.concatenate([S["pts"][k]] * 534) for k in sc.POINT_KEYS}
    assert len(big["usable"]) >= 160000 and len(big["usable"]) * 65 > (8 << 20)
    bi, bd = small.run(ctx, which=[1], pts=big)
    assert np.array_equal(bi[0], np.tile(small_tables["best_idx"][1], 534)) and np.array_equal(bd[0], np.tile(small_tables["best_dist"][1], 534))
    bi, bd = small.run(ctx, which=[1])                          # and the staged path still answers afterwards
    assert np.array_equal(bi[0], small_tables["best_idx"][1])


# ---- 7. drop-in ----------------------------------------------------------------------------------------------------------------------------
def test_dropin_loop_fuse_equals_the_chain_of_plain_fuses(tmp_path):
    """tests/cpp/test_loopfuse_dropin.cpp: one map on stand-in classes built twice; the chain of Bodies::fuse(pkf, pts, map, true, 4.0f, 0.8f, 8)
    against fuseLoopPoints(.., store): equal final maps, re-evaluations counted; the single-keyframe overload against Bodies::fuse with
    bLoop = false"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "orb_slam2_ros2_amd")
    exe = str(tmp_path / "tl")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(root, "tests", "cpp", "stubs"), "-I" + os.path.join(pkg, "host"),
                           "-I" + os.path.join(root, "include"), "-o", exe, os.path.join(root, "tests", "cpp", "test_loopfuse_dropin.cpp"), "-L" + pkg,
                           "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    inp = tmp_path / "in.txt"
    sc.write_dropin_input(sc.loop_scene(), str(inp))
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    tag, n_chain, n_loop, reeval, extra, n_single = r.stdout.split()
    assert tag == "OK" and int(n_chain) == int(n_loop) > 20 and int(reeval) > 0 and int(extra) > 0 and int(n_single) > 5
