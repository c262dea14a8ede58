"""The device-resident keyframe store (orbfe_kfstore) and the two calls over it, on the device.  Every comparison is between integers,
flags or copied bytes: the stored calls must equal the plain device calls (and the restatements) bit for bit, a fetched entry must be the
bytes that went in, and the stored grid must be VirtualFrame::initGrid restated in numpy.  No tolerances."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_restatement as fr  # noqa: E402
import fuse_scenes as fs  # noqa: E402
import tri_scenes as ts  # noqa: E402
import triangulation_restatement as tr  # noqa: E402
from orb_slam2_ros2_amd._lib import KP_DTYPE, Context, KeyframeStore, OrbfeError  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUR_ID = 1 << 40          # ids are 64 bit: the current keyframe's does not fit 32


@pytest.fixture(scope="module")
def ctx():
    c = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
    yield c
    c.close()


def eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- VirtualFrame::initGrid (src/Frame.cc:53-69), restated -----------------------------------------------------------------------------
def cv_ceil(v):
    i = int(v)
    return i + (i < v)


def init_grid(kps, bounds):
    """-> (rows, cols, cell_off, cell_feat): cells of 64 x 48 from the bounds, cvFloor(coordinate / size) clamped to the grid at both ends (a
    coordinate that is not > 0 in cell 0), each cell's features in ascending index"""
    b = np.asarray(bounds, F32)
    rows, cols = cv_ceil(F32(b[3] - b[2]) / F32(48)), cv_ceil(F32(b[1] - b[0]) / F32(64))

    def cell(v, size, n):
        q = v.astype(F32) / F32(size)
        with np.errstate(invalid="ignore"):
            return np.where(~(q > 0), 0, np.where(q >= F32(n - 1), n - 1, np.floor(q))).astype(np.int64)
    c = cell(kps["y"], 48, rows) * cols + cell(kps["x"], 64, cols)
    off = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=rows * cols))]).astype(np.int32)
    return rows, cols, off, np.argsort(c, kind="stable").astype(np.int32)


def check_entry(st, kid, kf, depth=None, right_u=None):
    n = len(kf["kps"])
    got = st.fetch(kid)
    assert eq(got["kps"], np.ascontiguousarray(kf["kps"], KP_DTYPE)) and eq(got["desc"], np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1, 32))
    assert eq(got["depth"], np.full(n, -1.0) if depth is None else np.asarray(depth, np.float64))
    assert eq(got["right_u"], np.full(n, -1.0) if right_u is None else np.asarray(right_u, np.float64))
    rows, cols, off, feat = init_grid(kf["kps"], kf["bounds"])
    info = st.info(kid)
    assert info["n"] == n and info["grid"] == (rows, cols) and eq(info["bounds"], np.asarray(kf["bounds"], F32))
    assert eq(got["cell_off"], off) and eq(got["cell_feat"], feat)
    return got


def rand_kf(rng, n, centre=(0, 0, 0), bounds=fs.BOUNDS):
    kps = np.zeros(n, KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, fs.W, n).astype(F32), rng.uniform(0, fs.H, n).astype(F32)
    kps["octave"], kps["size"], kps["class_id"] = rng.integers(0, 8, n), 7.0, -1
    return fs._kf(kps, rng.integers(0, 256, (n, 32), dtype=np.uint8), centre, bounds)


def rand_scene(rng, targets, n_cur=200):
    """queries cut out of the targets' own features (a few bits flipped), so that every target has matches"""
    src = [t for t in targets if len(t["kps"]) > 0]
    pick = [(src[i % len(src)], int(rng.integers(0, len(src[i % len(src)]["kps"])))) for i in range(n_cur)]
    q = np.array([t["kps"][j] for t, j in pick], KP_DTYPE)
    qd = np.array([t["desc"][j] for t, j in pick], np.uint8)
    qd[:, 3] ^= 5
    z = np.array([[0.2, -0.2, 0.0][k % 3] for k in range(len(targets))], F32)
    return dict(cur=fs._kf(q, qd), targets=targets, z=z, pts=fs._points_in_front(rng, q))


# ---- round trip ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 500])
def test_round_trip(n):
    rng = np.random.default_rng(n)
    st = KeyframeStore(fs.W, fs.H, 8)
    kf = rand_kf(rng, n)
    depth, ru = rng.uniform(-1, 30, n), rng.uniform(-1, 600, n)
    st.add(7, kf["kps"], kf["desc"], depth, ru, kf["bounds"])
    st.add(8, kf["kps"], kf["desc"])                              # no stereo columns, no bounds: -1 and the image
    assert len(st) == 2
    check_entry(st, 7, kf, depth, ru)
    check_entry(st, 8, kf)
    assert st.info(7)["has_bow"] is False and st.fetch(7)["fv"] is None and st.info(7)["bytes"] > 80 * n
    st.close()


def test_round_trip_dense_cell_borders_and_other_bounds():
    st = KeyframeStore(fs.W, fs.H, 8)
    dense = fs.dense_cell_scene(65)["targets"][0]
    st.add(1, dense["kps"], dense["desc"], bounds=dense["bounds"])
    got = check_entry(st, 1, dense)
    assert np.diff(got["cell_off"]).max() == len(dense["kps"])      # one cell holds them all
    bs = fs.border_scene()
    border = dict(bs["cur"], bounds=fs.BOUNDS)                      # keypoints on every border, at x == width, outside the image
    st.add(2, border["kps"], border["desc"], bounds=border["bounds"])
    check_entry(st, 2, border)
    wide = rand_kf(np.random.default_rng(3), 300, bounds=np.array([-20.5, 700.25, -10, 500], F32))
    wide["kps"]["x"][:20] -= 30                                      # some left of 0, some right of the image
    wide["kps"]["x"][20:40] += 100
    st.add(3, wide["kps"], wide["desc"], bounds=wide["bounds"])
    assert st.info(3)["grid"] == (11, 12) and st.info(1)["grid"] == (10, 10)
    check_entry(st, 3, wide)
    st.close()


def test_add_refuses_bad_input():
    st = KeyframeStore(fs.W, fs.H, 8)
    kf = rand_kf(np.random.default_rng(0), 50)
    st.add(1, kf["kps"], kf["desc"])
    before = st.fetch(1)
    other = rand_kf(np.random.default_rng(1), 70)
    bad_oct = other["kps"].copy()
    bad_oct["octave"][5] = 8
    for kid, kps, bounds in ((1, other["kps"], None), (2, bad_oct, None), (2, other["kps"], (0, 0, 0, 480)), (2, other["kps"], (0, np.nan, 0, 480))):
        with pytest.raises(OrbfeError) as ei:
            st.add(kid, kps, other["desc"], bounds=bounds)
        assert ei.value.status == 1
    with pytest.raises(OrbfeError) as ei:                          # 1024 x 16 cells: more than the grid build's LDS counters hold
        st.add(2, other["kps"], other["desc"], bounds=(0, 65536, 0, 768))
    assert ei.value.status == 2
    assert len(st) == 1 and all(eq(before[k], v) for k, v in st.fetch(1).items() if isinstance(v, np.ndarray))
    with pytest.raises(OrbfeError) as ei:
        st.info(2)
    assert ei.value.status == 1
    st.close()


# ---- add_from_slot ---------------------------------------------------------------------------------------------------------------------
def test_add_from_slot():
    from orb_slam2_ros2_amd import synth
    L, R = synth.stereo_pair(0, 640, 240, n_rect=120)
    c = Context(640, 240, n_features=600, n_levels=6, device_id=0, max_images=2)
    st = KeyframeStore(640, 240, 6)
    try:
        c.frame_stereo(L, R, 400.0, 200.0)
        kps, desc = c.fetch_features(0)
        _, ru, dp, _, _ = c.fetch_stereo(0)
        n = len(kps)
        assert n > 100 and (dp[:n] > 0).any()
        bounds = np.array([0, 640, 0, 240], F32)
        assert st.add_from_slot(c, 1, 0, 0, bounds) == n
        kf = dict(kps=kps, desc=desc, bounds=bounds)
        a = check_entry(st, 1, kf, dp[:n], ru[:n])
        assert st.add_from_slot(c, 2, 0, -1) == n                   # no pair, no bounds
        assert st.info(1)["has_stereo"] and not st.info(2)["has_stereo"]
        check_entry(st, 2, kf)
        st.add(3, kps, desc, dp[:n], ru[:n], bounds)                # the route it replaces
        b = st.fetch(3)
        assert eq(a["cell_off"], b["cell_off"]) and eq(a["cell_feat"], b["cell_feat"]) and st.info(1)["bytes"] == st.info(3)["bytes"]
        with pytest.raises(OrbfeError) as ei:
            st.add_from_slot(c, 1, 0, 0)
        assert ei.value.status == 1 and len(st) == 3
        small = KeyframeStore(640, 240, 5)                          # the extractor's octaves go up to 5
        with pytest.raises(OrbfeError) as ei:
            small.add_from_slot(c, 1, 0, 0)
        assert ei.value.status == 1
        small.close()
    finally:
        st.close()
        c.close()


# ---- stored fuse -------------------------------------------------------------------------------------------------------------------------
def fill(st, sc, first_id=1):
    """the scene's keyframes into the store -> the targets' ids (the current keyframe, if it is a target, under its own id)"""
    st.add(CUR_ID, sc["cur"]["kps"], sc["cur"]["desc"], bounds=sc["cur"]["bounds"])
    ids = []
    for k, t in enumerate(sc["targets"]):
        if t is sc["cur"]:
            ids.append(CUR_ID)
            continue
        st.add(first_id + k, t["kps"], t["desc"], bounds=t["bounds"])
        ids.append(first_id + k)
    return ids


def run_stored(ctx, st, sc, ids, **kw):
    return ctx.fuse_into_keyframes_stored(st, CUR_ID, sc["pts"], ids, sc["targets"], sc["z"], fs.CAM, fs.BL, fs.SF, **kw)


def run_plain(ctx, sc):
    return ctx.fuse_into_keyframes(sc["cur"], sc["pts"], sc["targets"], sc["z"], fs.CAM, fs.BL, fs.SF)


def same_fuse(ctx, orc, sc, restated=True):
    st = KeyframeStore(fs.W, fs.H, 8)
    try:
        got = run_stored(ctx, st, sc, fill(st, sc))
    finally:
        st.close()
    for g, w, what in zip(got, run_plain(ctx, sc), ("best_idx", "best_dist", "visible")):
        assert eq(g, w), what
    if restated:
        for g, w, what in zip(got, fr.fuse_into_keyframes(orc, sc["cur"], sc["pts"], sc["targets"], sc["z"], fs.CAM, fs.BL, fs.SF), ("best_idx", "best_dist", "visible")):
            assert eq(g, w), what
    return got


@pytest.mark.parametrize("name", ["k3", "n1", "n63", "n64", "n65", "k64", "mixed"])   # 'mixed': targets of 0 and 1 features
def test_stored_fuse_bit_exact(ctx, orc, name):
    bi, _, _ = same_fuse(ctx, orc, fs.gpu_scene(name))
    assert (bi >= 0).any()


def test_stored_fuse_dense_cell_and_borders(ctx, orc):
    same_fuse(ctx, orc, fs.dense_cell_scene(65))
    same_fuse(ctx, orc, fs.border_scene())


def test_stored_fuse_one_target_at_a_time_and_cur_among_the_targets(ctx, orc):
    sc = fs.gpu_scene("k3")
    for k in range(3):                                               # K = 1, once per octave-window case
        same_fuse(ctx, orc, dict(sc, targets=sc["targets"][k:k + 1], z=sc["z"][k:k + 1]))
    own = fs.scene(16, K=3, n=200, include_cur=True)
    assert own["targets"][0] is own["cur"]
    bi, _, _ = same_fuse(ctx, orc, own)
    assert (bi[0] == np.arange(bi.shape[1])).any()                   # a feature finds itself in its own keyframe


def test_stored_fuse_follows_the_poses_of_each_call(ctx):
    sc = fs.gpu_scene("k3")
    st = KeyframeStore(fs.W, fs.H, 8)
    try:
        ids = fill(st, sc)
        first = run_stored(ctx, st, sc, ids)
        assert all(eq(a, b) for a, b in zip(first, run_plain(ctx, sc)))
        moved = [dict(t, Rcw=ts.yaw(0.3).astype(F32) @ t["Rcw"], tcw=t["tcw"] + F32(0.4)) for t in sc["targets"]]
        sc2 = dict(sc, targets=moved, z=sc["z"][::-1].copy())
        second = run_stored(ctx, st, sc2, ids)
        assert all(eq(a, b) for a, b in zip(second, run_plain(ctx, sc2)))
        assert not eq(first[2], second[2])                                           # (the visibility did move)
        assert all(eq(a, b) for a, b in zip(run_stored(ctx, st, sc, ids), first))   # and back
    finally:
        st.close()


# ---- stored triangulation ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tri_case():
    cur, nbs, _ = ts.scene(9, n_nb=3, n=300, n_pts=400, baselines=[0.03, 0.08, 0.3], stereo_frac=0.6)   # neighbour 0 inside the baseline skip (T7)
    e = nbs[2]
    empty = dict(e, kps=e["kps"][:0], desc=e["desc"][:0], fv=(np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32)),
                 flags=e["flags"][:0], depth=e["depth"][:0], right_u=e["right_u"][:0])
    nbs = nbs + [empty]
    want = tr.create_new_map_points(cur, nbs, ts.CAM, ts.k_inv(), ts.BL, ts.SF)
    return cur, nbs, want


def tri_store(cur, nbs, with_bow=True):
    st = KeyframeStore(ts.W, ts.H, 8)
    for kid, kf in [(CUR_ID, cur)] + [(1 + i, kf) for i, kf in enumerate(nbs)]:
        st.add(kid, kf["kps"], kf["desc"], kf["depth"], kf["right_u"])
        if with_bow:
            st.set_bow(kid, *kf["fv"])
    return st, [1 + i for i in range(len(nbs))]


def test_stored_triangulation_bit_exact(ctx, tri_case):
    cur, nbs, (want, wtail, _, wcons) = tri_case
    plain = ctx.create_new_map_points(cur, nbs, ts.CAM, ts.k_inv(), ts.BL, ts.SF)
    st, ids = tri_store(cur, nbs)
    try:
        got = ctx.create_new_map_points_stored(st, CUR_ID, cur, ids, nbs, ts.CAM, ts.k_inv(), ts.BL, ts.SF)
        assert all(eq(g, p) for g, p in zip(got, plain))
        recs, tail, cons = got
        assert len(recs) == len(want) and len(recs) > 50 and set(recs["nb"]) == {1, 2} and set(recs["kind"]) == {1, 2, 3} and cons.any() and len(tail)
        for f in ("nb", "q", "t", "kind"):
            assert np.array_equal(recs[f], want[f]), f
        assert np.array_equal(recs["xyz"].view(np.int32), want["xyz"].view(np.int32)) and np.array_equal(tail, wtail) and np.array_equal(cons, wcons)
        fv = st.fetch(2)["fv"]
        assert st.info(2)["has_bow"] and all(eq(a, np.ascontiguousarray(b, a.dtype)) for a, b in zip(fv, nbs[1]["fv"]))
        # capacity exceeded: the counts are set, nothing is written
        with pytest.raises(OrbfeError) as ei:
            ctx.create_new_map_points_stored(st, CUR_ID, cur, ids, nbs, ts.CAM, ts.k_inv(), ts.BL, ts.SF, cap=len(recs) - 1)
        assert ei.value.status == 4 and ctx.last_counts == (len(recs), len(tail))
        assert not any(ctx._tri_stored_keep[4].tobytes()) and not ctx._tri_stored_keep[5].any()      # records and tail as they were
        # a changed map state is followed: every current feature holds a good in-map point -> no candidates
        full = dict(cur, flags=np.full(len(cur["kps"]), 3, np.uint8))
        assert len(ctx.create_new_map_points_stored(st, CUR_ID, full, ids, nbs, ts.CAM, ts.k_inv(), ts.BL, ts.SF)[0]) == 0
    finally:
        st.close()


def test_stored_triangulation_refusals(ctx, tri_case):
    cur, nbs, _ = tri_case
    st, ids = tri_store(cur, nbs, with_bow=False)
    try:
        args = (ts.CAM, ts.k_inv(), ts.BL, ts.SF)
        with pytest.raises(OrbfeError) as ei:                       # no FeatureVector yet
            ctx.create_new_map_points_stored(st, CUR_ID, cur, ids, nbs, *args)
        assert ei.value.status == 1 and "FeatureVector" in str(ei.value)
        nodes, offs, feats = nbs[1]["fv"]
        for bad in ((nodes[::-1].copy(), offs, feats), (nodes, offs, feats + np.uint32(10000))):    # unsorted nodes, a feature index out of range
            with pytest.raises(OrbfeError) as ei:
                st.set_bow(2, *bad)
            assert ei.value.status == 1
        assert st.info(2)["has_bow"] is False
        for kid, kf in [(CUR_ID, cur)] + list(zip(ids, nbs)):
            st.set_bow(kid, *kf["fv"])
        with pytest.raises(OrbfeError) as ei:                       # an unknown neighbour
            ctx.create_new_map_points_stored(st, CUR_ID, cur, ids[:1] + [999], nbs[:2], *args)
        assert ei.value.status == 1 and ctx.last_counts == (0, 0)
        with pytest.raises(OrbfeError) as ei:                       # a state of the wrong length
            ctx.create_new_map_points_stored(st, CUR_ID, cur, ids[:1], [dict(nbs[0], flags=nbs[0]["flags"][:-1])], *args)
        assert ei.value.status == 1
    finally:
        st.close()


# ---- life cycle ------------------------------------------------------------------------------------------------------------------------
def test_life_cycle_across_slabs(ctx):
    rng = np.random.default_rng(5)
    st = KeyframeStore(fs.W, fs.H, 8, slab_bytes=1 << 20)
    try:
        kfs = {}
        for kid in range(1, 13):                                   # a dozen 2000-feature keyframes: six fit a slab
            kfs[kid] = rand_kf(rng, 2000)
            st.add(kid, kfs[kid]["kps"], kfs[kid]["desc"], bounds=kfs[kid]["bounds"])
            for old in kfs:                                        # growth moves nothing
                g = st.fetch(old)
                assert eq(g["kps"], kfs[old]["kps"]) and eq(g["desc"], kfs[old]["desc"])
        used, reserved = st.bytes()
        assert reserved == 2 << 20 and used == 12 * st.info(1)["bytes"] and 150_000 < st.info(1)["bytes"] < 180_000
        st.erase([5, 6, 777])                                       # (unknown ids are ignored)
        assert len(st) == 10
        for kid in (105, 106, 107):
            kfs[kid] = rand_kf(rng, 1000)
            st.add(kid, kfs[kid]["kps"], kfs[kid]["desc"], bounds=kfs[kid]["bounds"])
        assert st.bytes()[1] == 2 << 20                             # all three (81 KB each) went into the 322 KB the two erased ones left
        for kid in kfs:
            if kid not in (5, 6):
                check_entry(st, kid, kfs[kid])
        order = [3, 105, 12, 106, 1, 107]                           # old and new ids
        sc = rand_scene(rng, [kfs[k] for k in order])
        st.add(CUR_ID, sc["cur"]["kps"], sc["cur"]["desc"], bounds=sc["cur"]["bounds"])
        got = run_stored(ctx, st, sc, order)
        assert all(eq(a, b) for a, b in zip(got, run_plain(ctx, sc))) and (got[0] >= 0).any()
        # a present id: refused, nothing changes
        with pytest.raises(OrbfeError) as ei:
            st.add(3, kfs[1]["kps"], kfs[1]["desc"])
        assert ei.value.status == 1
        check_entry(st, 3, kfs[3])
        # an erased or unknown id in a stored call: refused, the outputs untouched
        n = len(sc["cur"]["kps"])
        for ids in (order[:2] + [5], [424242] + order[:2]):
            guard = (np.full((3, n), 7, np.int32), np.full((3, n), 7, np.int32), np.full((3, n), 7, np.uint8))
            with pytest.raises(OrbfeError) as ei:
                run_stored(ctx, st, dict(sc, targets=sc["targets"][:3], z=sc["z"][:3]), ids, out=guard)
            assert ei.value.status == 1 and all((g == 7).all() for g in guard)
        with pytest.raises(ValueError):                            # rows for 200 features against a stored keyframe of 2000: the binding refuses
            ctx.fuse_into_keyframes_stored(st, 3, sc["pts"], order, sc["targets"], sc["z"], fs.CAM, fs.BL, fs.SF)
        st.erase([CUR_ID])                                          # the current keyframe erased
        with pytest.raises(OrbfeError) as ei:
            run_stored(ctx, st, sc, order)
        assert ei.value.status == 1
    finally:
        st.close()


def test_entry_larger_than_a_slab(ctx):
    rng = np.random.default_rng(6)
    st = KeyframeStore(fs.W, fs.H, 8, slab_bytes=64 << 10)
    try:
        big, small = rand_kf(rng, 2000), rand_kf(rng, 100)          # 161 KB against slabs of 64 KB
        st.add(1, big["kps"], big["desc"], bounds=big["bounds"])
        st.add(2, small["kps"], small["desc"], bounds=small["bounds"])
        assert st.info(1)["bytes"] > 64 << 10 and st.bytes()[1] == st.info(1)["bytes"] + (64 << 10)
        check_entry(st, 1, big)
        check_entry(st, 2, small)
        sc = rand_scene(rng, [big, small], n_cur=65)
        st.add(CUR_ID, sc["cur"]["kps"], sc["cur"]["desc"], bounds=sc["cur"]["bounds"])
        assert all(eq(a, b) for a, b in zip(run_stored(ctx, st, sc, [1, 2]), run_plain(ctx, sc)))
        st.erase([1])
        assert st.bytes()[1] == 64 << 10                            # its allocation went back whole
        check_entry(st, 2, small)
    finally:
        st.close()


def test_two_threads_two_contexts_one_store(ctx):
    sc = fs.gpu_scene("mid")
    st = KeyframeStore(fs.W, fs.H, 8)
    ids = fill(st, sc)
    out = [None, None]

    def work(i):
        c = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
        try:
            out[i] = [run_stored(c, st, sc, ids) for _ in range(3)]
        finally:
            c.close()
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    try:
        assert out[0] is not None and out[1] is not None
        ref = run_plain(ctx, sc)
        for res in out[0] + out[1]:
            assert all(eq(a, b) for a, b in zip(res, ref))
    finally:
        st.close()


# ---- drop-in -----------------------------------------------------------------------------------------------------------------------------
def build_dropin(tmp_path, name, *defs):
    pkg = os.path.join(ROOT, "orb_slam2_ros2_amd")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", *defs, "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), "-I" + os.path.join(pkg, "host"),
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_kfstore_dropin.cpp"), "-L" + pkg,
                           "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    return exe


def test_dropin_fuse_over_the_store(tmp_path):
    """tests/cpp/test_kfstore_dropin.cpp: the same map through orbfe::dropin::fuseMapPoints and through the overload that takes a store"""
    sc = fs.scene(21, K=9, n=300, include_cur=True)
    t = sc["target_kfs"]
    conn = {fs.CUR: t[1:5], t[1]: [fs.CUR, t[5], t[6]], t[2]: [t[6], t[7]], t[3]: [t[8], t[1]], t[4]: []}
    inp = tmp_path / "in.txt"
    fs.write_dropin_input(sc, str(inp), conn)
    r = subprocess.run([build_dropin(tmp_path, "tf"), str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    tag, n_fuse, flags, reeval, n_replaced, n_targets = r.stdout.split()
    assert tag == "OK" and int(n_targets) == 9 and int(n_fuse) > 50 and int(n_replaced) > 10 and int(flags) > 0 and int(reeval) > 0


def test_dropin_create_new_map_points_over_the_store(tmp_path):
    """... and createNewMapPoints on the input format of tests/cpp/test_tri_dropin.cpp"""
    cur, nbs, _ = ts.scene(8, n_nb=4, n=400, n_pts=1200)
    f = lambda v: repr(float(v))  # noqa: E731
    lines = [" ".join(f(v) for v in ts.CAM), " ".join(f(v) for v in ts.k_inv().reshape(9)), f(ts.BL), f"{len(ts.SF)} " + " ".join(f(v) for v in ts.SF),
             str(1 + len(nbs))]
    for k, kf in enumerate([cur] + nbs):
        lines.append(f"{len(kf['kps'])} " + " ".join(f(v) for v in np.concatenate([kf["Tcw"].reshape(16), kf["Twc"].reshape(16), kf["Ow"]])))
        for i, kp in enumerate(kf["kps"]):
            s = f"{f(kp['x'])} {f(kp['y'])} {int(kp['octave'])} {f(kf['depth'][i])} {f(kf['right_u'][i])} {int(kf['flags'][i])} " + \
                " ".join(str(int(b)) for b in kf["desc"][i])
            if k == 0:
                s += f" {int(kf['unproc'][i])} " + " ".join(f(v) for v in kf["unproc_pos"][i])
            lines.append(s)
        nodes, offs, feats = kf["fv"]
        lines.append(str(len(nodes)))
        for j in range(len(nodes)):
            lines.append(f"{int(nodes[j])} {offs[j + 1] - offs[j]} " + " ".join(str(int(x)) for x in feats[offs[j]:offs[j + 1]]))
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([build_dropin(tmp_path, "tt", "-DKFSTORE_TRI"), str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    tag, n_added, n_stored, n_again, n_own_stereo = r.stdout.split()
    assert tag == "OK" and int(n_added) > 20 and int(n_stored) == 5 and int(n_own_stereo) > 0     # (stereo records: the columns were not lost)
