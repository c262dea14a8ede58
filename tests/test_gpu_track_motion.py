"""orbfe_track_motion_model_slots on the device against the restatement of track_motion_restatement.py.

Stage by stage, every stage fed with the DEVICE's own previous outputs: the temporary points bit-equal; the assignment, the excluded hits,
the query matches, the match count and the number of searches element for element; the optimisation against orc.pose_only_optimize on the
device's edge list with the tolerance of test_track_chain.py (the pose within 1e-6, at most one inlier flip); Tcw bit-equal to the
conversion of the reported estimate; the post-check on the device's own inlier flags exact; the in-map count and the verdict equal to the
rule on what was reported.  Exact on the boundary scenes.  Then the equivalence with the array call and between the store and the
position form, the shapes and the errors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reloc_refine_restatement as rr  # noqa: E402
import track_motion_restatement as tm  # noqa: E402
import track_motion_scenes as sc  # noqa: E402

OUT_KEYS = ("verdict", "passes", "n_matches", "n_edges", "n_inliers", "n_in_map", "assigned", "final_assigned", "inlier", "excluded_hits",
            "query_matches", "temp", "temp_pos", "pose_se3", "Tcw")


class Rig:
    """the last pair extracted into slots 2 / 3 (stereo pair 1), the current one into 0 / 1 (pair 0), once; a map-point store"""

    def __init__(self, orc, geom):
        from orb_slam2_ros2_amd._lib import Context, MapPointStore
        g = sc.GEOM[geom]
        self.geom, self.nf = geom, g["NF"]
        self.ctx = Context(g["W"], g["H"], n_features=g["NF"], max_images=4)
        assert self.ctx.n_features == g["NF"]
        self.store = MapPointStore()
        for pair, ref, slot in zip(sc.images(geom), sc.frames(orc, geom), (2, 0)):
            (lk, ld), _, nm, ru, dp = self.ctx.frame_stereo(pair[0], pair[1], g["cam"][0], g["cam"][4], slot_left=slot)
            n = len(lk)          # the device's extraction and stereo results are the oracle's, bit for bit
            assert np.array_equal(lk, ref["lk"]) and np.array_equal(ld, ref["ld"]) and nm == ref["n_matches"]
            assert np.array_equal(ru.reshape(-1)[:n], ref["right_u"][:n]) and np.array_equal(dp.reshape(-1)[:n], ref["depth"][:n])

    def upsert(self, s):
        n = len(s["store_ids"])
        if n:
            self.store.upsert(s["store_ids"], pos=s["store_pos"], view_dir=np.zeros((n, 3), np.float32), max_dist=np.ones(n, np.float32),
                              min_dist=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8))

    def run(self, s, by="store", ctx=None, slot=0, last_slot=2, **kw):
        assert s["geom"] == self.geom
        form = dict(store=self.store, last_ids=s["last_ids"]) if by == "store" else dict(last_pos=s["last_pos"])
        if by == "store":
            self.upsert(s)
        form.update(kw)
        return (ctx or self.ctx).track_motion_model_slots(slot, s["pair"], last_slot, s["last_pair"], s["last_flags"], (s["Rcw"], s["tcw"]),
                                                          (s["last_Rcw"], s["last_tcw"], s["last_Rwc"], s["last_twc"]), s["cam"], s["bounds"],
                                                          s["baseline"], s["sigma2"], s["inv_sigma2"], **form)

    def close(self):
        self.store.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def rig(orc):
    r = Rig(orc, "kitti")
    yield r
    r.close()


def check_stages(orc, s, g, **kw):
    """every stage of the device's result g against the restatement fed with the device's own outputs of the stage before"""
    p = dict(tm.DEFAULTS, **kw)
    NF = s["nf"]
    temp, tpos = tm.unproject(s)
    assert np.array_equal(g["temp"], temp) and np.array_equal(g["temp_pos"].view(np.uint32), tpos.view(np.uint32))
    q = tm.queries(s, g["temp"], g["temp_pos"])
    r1 = tm.search(orc, s, q, np.full(NF, -1, np.int32), p["th"], p)
    a, hits, qm, nm, passes = r1["assigned"], r1["hits"], r1["accepted"].astype(np.int32), r1["n_added"], 1
    if nm < p["min_matches"] and p["th_second"] > 0:
        r2 = tm.search(orc, s, q, a, p["th_second"], p)
        a, hits, qm, nm, passes = r2["assigned"], hits + r2["hits"], qm + r2["accepted"], nm + r2["n_added"], 2
    assert g["passes"] == passes and g["n_matches"] == nm
    assert np.array_equal(g["assigned"], a) and np.array_equal(g["excluded_hits"], hits) and np.array_equal(g["query_matches"], qm)
    if nm < p["min_matches"]:
        assert g["verdict"] == tm.REJECT_MATCHES and np.array_equal(g["final_assigned"], a)
        assert g["n_edges"] == 0 and g["n_inliers"] == 0 and g["n_in_map"] == 0
        assert not g["inlier"].any() and not g["pose_se3"].any() and not g["Tcw"].any()
        return
    pose_ref, ef, inl_ref = tm.optimise(orc, s, q, a)
    assert g["n_edges"] == len(ef)
    if len(ef):
        assert np.abs(g["pose_se3"] - pose_ref).max() < 1e-6
    else:
        assert np.array_equal(g["pose_se3"], rr.tcw_to_se3(s["Rcw"], s["tcw"]))
    R, t = rr.se3_to_tcw(g["pose_se3"])
    assert np.array_equal(g["Tcw"].view(np.uint32), np.concatenate([R, t]).view(np.uint32))
    c = tm.post_check(s, q, a, ef, inl_ref, g["pose_se3"])
    assert (c["inlier"] != g["inlier"]).sum() <= 1                         # an edge exactly on a threshold may flip
    # the post-check and the nulling on the device's own inlier flags: every inlier is an edge that passes the projection test
    dev_in = np.flatnonzero(g["inlier"])
    assert (a[dev_in] >= 0).all() and g["n_inliers"] == len(dev_in)
    own = tm.post_check(s, q, a, dev_in, np.ones(len(dev_in), bool), g["pose_se3"])
    assert np.array_equal(own["inlier"], g["inlier"])
    final = a.copy()
    final[g["inlier"] == 0] = -1
    assert np.array_equal(g["final_assigned"], final)
    assert g["n_in_map"] == tm.count_in_map(s, g["final_assigned"])
    assert g["verdict"] == (tm.ACCEPT if g["n_in_map"] >= p["min_inliers"] else tm.REJECT_INLIERS)


def same(a, b):
    return all(np.array_equal(np.atleast_1d(a[k]).view(np.uint8), np.atleast_1d(b[k]).view(np.uint8)) for k in OUT_KEYS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.SCENES)
def test_every_scene_stage_by_stage_and_free_running(orc, rig, name):
    s, o, kw = sc.scene(orc, name)
    g = rig.run(s, **kw)
    check_stages(orc, s, g, **kw)
    assert g["verdict_name"] == o["verdict_name"] and g["passes"] == o["passes"] and np.array_equal(g["assigned"], o["assigned"])
    if name == "second":        # the matches of the first search stay; the second one met them as excluded candidates
        assert g["passes"] == 2 and g["excluded_hits"].sum() >= 12 and (g["query_matches"] <= 2).all()
    if name == "zero":
        assert g["n_matches"] == 0 and (g["assigned"] == -1).all() and not g["temp"].any()
    if name == "all_temp":
        assert g["temp"].sum() == len(o["q"]["who"]) > 100 and g["n_in_map"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.BOUNDARY))
def test_boundary_scenes_are_exact(orc, rig, name):
    s, o, kw = sc.scene(orc, name)
    g = rig.run(s, **kw)
    check_stages(orc, s, g, **kw)
    assert g["verdict_name"] == sc.BOUNDARY[name] == o["verdict_name"]
    for k in ("passes", "n_matches", "n_edges", "n_inliers", "n_in_map", "inlier", "assigned", "final_assigned", "excluded_hits", "query_matches"):
        assert np.array_equal(g[k], o[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("neither", "mono", "temp_inliers", "in_map_10"))
def test_equals_the_array_call_and_both_forms_agree(orc, rig, name):
    """scenes without a second search: the array call, given the arrays the restatement's M1-M3 produce, runs the same kernels on the same
    lists; the store form and the position form are byte-identical in every output"""
    s, o, kw = sc.scene(orc, name)
    g = rig.run(s, **kw)
    assert g["passes"] == 1 and same(g, rig.run(s, by="pos", **kw)) and same(g, rig.run(s, **kw))
    q = o["q"]
    ai = tm.array_call_inputs(s, q)
    r = rig.ctx.track_motion_model(0, ai["qxy"], ai["q_octave"], ai["q_min_level"], ai["q_max_level"], ai["desc"], ai["pos"], s["cam"], s["bounds"],
                                   rr.tcw_to_se3(s["Rcw"], s["tcw"]), s["sigma2"], s["inv_sigma2"], right_u=s["right_u"])
    assert r["passes"] == 1 and r["n_matches"] == g["n_matches"] and r["n_edges"] == g["n_edges"]
    assert np.array_equal(np.where(r["assigned"] >= 0, q["who"][np.maximum(r["assigned"], 0)], -1), g["assigned"])
    assert np.array_equal(r["pose"].view(np.uint64), g["pose_se3"].view(np.uint64))
    assert np.array_equal(r["query_matches"], g["query_matches"][q["who"]]) and np.array_equal(r["excluded_hits"], g["excluded_hits"])
    # the optimiser's inlier flags of the array call, through the post-check, are the call's inliers
    e_in = np.flatnonzero(r["inlier"])
    own = tm.post_check(s, q, g["assigned"], e_in, np.ones(len(e_in), bool), g["pose_se3"])
    assert np.array_equal(own["inlier"], g["inlier"])


@pytest.mark.gpu
def test_one_stride_of_the_workgroup_loops(orc):
    """500 features on 640 x 480: every 1024-thread loop runs once (2000 features: twice)"""
    small = Rig(orc, "small")
    try:
        s, o, kw = sc.scene(orc, "small")
        g = small.run(s)
        check_stages(orc, s, g)
        assert g["verdict_name"] == o["verdict_name"] == "ACCEPT" and same(g, small.run(s, by="pos"))
    finally:
        small.close()


@pytest.mark.gpu
def test_a_repeated_id_and_repeated_calls(orc, rig):
    s, o, kw = sc.scene(orc, "in_map_10")
    g = rig.run(s)
    # two last-frame features name one map point: both read the same row
    held = np.flatnonzero(s["last_flags"] & 1)
    t = dict(s, last_ids=s["last_ids"].copy(), last_pos=s["last_pos"].copy())
    t["last_ids"][held[1]] = t["last_ids"][held[0]]
    t["last_pos"][held[1]] = t["last_pos"][held[0]]
    h = rig.run(t)
    check_stages(orc, t, h)
    assert same(h, rig.run(t, by="pos"))
    # the unchanged scene again, then the slots the other way round are another frame pair but a valid call
    assert same(g, rig.run(s))
    back = rig.run(s, by="pos", slot=2, last_slot=0)
    assert back["verdict"] in (1, 2, 3) and not same(back, g)
    assert same(g, rig.run(s))


@pytest.mark.gpu
def test_errors_leave_every_output_untouched(orc, rig):
    from orb_slam2_ros2_amd._lib import Context, MapPointStore, OrbfeError, motion_slots_outputs
    s, o, _ = sc.scene(orc, "in_map_10")
    good = rig.run(s)

    def call(status, ctx=None, match=None, scene=None, **kw):
        """scene: entries of the scene that change; kw: arguments of the run (they override what the form of the call would pass)"""
        a = dict(s, **(scene or {}))
        c = ctx or rig.ctx
        out, ref = motion_slots_outputs(c.n_features, fill=0x5A), motion_slots_outputs(c.n_features, fill=0x5A)
        with pytest.raises(OrbfeError) as ei:
            rig.run(a, ctx=c, out=out, **kw)
        assert ei.value.status == status, str(ei.value)
        if match:
            assert match in str(ei.value), str(ei.value)
        assert all(np.array_equal(out[k].view(np.uint8), ref[k].view(np.uint8)) for k in out)

    # ids the store does not hold are found on the device: the first one is named, nothing is written
    held = np.flatnonzero(s["last_flags"] & 1)
    gone = s["last_ids"][held[[2, 7]]]
    rig.upsert(s)
    rig.store.erase(gone)
    real_upsert, rig.upsert = rig.upsert, lambda scene: None
    try:
        call(1, match=f"map point {int(gone[0])} (last_ids[{int(held[2])}])")
    finally:
        rig.upsert = real_upsert
    assert same(rig.run(s), good)                                              # nothing of the refused call is left in the scratch
    call(1, last_pos=s["last_pos"])                                            # both a store with ids and positions
    call(1, by="pos", last_pos=None)                                           # neither
    call(1, by="pos", store=rig.store)                                         # a store without ids
    call(1, last_slot=0)                                                       # slot == last_slot
    call(1, slot=4)                                                            # slots and pairs out of range
    call(1, last_slot=-1)
    call(1, scene=dict(pair=2))
    call(1, scene=dict(last_pair=2))
    nan = s["Rcw"].copy(); nan[4] = np.nan
    call(1, scene=dict(Rcw=nan))                                               # a pose, a bound, a camera entry that is not finite
    inf = s["last_twc"].copy(); inf[1] = np.inf
    call(1, scene=dict(last_twc=inf))
    call(1, scene=dict(bounds=(0.0, np.inf, 0.0, s["bounds"][3])))
    call(1, scene=dict(cam=(s["cam"][0], np.nan) + tuple(s["cam"][2:])))
    g = sc.GEOM["kitti"]
    big = Context(g["W"], g["H"], n_features=2100, max_images=2)               # a context of more than 2048 features
    call(2, ctx=big, by="pos", slot=0, last_slot=1,
         scene=dict(pair=-1, last_pair=-1, last_flags=np.zeros(2100, np.uint8), last_pos=np.zeros((2100, 3), np.float32)))
    big.close()
    import torch
    if torch.cuda.device_count() > 1:                                          # a store made for another device: refused before any launch
        far = MapPointStore(device_id=1)
        call(1, store=far, match="device")
        far.close()
    # a NULL required array is refused by the C entry itself
    import ctypes as C
    from orb_slam2_ros2_amd._lib import MotionSlotsOutput
    args, keep = rig.ctx.track_motion_slots_call(0, s["pair"], 2, s["last_pair"], s["last_flags"], (s["Rcw"], s["tcw"]),
                                                 (s["last_Rcw"], s["last_tcw"], s["last_Rwc"], s["last_twc"]), s["cam"], s["bounds"], s["baseline"],
                                                 s["sigma2"], s["inv_sigma2"], last_pos=s["last_pos"])
    assert rig.ctx.lib.orbfe_track_motion_model_slots(*args) == 0 and keep[-1]["verdict"][0] == tm.ACCEPT
    broken = MotionSlotsOutput.from_buffer_copy(args[-1]._obj)
    broken.temp_pos = None
    assert rig.ctx.lib.orbfe_track_motion_model_slots(*args[:-1], C.byref(broken)) == 1
    # afterwards the same context and store still answer
    assert same(rig.run(s), good)


@pytest.mark.gpu
def test_dropin_track_motion_model_equals_the_body_on_the_bodies(tmp_path):
    """tests/cpp/test_motion_dropin.cpp: one small map per scenario on stand-in classes, built twice; the reference's body of
    Tracking::trackMotionModel on the existing bodies (Frame::unProject, Bodies::trackMotionModel, the isInMap count) on one copy,
    orbfe::dropin::trackMotionModel (one device call) on the other: the verdict, the temporary points to the bit, the frame's final map
    points, the pose, both counters of every point.  Four scenarios: accepted; too few matches without depth; many temporaries but too few
    in-map inliers; a current frame that arrives holding a point (the fallback)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "orb_slam2_ros2_amd")
    exe = str(tmp_path / "test_motion_dropin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(root, "tests", "cpp", "stubs"), "-o", exe,
                           os.path.join(root, "tests", "cpp", "test_motion_dropin.cpp"), "-L" + pkg, "-lorbfe_hip", "-pthread",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=600)
    g = sc.GEOM["kitti"]
    last, cur = sc.images("kitti")
    names = []
    for tag, im in zip(("lastL", "lastR", "curL", "curR"), last + cur):
        im.tofile(tmp_path / (tag + ".raw"))
        names.append(str(tmp_path / (tag + ".raw")))
    out = subprocess.run([exe, *names, str(g["W"]), str(g["H"])], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    tag, *rows = out.stdout.split()
    rows = [r.split(":") for r in rows]           # accepted, matches, points held at the end, temporaries, the device call was made
    assert tag == "MOTION_OK" and [r[0] for r in rows] == ["1", "0", "0", "1"] and [r[4] for r in rows] == ["1", "1", "1", "0"]
    assert int(rows[0][1]) > 200 and int(rows[1][1]) < 20 and int(rows[1][3]) == 0 and int(rows[2][3]) > 50
