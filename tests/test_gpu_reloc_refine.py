"""orbfe_reloc_refine_stored on the device against the restatement of reloc_refine_restatement.py.

Stage by stage, every stage fed with the DEVICE's own previous outputs: an optimisation against orc.pose_only_optimize on the device's
edge list with the tolerance of test_track_chain.py (at most one inlier flip, the pose within 1e-6); Tcw bit-equal to the conversion of
the reported estimate; the post-check, the nulling, tlc.z, the windows, the hits, the accepted queries, the last-wins assignment and the
counts element for element; the verdict equal to the rule on the reported counts.  Free-running on the margin scenes (verdict and final
assignment) and exact on the boundary scenes of 9 / 10 / 49 / 50 seeds.  Then the shapes and the errors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reloc_refine_restatement as rr  # noqa: E402
import reloc_refine_scenes as sc  # noqa: E402

from orb_slam2_ros2_amd import synth  # noqa: E402

P = rr.DEFAULTS
OUT_KEYS = ("n_edges", "n_inliers", "n_added", "tlc_z", "pose_se3", "Tcw", "inlier", "assigned", "final_assigned", "excluded_hits", "query_accepted")


class Rig:
    def __init__(self):
        from orb_slam2_ros2_amd._lib import Context, KeyframeStore
        self.ctx = Context(sc.W, sc.H, n_features=sc.NF, max_images=2)
        assert self.ctx.n_features == sc.NF
        self.store = KeyframeStore(sc.W, sc.H)
        self.in_slot = None
        self.next_id = 100

    def frame(self, s):
        """the scene's frame into slot 0 (the device's extraction is the oracle's, bit for bit)"""
        if self.in_slot != s["image_seed"]:
            (kps, desc), _ = self.ctx.extract_batch(list(synth.stereo_pair(s["image_seed"])))
            assert np.array_equal(kps, s["kps"]) and np.array_equal(desc, s["desc"])
            self.in_slot = s["image_seed"]

    def keyframe(self, s):
        self.next_id += 1
        self.store.add(self.next_id, s["kf_kps"], s["kf_desc"], bounds=sc.BOUNDS)
        return self.next_id

    def run(self, s, kf_id=None, **kw):
        self.frame(s)
        own = kf_id is None
        kf_id = self.keyframe(s) if own else kf_id
        try:
            return self.ctx.reloc_refine_stored(0, self.store, kf_id, s["good"], s["pos"], s["kf_Rcw"], s["kf_tcw"], s["held"], s["Rcw"], s["tcw"],
                                                s["cam"], s["bounds"], s["sigma2"], s["inv_sigma2"], s["baseline"], right_u=s["right_u"], **kw)
        finally:
            if own:
                self.store.erase([kf_id])

    def close(self):
        self.store.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def check_stages(orc, s, g, P=P):
    """every stage of the device's result g against the restatement fed with the device's own outputs of the stage before
    -> the stages that ran, as a string (o: optimisation + post-check, s: search)"""
    ran = ""
    cur = rr.seed(s)
    p_init = rr.tcw_to_se3(s["Rcw"], s["tcw"])
    before = (np.asarray(s["Rcw"], np.float32).reshape(9), np.asarray(s["tcw"], np.float32).reshape(3))
    expect = 0
    for st in range(2):
        ran += "o"
        pose_ref, ef, inl_ref = rr.optimise(orc, s, cur, p_init)
        assert g["n_edges"][st] == len(ef)
        if len(ef):
            assert np.abs(g["pose_se3"][st] - pose_ref).max() < 1e-6
        else:
            assert np.array_equal(g["pose_se3"][st], p_init)
        R, t = rr.se3_to_tcw(g["pose_se3"][st])
        assert np.array_equal(g["Tcw"][st].view(np.uint32), np.concatenate([R, t]).view(np.uint32))
        c = rr.post_check(s, cur, ef, inl_ref, g["pose_se3"][st], before)
        assert (c["inlier"] != g["inlier"][st]).sum() <= 1                     # an edge exactly on a threshold may flip
        # the post-check and the nulling on the device's own inlier flags: every inlier is an edge that passes the projection test
        dev_in = np.flatnonzero(g["inlier"][st])
        assert (cur[dev_in] >= 0).all() and g["n_inliers"][st] == len(dev_in)
        own = rr.post_check(s, cur, dev_in, np.ones(len(dev_in), bool), g["pose_se3"][st], before)
        assert np.array_equal(own["inlier"], g["inlier"][st])
        dropped = np.flatnonzero((c["inlier"] == 0) & (cur >= 0))
        assert np.isin(dropped, dev_in).sum() <= 1
        cur = cur.copy()
        cur[g["inlier"][st] == 0] = -1
        n_in = int(g["n_inliers"][st])
        if st == 0 and n_in < P["min_inliers"]:
            expect = rr.REJECT_1
            break
        if n_in >= P["enough"]:
            expect = rr.ACCEPT_1 if st == 0 else rr.ACCEPT_2
            break
        ran += "s"
        r = rr.search(orc, s, cur, R, t, P["th_first"] if st == 0 else P["th_second"], P)
        assert np.float32(r["tlc_z"]).view(np.uint32) == g["tlc_z"][st].view(np.uint32)
        assert np.array_equal(r["hits"], g["excluded_hits"][st]) and np.array_equal(r["accepted"], g["query_accepted"][st])
        assert r["n_added"] == g["n_added"][st] and np.array_equal(r["assigned"], g["assigned"][st])
        cur = g["assigned"][st].copy()
        if r["n_added"] + n_in < P["enough"]:
            expect = rr.REJECT_2 if st == 0 else rr.REJECT_3
            break
        if st == 1:
            expect = rr.ACCEPT_3
            break
        p_init, before = rr.tcw_to_se3(R, t), (R, t)
    assert g["verdict"] == expect and np.array_equal(g["final_assigned"], cur)
    # a stage that did not run left zeros, -1 in the assignments
    for st, searched in ((0, len(ran) >= 2), (1, len(ran) == 4)):
        if not searched:
            assert (g["assigned"][st] == -1).all() and not g["excluded_hits"][st].any() and not g["query_accepted"][st].any()
            assert g["n_added"][st] == 0 and g["tlc_z"][st] == 0
    if len(ran) < 3:
        assert g["n_edges"][1] == 0 and g["n_inliers"][1] == 0 and not g["inlier"][1].any() and not g["pose_se3"][1].any() and not g["Tcw"][1].any()
    return ran


def same(a, b):
    return a["verdict"] == b["verdict"] and all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in OUT_KEYS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.VERDICT_SCENES))
def test_every_verdict_stage_by_stage_and_free_running(orc, rig, name):
    s, o = sc.restated(orc, name)
    g = rig.run(s)
    ran = check_stages(orc, s, g)
    assert ran == {"REJECT_1": "o", "ACCEPT_1": "o", "REJECT_2": "os", "ACCEPT_2": "oso", "REJECT_3": "osos", "ACCEPT_3": "osos"}[name]
    assert g["verdict_name"] == name == o["verdict_name"] and np.array_equal(g["final_assigned"], o["final_assigned"])


@pytest.mark.gpu
@pytest.mark.parametrize("n_seed", list(sc.BOUNDARY_SCENES))
def test_boundary_scenes_are_exact(orc, rig, n_seed):
    s, o = sc.restated(orc, n_seed)
    g = rig.run(s)
    check_stages(orc, s, g)
    assert g["verdict_name"] == sc.BOUNDARY_SCENES[n_seed] == o["verdict_name"]
    for k in ("n_edges", "n_inliers", "n_added", "inlier", "assigned", "final_assigned", "excluded_hits", "query_accepted"):
        assert np.array_equal(g[k], o[k]), k


@pytest.mark.gpu
def test_shapes(orc, rig):
    base = sc.build(orc, **sc.VERDICT_SCENES["ACCEPT_2"])
    # no good keyframe point; nothing held
    for change in (dict(good=np.zeros_like(base["good"])), dict(held=np.full(sc.NF, -1, np.int32))):
        s = dict(base, **change)
        g = rig.run(s)
        assert check_stages(orc, s, g) == "o" and g["verdict"] == rr.REJECT_1 and g["n_edges"][0] == 0 and (g["final_assigned"] == -1).all()
        assert np.array_equal(g["pose_se3"][0], rr.tcw_to_se3(s["Rcw"], s["tcw"]))
    # a stored keyframe of one feature, nothing held, no minimum: no edge, and the search runs with one query, which finds its feature
    bits = np.unpackbits(base["kf_desc"] ^ base["desc"][base["src"]], axis=1).sum(1)      # (a query made from a feature of the frame)
    i = int(np.flatnonzero((base["good"] == 1) & ~np.isin(np.arange(len(base["good"])), base["held"]) & (bits <= 12))[0])
    one = dict(base, kf_kps=base["kf_kps"][i:i + 1], kf_desc=base["kf_desc"][i:i + 1], good=np.ones(1, np.uint8), pos=base["pos"][i:i + 1],
               held=np.full(sc.NF, -1, np.int32))
    g = rig.run(one, min_inliers=0)
    assert check_stages(orc, one, g, dict(P, min_inliers=0)) == "os" and g["verdict"] == rr.REJECT_2 and g["query_accepted"].tolist() == [[1], [0]]
    # a mono frame: the same scene without right_u goes the same way, on mono edges
    mono = dict(base, right_u=None)
    g = rig.run(mono)
    assert check_stages(orc, mono, g) == "oso" and g["verdict"] == rr.ACCEPT_2
    # queries on and beyond the image border were searched (the scene has eight)
    border = np.flatnonzero((base["kf_kps"]["x"] < 0) | (base["kf_kps"]["x"] > sc.W) | (base["kf_kps"]["y"] < 0) | (base["kf_kps"]["y"] > sc.H))
    full = rig.run(base)
    assert len(border) >= 4 and check_stages(orc, base, full) == "oso"
    # a second call on the same inputs: bit-identical
    kf = rig.keyframe(base)
    a, b = rig.run(base, kf_id=kf), rig.run(base, kf_id=kf)
    assert same(a, b) and same(a, full)
    # another extraction into the slot, then this frame again: the grid is rebuilt both times
    other, o_other = sc.restated(orc, "ACCEPT_3")
    assert other["image_seed"] != base["image_seed"]
    g = rig.run(other)
    assert g["verdict_name"] == o_other["verdict_name"] and np.array_equal(g["final_assigned"], o_other["final_assigned"])
    assert same(rig.run(base, kf_id=kf), a)
    rig.store.erase([kf])


@pytest.mark.gpu
def test_errors_leave_every_output_untouched(orc, rig):
    from orb_slam2_ros2_amd._lib import Context, OrbfeError
    s, _ = sc.restated(orc, "REJECT_2")
    rig.frame(s)
    kf = rig.keyframe(s)
    n = len(s["good"])

    def fresh():
        return dict(verdict=np.full(1, 0x5A5A5A5A, np.int32), n_edges=np.full(2, 0x5A5A5A5A, np.int32), n_inliers=np.full(2, 0x5A5A5A5A, np.int32),
                    n_added=np.full(2, 0x5A5A5A5A, np.int32), tlc_z=np.full(2, 7.5, np.float32), pose_se3=np.full((2, 7), 7.5),
                    Tcw=np.full((2, 12), 7.5, np.float32), inlier=np.full((2, sc.NF), 0x5A, np.uint8), assigned=np.full((2, sc.NF), 0x5A5A5A5A, np.int32),
                    final_assigned=np.full(sc.NF, 0x5A5A5A5A, np.int32), excluded_hits=np.full((2, sc.NF), 0x5A5A5A5A, np.int32),
                    query_accepted=np.full((2, n), 0x5A, np.uint8))

    def call(ctx, status, kf_id=kf, **change):
        a = dict(s, **change)
        out, ref = fresh(), fresh()
        with pytest.raises(OrbfeError) as ei:
            ctx.reloc_refine_stored(0, rig.store, kf_id, a["good"], a["pos"], a["kf_Rcw"], a["kf_tcw"], a["held"], a["Rcw"], a["tcw"], a["cam"],
                                    a["bounds"], a["sigma2"], a["inv_sigma2"], a["baseline"], right_u=a["right_u"], out=out)
        assert ei.value.status == status
        assert all(np.array_equal(out[k].view(np.uint8), ref[k].view(np.uint8)) for k in out)

    call(rig.ctx, 1, kf_id=kf + 1000)                                                        # an unknown id
    call(rig.ctx, 1, good=s["good"][:-1], pos=s["pos"][:-1], held=np.minimum(s["held"], n - 2))  # n different from the stored count
    bad = s["held"].copy(); bad[5] = n
    call(rig.ctx, 1, held=bad)                                                               # a held out of range
    bad = s["held"].copy(); bad[5] = -2
    call(rig.ctx, 1, held=bad)
    nan = s["Rcw"].copy(); nan[4] = np.nan
    call(rig.ctx, 1, Rcw=nan)                                                                # a pose that is not finite
    inf = s["tcw"].copy(); inf[1] = np.inf
    call(rig.ctx, 1, tcw=inf)
    big = Context(sc.W, sc.H, n_features=2100, max_images=1)                                 # a context of more than 2048 features
    NFb = big.n_features
    call(big, 2, held=np.full(NFb, -1, np.int32), right_u=None)
    big.close()
    import torch
    if torch.cuda.device_count() > 1:                                                        # a context on another device
        far = Context(sc.W, sc.H, n_features=sc.NF, device_id=1, max_images=1)
        call(far, 1)
        far.close()
    # afterwards the same context and store still answer
    g = rig.run(s, kf_id=kf)
    assert g["verdict"] == rr.REJECT_2
    rig.store.erase([kf])


@pytest.mark.gpu
def test_dropin_reloc_refine_equals_the_chain_of_the_bodies(tmp_path):
    """tests/cpp/test_reloc_refine_dropin.cpp: one small map per scenario on stand-in classes, built twice; the chain of the existing bodies
    in Tracking.cc's order on one copy, orbfe::dropin::relocRefine (one device call) on the other: the verdict, the frame's final map
    points, the pose and both counters of every map point.  Four scenarios: accepted at once, accepted after the search and the second
    optimisation, rejected at once, rejected after the search."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "orb_slam2_ros2_amd")
    exe = str(tmp_path / "test_reloc_refine_dropin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(root, "tests", "cpp", "stubs"), "-o", exe,
                           os.path.join(root, "tests", "cpp", "test_reloc_refine_dropin.cpp"), "-L" + pkg, "-lorbfe_hip", "-pthread",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=600)
    L, R = synth.stereo_pair(3)
    L.tofile(tmp_path / "L.raw")
    R.tofile(tmp_path / "R.raw")
    out = subprocess.run([exe, str(tmp_path / "L.raw"), str(tmp_path / "R.raw"), str(sc.W), str(sc.H)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    tag, *rows = out.stdout.split()
    rows = [[int(v) for v in r.split(":")] for r in rows]           # accepted, first inliers, points held at the end, addMatchInTrack calls
    assert tag == "RELOC_OK" and [r[0] for r in rows] == [1, 1, 0, 0]
    assert rows[0][1] >= 50 and 10 <= rows[1][1] < 50 and rows[2][1] < 10 and 10 <= rows[3][1] < 50 and rows[1][2] > 200
