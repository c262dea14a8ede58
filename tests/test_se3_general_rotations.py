"""The SE3 code on general rotations and on every branch of the exp map.

Every other fp64 pose of the suite is a few degrees from the identity (ba_synth.make_problem rotates about y only, within 0.3 rad), so
most product terms of the rotation matrix are exactly zero there, w is never small or negative and the trace of R never <= 0.  Here
the same synthetic problems are moved into worlds X' = R_g X + t_g (se3_reference.gauge), which leaves every measurement where it was
and gives every pose four large quaternion components, and the oracle and the device are compared with 40- to 50-digit mpmath
references that share no spelling with them (se3_reference.mp_edge / mp_oplus).

CPU part: oracle against the reference (edges, exp map), the two optimiser restatements of the oracle through gauge covariance, and the
kernels' own edge model (csrc/ba_edge_dev.h, csrc/se3_dev.h) compiled for the host and run as a stand-alone program.
GPU part: orbfe_debug_se3_oplus, ba_eval_edges, ba_build_system, pose_only_optimize and ba_local_optimize on gauged problems."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import se3_reference as S
from orb_slam2_ros2_amd import ba_synth
from test_local_ba import _pose_dist, _problem
from test_pose_only import _args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_KEYS = ("poses", "points", "edge_pose", "edge_point", "meas", "is_stereo", "info", "huber_delta", "fx", "fy", "cx", "cy", "bf")


def _edge_args(p):
    return {k: p[k] for k in EDGE_KEYS}


def _rel(a, ref):
    """worst |a - ref| / max(1, |ref|)"""
    return float((np.abs(a - ref) / np.maximum(1.0, np.abs(ref))).max())


@pytest.fixture(scope="module")
def gauged():
    """make_problem(seed=5, n_kf=6, n_pt=40) in the four gauged worlds, each with its 40-digit edge reference (computed once)"""
    base = ba_synth.make_problem(seed=5, n_kf=6, n_pt=40)
    out = {}
    for name, g in S.GAUGES.items():
        p = S.gauge(base, *g)
        out[name] = (p, S.mp_edges(p))
    out["_base"] = (base, None)
    return out


@pytest.fixture(scope="module")
def oplus_table():
    """the exp-map case table with its 50-digit reference: poses, updates, reference R and t, branch per case"""
    poses, upd = S.oplus_cases()
    ref = [S.mp_oplus(T, u) for T, u in zip(poses, upd)]
    return poses, upd, np.array([r[0] for r in ref]), np.array([r[1] for r in ref]), [r[2] for r in ref]


def _assert_general(poses, floor=0.01):
    """the premise of every test here: no quaternion component of any pose is small"""
    assert np.abs(np.asarray(poses).reshape(-1, 7)[:, :4]).min() > floor


def _assert_oplus_reach(poses, upd, branches):
    """the case table reaches the series branch, trace > 0, all three largest-diagonal branches, and both signs of the product's w"""
    assert set(branches) == {"series", "tr>0", 0, 1, 2}
    raw_w = np.array([S.quat_mul(S.quat_of(u[:3], np.linalg.norm(u[:3])), T[:4])[3] for T, u in zip(poses, upd)])
    assert (raw_w < -0.01).any() and (raw_w > 0.01).any()        # the w < 0 negation of normalizeRotation is taken, and not taken
    assert (poses[:, 3] < 0).any() and (poses[:, 3] > 0).any()


# ---- CPU: the oracle against the references -----------------------------------------------------------------------------------------
def test_gauge_moves_no_camera_frame_point(orc, gauged):
    """the gauge itself: same errors in every world (to the rounding of the moved vertices: 1e-15 * 6 m * fx / z), other poses"""
    base = gauged["_base"][0]
    e0 = orc.ba_eval_edges(**_edge_args(base))["error"]
    for name in S.GAUGES:
        p = gauged[name][0]
        assert np.abs(orc.ba_eval_edges(**_edge_args(p))["error"] - e0).max() < 1e-9
        assert np.abs(p["poses"][:, :4] - base["poses"][:, :4]).max(1).min() > 0.5 and np.array_equal(p["meas"], base["meas"])


def test_oracle_edges_match_the_40_digit_reference(orc, gauged):
    """Reaches all twelve product terms of quat_to_rot and the qx, qz parts of the quaternion-vector product with non-zero factors:
    asserted through every |q_i| > 0.01; and poses of trace <= 0 with each largest-diagonal index, computed from the quaternions.
    Bounds (issue): 1e-11 absolute on the error, 1e-11 relative on the Jacobians."""
    seen = set()
    for name in S.GAUGES:
        p, ref = gauged[name]
        _assert_general(p["poses"])
        for q in p["poses"][:, :4]:
            tr, i = S.trace_branch(q)
            if tr <= 0:
                seen.add(i)
        o = orc.ba_eval_edges(**_edge_args(p))
        d = (np.abs(o["error"] - ref["error"]).max(), _rel(o["j_point"], ref["j_point"]), _rel(o["j_pose"], ref["j_pose"]))
        print(f"oracle vs reference, {name}: error {d[0]:.2e}  j_point {d[1]:.2e}  j_pose {d[2]:.2e}")
        assert d[0] < 1e-11 and d[1] < 1e-11 and d[2] < 1e-11, (name, d)
        assert np.abs(ref["j_point"]).max() > 10 and (p["is_stereo"] == 0).any() and (p["is_stereo"] == 1).any()
    assert seen == {0, 1, 2}


def test_oracle_edges_are_blind_to_the_quaternion_sign(orc, gauged):
    p = gauged["skew"][0]
    a, b = orc.ba_eval_edges(**_edge_args(p)), orc.ba_eval_edges(**_edge_args(S.negate_q(p)))
    assert (S.negate_q(p)["poses"][:, 3] < 0).all() and (p["poses"][:, 3] > 0).all()
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_oracle_se3_oplus_matches_the_50_digit_reference(orc, oplus_table):
    """orc.se3_oplus on the whole case table (series branch, trace > 0, the three largest-diagonal branches, the w < 0 negation:
    asserted by _assert_oplus_reach), as rotation matrices and translations.  Bound (issue): 1e-11 on both."""
    poses, upd, R_ref, t_ref, branches = oplus_table
    _assert_general(poses)
    _assert_oplus_reach(poses, upd, branches)
    worst = [0.0, 0.0]
    for T, u, R, t in zip(poses, upd, R_ref, t_ref):
        o = orc.se3_oplus(T, u)
        assert abs(np.linalg.norm(o[:4]) - 1) < 1e-15 and o[3] >= 0
        worst = [max(worst[0], np.abs(S.quat_to_R(o[:4]) - R).max()), max(worst[1], np.abs(o[4:] - t).max())]
    print(f"oracle se3_oplus vs reference: R {worst[0]:.2e}  t {worst[1]:.2e}")
    assert worst[0] < 1e-11 and worst[1] < 1e-11, worst


def test_oracle_pose_only_is_gauge_covariant(orc):
    """pose_oracle.cpp's restatement of the exp map and of the pose Jacobians, through its optimiser: the optimisation of a gauged
    problem is the gauge image of the optimisation of the original.  Bounds (issue): pose 1e-9, identical inlier flags."""
    p = ba_synth.make_pose_problem(seed=11, n=300)
    g = S.GAUGES["skew"]
    pg = S.gauge(p, *g)
    _assert_general(pg["pose"])
    n0, pose0, inl0 = orc.pose_only_optimize(**_args(p))
    n1, pose1, inl1 = orc.pose_only_optimize(**_args(pg))
    back = S.ungauge_poses(pose1, *g)
    print(f"gauged pose-only: {n1} inliers, mapped-back pose off by {_pose_dist(back[None], pose0[None]):.2e}")
    assert n0 == n1 and np.array_equal(inl0, inl1) and 200 < n0 < 300
    assert _pose_dist(back[None], pose0[None]) < 1e-9
    assert abs(np.linalg.norm(pose1[:4]) - 1) < 1e-12 and pose1[3] > 0


def test_oracle_local_ba_is_gauge_covariant(orc):
    """lba_oracle.cpp's restatements, through its optimiser: same Levenberg-Marquardt trajectory in the gauged world.  Bounds (issue):
    the same (5, 10) iterations, identical level / bad flags, chi2 to rtol 1e-6."""
    pr, fixed = _problem(3, 12, 400)
    pg = S.gauge(pr, *S.GAUGES["skew"])
    _assert_general(pg["poses"])
    a, b = orc.ba_local_optimize(pr, fixed), orc.ba_local_optimize(pg, fixed)
    print(f"gauged local BA: iterations {tuple(b['iters'])}, chi2 off by {np.abs(a['chi2'] - b['chi2']).max():.2e}")
    assert tuple(a["iters"]) == tuple(b["iters"]) == (5, 10)
    assert np.array_equal(a["level"], b["level"]) and np.array_equal(a["bad"], b["bad"])
    assert np.allclose(a["chi2"], b["chi2"], rtol=1e-6, atol=1e-9)
    back = S.ungauge_poses(b["poses"], *S.GAUGES["skew"])
    assert _pose_dist(back, a["poses"]) < 1e-7


# ---- CPU: the kernels' edge model, compiled by the host compiler ------------------------------------------------------------------------
def _doubles(p):
    """one problem in the layout tests/cpp/test_ba_edge.cpp reads"""
    nk, npt, ne = len(p["poses"]), len(p["points"]), len(p["edge_pose"])
    parts = [[nk, npt, ne], [p[k] for k in ("fx", "fy", "cx", "cy", "bf")]]
    parts += [np.asarray(p[k], np.float64).ravel() for k in ("poses", "points", "edge_pose", "edge_point", "meas", "is_stereo", "info", "huber_delta")]
    return np.concatenate([np.asarray(a, np.float64) for a in parts])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_edge_model_stand_alone(orc, gauged, oplus_table, tmp_path):
    """tests/cpp/test_ba_edge.cpp: ba_edge_dev.h and se3_dev.h have no HIP in them for a host compiler, so the source lines the kernels
    inline run here, under the host compiler's address and undefined-behaviour sanitizers when this g++ has their runtimes (a stand-alone
    program; nothing of it is loaded into python).  Problems: the four gauged worlds, 'skew' with every quaternion negated, 'skew' with
    per-edge Huber widths either side of every chi2; and the exp-map case table.  Bounds (issue): error 1e-11 absolute, j_point / j_pose /
    the pose-only j_pose 1e-11 relative to the 40-digit reference; q and -q the same bits; rho against the oracle at rtol 1e-9, atol 1e-12
    with both Huber branches taken (asserted); pose_oplus 1e-11 on R and t against the 50-digit reference, |q| = 1 within 1e-15, w >= 0.
    The damped 3x3 inverse is checked inside the program."""
    src = os.path.join(ROOT, "tests", "cpp", "test_ba_edge.cpp")
    exe = str(tmp_path / "t")
    base = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "orb_slam2_ros2_amd", "csrc"), "-o", exe, src]
    mode = "address + undefined-behaviour sanitizers"
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        # only a g++ WITHOUT the sanitizers' runtimes (the link step cannot find libasan / libubsan) may run the program plain
        assert re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S* ?: No such file", r.stderr), r.stderr[-3000:]
        mode = "no sanitizer runtime on this machine: plain build"
        subprocess.check_call(base, timeout=300)
    print("test_ba_edge.cpp:", mode)
    names = list(S.GAUGES)
    skew = gauged["skew"][0]
    # Huber widths from the oracle's chi2: half of it (the sqrt branch), twice it plus one (the quadratic branch), none (delta <= 0)
    chi2 = orc.ba_eval_edges(**_edge_args(skew))["chi2"]
    hub = dict(skew)
    hub["huber_delta"] = np.where(np.arange(chi2.size) % 3 == 0, 0.5 * np.sqrt(chi2), np.where(np.arange(chi2.size) % 3 == 1, 2 * np.sqrt(chi2) + 1, -1.0))
    probs = [gauged[n][0] for n in names] + [S.negate_q(skew), hub]
    poses, upd, R_ref, t_ref, branches = oplus_table
    _assert_oplus_reach(poses, upd, branches)
    blob = np.concatenate([[len(probs)]] + [_doubles(p) for p in probs] + [[len(poses)], poses.ravel(), upd.ravel()]).astype("<f8")
    blob.tofile(str(tmp_path / "in.bin"))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout + r.stderr)[-2000:]
    res = np.fromfile(str(tmp_path / "out.bin"), "<f8")
    at, outs = 0, []
    for p in probs:
        ne, o = len(p["edge_pose"]), {}
        for k, shape in (("error", (3,)), ("chi2", ()), ("rho", (2,)), ("j_point", (3, 3)), ("j_pose", (3, 6)), ("pose_j", (3, 6)),
                         ("depth_positive", ()), ("bad", ())):
            n = ne * int(np.prod(shape, dtype=int))
            o[k] = res[at:at + n].reshape((ne,) + shape)
            at += n
        outs.append(o)
    oplus = res[at:].reshape(-1, 7)
    assert oplus.shape == poses.shape
    for name, p, o in zip(names, probs, outs):
        ref = gauged[name][1]
        _assert_general(p["poses"])
        d = (np.abs(o["error"] - ref["error"]).max(), _rel(o["j_point"], ref["j_point"]), _rel(o["j_pose"], ref["j_pose"]), _rel(o["pose_j"], ref["j_pose"]))
        print(f"edge model vs reference, {name}: error {d[0]:.2e}  j_point {d[1]:.2e}  j_pose {d[2]:.2e}  pose-only j_pose {d[3]:.2e}")
        assert all(v < 1e-11 for v in d), (name, d)
        assert (p["is_stereo"] == 0).any() and (p["is_stereo"] == 1).any() and o["depth_positive"].all()
        th = np.where(p["is_stereo"] != 0, 7.815, 5.991)
        assert np.array_equal(o["bad"] != 0, o["chi2"] > th)
    neg, hb = outs[len(names)], outs[len(names) + 1]
    assert (probs[len(names)]["poses"][:, 3] < 0).all() and (skew["poses"][:, 3] > 0).all()
    assert all(np.array_equal(neg[k], outs[names.index("skew")][k]) for k in neg)
    rho = orc.ba_eval_edges(**_edge_args(hub))["rho"]
    d_hub = hub["huber_delta"]
    assert ((hb["rho"][:, 1] < 1) & (d_hub > 0)).any() and ((hb["rho"][:, 1] == 1) & (d_hub > 0)).any() and (d_hub <= 0).any()
    assert np.array_equal(hb["rho"][d_hub <= 0], np.stack([hb["chi2"][d_hub <= 0], np.ones((d_hub <= 0).sum())], 1))
    assert np.allclose(hb["rho"], rho, rtol=1e-9, atol=1e-12)
    dR = max(np.abs(S.quat_to_R(o[:4]) - R).max() for o, R in zip(oplus, R_ref))
    dt = np.abs(oplus[:, 4:] - t_ref).max()
    print(f"host pose_oplus vs reference: R {dR:.2e}  t {dt:.2e}")
    assert dR < 1e-11 and dt < 1e-11
    assert np.abs(np.linalg.norm(oplus[:, :4], axis=1) - 1).max() < 1e-15 and (oplus[:, 3] >= 0).all()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def ctx():
    from orb_slam2_ros2_amd._lib import Context
    c = Context(640, 480, n_features=500, max_images=1)
    yield c
    c.close()


@pytest.mark.gpu
def test_device_se3_oplus_matches_reference_and_oracle(orc, ctx, oplus_table):
    """orbfe_debug_se3_oplus = the device's pose_oplus (se3_dev.h), the whole case table in one call: the theta < 1e-5 series branch,
    trace > 0, the three hand-spelled largest-diagonal branches and the w < 0 negation (asserted by _assert_oplus_reach).
    Bounds (issue): 1e-11 against the 50-digit reference on R and t, 1e-12 against the oracle, |q| = 1 within 1e-15, w >= 0."""
    from orb_slam2_ros2_amd._lib import OrbfeError
    poses, upd, R_ref, t_ref, branches = oplus_table
    _assert_oplus_reach(poses, upd, branches)
    out = ctx.debug_se3_oplus(poses, upd)
    orc_out = np.array([orc.se3_oplus(T, u) for T, u in zip(poses, upd)])
    dR = max(np.abs(S.quat_to_R(o[:4]) - R).max() for o, R in zip(out, R_ref))
    dt = np.abs(out[:, 4:] - t_ref).max()
    d_orc = _pose_dist(out, orc_out)
    print(f"device se3_oplus vs reference: R {dR:.2e}  t {dt:.2e};  vs oracle {d_orc:.2e}")
    assert dR < 1e-11 and dt < 1e-11
    assert d_orc < 1e-12
    assert np.abs(np.linalg.norm(out[:, :4], axis=1) - 1).max() < 1e-15 and (out[:, 3] >= 0).all()
    # one item, 65 items (a second workgroup with one live lane), none; every item is computed alone: same bits as in the table's call
    assert np.array_equal(ctx.debug_se3_oplus(poses[29:30], upd[29:30]), out[29:30])
    idx = np.arange(65) % len(poses)
    assert np.array_equal(ctx.debug_se3_oplus(poses[idx], upd[idx]), out[idx])
    assert ctx.debug_se3_oplus(np.zeros((0, 7)), np.zeros((0, 6))).shape == (0, 7)
    with pytest.raises(OrbfeError) as ei:
        ctx._check(ctx.lib.orbfe_debug_se3_oplus(ctx.h, -1, poses.ctypes.data, upd.ctypes.data, out.ctypes.data))
    assert ei.value.status == 1                                     # ORBFE_EBADARG
    assert ctx.lib.orbfe_debug_se3_oplus(ctx.h, 4, poses.ctypes.data, None, out.ctypes.data) == 1
    assert ctx.lib.orbfe_debug_se3_oplus(None, 4, poses.ctypes.data, upd.ctypes.data, out.ctypes.data) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(S.GAUGES))
def test_device_ba_edges_on_gauged_problems(orc, ctx, gauged, name):
    """k_ba_edges (the edge model of ba_edge_dev.h) with every product term of the rotation matrix non-zero (every |q_i| > 0.01, asserted): against the
    oracle at the tolerances of test_ba_edges_match_oracle, against the 40-digit reference at 1e-11 (issue), and q against -q."""
    p, ref = gauged[name]
    _assert_general(p["poses"])
    out, o = ctx.ba_eval_edges(**_edge_args(p)), orc.ba_eval_edges(**_edge_args(p))
    d = (np.abs(out["error"] - ref["error"]).max(), _rel(out["j_point"], ref["j_point"]), _rel(out["j_pose"], ref["j_pose"]))
    print(f"device vs reference, {name}: error {d[0]:.2e}  j_point {d[1]:.2e}  j_pose {d[2]:.2e}")
    for k in ("error", "chi2", "rho", "j_point", "j_pose"):
        assert out[k].shape == o[k].shape and np.allclose(out[k], o[k], rtol=1e-9, atol=1e-12), k
    assert d[0] < 1e-11 and d[1] < 1e-11 and d[2] < 1e-11, d
    assert np.array_equal(out["depth_positive"], o["depth_positive"]) and out["depth_positive"].all()
    neg = ctx.ba_eval_edges(**_edge_args(S.negate_q(p)))
    assert all(np.array_equal(neg[k], out[k]) for k in out)


@pytest.mark.gpu
def test_device_ba_build_system_on_a_gauged_problem(orc, ctx):
    """k_lm_linpoints / k_lm_poseblocks (k_lm.hip, what orbfe_ba_build_system launches) on general rotations; a free pose with more than
    64 edges and one with fewer (asserted).  Against the oracle at the tolerances of test_ba_normal_equation_blocks_match_oracle,
    and H_ll / H_pp against blocks assembled in numpy from the 40-digit Jacobians and the oracle's rho (issue: rtol 1e-9, atol 1e-7)."""
    p = S.gauge(ba_synth.make_problem(n_kf=6, n_pt=120), *S.GAUGES["skew"])
    _assert_general(p["poses"])
    nk = 6
    fixed = np.zeros(nk, np.uint8)
    fixed[0] = 1
    per_pose = np.bincount(p["edge_pose"], minlength=nk)[1:]
    assert (per_pose > 64).any() and ((per_pose < 64) & (per_pose > 0)).any(), per_pose
    out = ctx.ba_build_system(**_edge_args(p), pose_fixed=fixed)
    ref = orc.ba_build_system(**_edge_args(p), pose_fixed=fixed)
    for k in ("Hpp", "bp", "Hll", "bl", "Hpl"):
        assert np.allclose(out[k], ref[k], rtol=1e-9, atol=1e-12 * np.abs(ref[k]).max()), k
    lean = ctx.ba_build_system(**_edge_args(p), pose_fixed=fixed, want_hpl=False)
    assert "Hpl" not in lean and all(np.array_equal(lean[k], out[k]) for k in lean)
    assert not out["Hpp"][0].any() and all(out["Hpp"][k].any() for k in range(1, nk))
    m = S.mp_edges(p)
    w = orc.ba_eval_edges(**_edge_args(p))["rho"][:, 1] * p["info"]
    Hll, Hpp = np.zeros_like(out["Hll"]), np.zeros_like(out["Hpp"])
    for e in range(w.size):
        A, B = m["j_point"][e], m["j_pose"][e]
        Hll[p["edge_point"][e]] += w[e] * A.T @ A
        if not fixed[p["edge_pose"][e]]:
            Hpp[p["edge_pose"][e]] += w[e] * B.T @ B
    assert np.allclose(out["Hll"], Hll, rtol=1e-9, atol=1e-7) and np.allclose(out["Hpp"], Hpp, rtol=1e-9, atol=1e-7)


def _skew_with_pose_0_fixed(gauged):
    """the 'skew' world (6 keyframes, 40 points, mono and stereo edges: asserted), pose 0 fixed -> problem, stereo mask, fixed flags"""
    p = gauged["skew"][0]
    st = p["is_stereo"] != 0
    assert st.any() and (~st).any()
    fixed = np.zeros(len(p["poses"]), np.uint8)
    fixed[0] = 1
    return p, st, fixed


@pytest.mark.gpu
def test_device_entry_points_share_one_edge_model(ctx, gauged):
    """k_lm_linpoints (ba_build_system) and k_ba_edges (ba_eval_edges) run the same edge arithmetic (ba_edge_dev.h): Hpl(e) = B^T W A of
    the system equals, bit for bit, the block assembled here from ba_eval_edges' Jacobians, rho' and the information in the kernel's own
    order, h = 0; for r < rows: h += (j_pose[e, r, a] * w) * j_point[e, r, c]; and it is zero for the fixed pose's edges."""
    p, st, fixed = _skew_with_pose_0_fixed(gauged)
    ev = ctx.ba_eval_edges(**_edge_args(p))
    Hpl = ctx.ba_build_system(**_edge_args(p), pose_fixed=fixed)["Hpl"]
    w = ev["rho"][:, 1] * p["info"]
    rows = np.where(st, 3, 2)
    ref = np.zeros_like(Hpl)
    for a in range(6):
        for c in range(3):
            h = np.zeros(w.size)
            for r in range(3):
                h = np.where(r < rows, h + (ev["j_pose"][:, r, a] * w) * ev["j_point"][:, r, c], h)
            ref[:, a, c] = h
    of_fixed = fixed[p["edge_pose"]] != 0
    assert of_fixed.any() and (~of_fixed & st).any() and (~of_fixed & ~st).any()
    ref[of_fixed] = 0.0
    off = (Hpl != ref).any((1, 2))
    print(f"Hpl vs blocks from ba_eval_edges: {int(off.sum())} of {w.size} edges differ ({int((off & ~st).sum())} mono), "
          f"worst {np.abs(Hpl - ref).max():.2e}")
    assert np.array_equal(Hpl, ref) and not Hpl[of_fixed].any() and all(Hpl[e].any() for e in np.flatnonzero(~of_fixed))


@pytest.mark.gpu
def test_device_final_report_is_the_edge_evaluation(ctx, gauged):
    """k_lm_final against k_ba_edges: with no iterations the report of ba_local_optimize is ba_eval_edges' chi2 bit for bit, and
    bad == (chi2 > 7.815 / 5.991) | ~depth_positive; the estimates come back untouched."""
    p, st, fixed = _skew_with_pose_0_fixed(gauged)
    ev = ctx.ba_eval_edges(**_edge_args(p))
    g = ctx.ba_local_optimize(p, fixed, 0, 0)
    assert tuple(g["iters"]) == (0, 0)
    assert np.array_equal(g["chi2"], ev["chi2"])
    assert np.array_equal(g["bad"] != 0, (ev["chi2"] > np.where(st, 7.815, 5.991)) | (ev["depth_positive"] == 0))
    assert np.array_equal(g["poses"], p["poses"]) and np.array_equal(g["points"], p["points"])


# (seed, n) as test_device_optimiser_matches_oracle: the 256-thread register kernel up to 1024 edges, the 512-thread one up to 2048, the
# in-memory kernel beyond
@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,kernel,gauge,variant", [
    (10, 40, "reg256", "skew", ""), (9, 257, "reg256", "skew", ""), (13, 1025, "reg512", "skew", ""), (15, 2500, "memory", "skew", ""),
    (9, 257, "reg256", "near_x", ""), (9, 257, "reg256", "skew", "negated"), (9, 257, "reg256", "skew", "mono")])
def test_device_pose_only_on_gauged_problems(orc, ctx, seed, n, kernel, gauge, variant):
    """k_pose_only_reg<256>, <512> and k_pose_only (the kernel follows from n: asserted) with a start pose of four large quaternion
    components (asserted), w < 0 for 'negated'; rightU < 0 everywhere for 'mono'.  Asserts of test_device_optimiser_matches_oracle."""
    assert kernel == ("reg256" if n <= 1024 else "reg512" if n <= 2048 else "memory")
    p = S.gauge(ba_synth.make_pose_problem(seed=seed, n=n), *S.GAUGES[gauge])
    if variant == "negated":
        p = S.negate_q(p)
    a = _args(p)
    if variant == "mono":
        a["meas"] = a["meas"].copy()
        a["meas"][:, 2] = -1.0
    _assert_general(a["pose"])
    assert (a["pose"][3] < 0) == (variant == "negated")
    n_good, pose, inl = ctx.pose_only_optimize(**a)
    r_good, r_pose, r_inl = orc.pose_only_optimize(**a)
    print(f"pose-only n={n} {gauge} {variant}: device vs oracle {np.abs(pose - r_pose).max():.2e}, {n_good} inliers")
    assert np.abs(pose - r_pose).max() < 1e-6
    assert (inl != r_inl).sum() <= 1 and abs(n_good - r_good) <= 1
    assert not inl[p["outlier"]].any()
    assert pose[3] > 0 and abs(np.linalg.norm(pose[:4]) - 1) < 1e-12
    assert np.abs(pose - a["pose"]).max() > 1e-3                      # it moved


def _far_start(pose, start_seed=6):
    """the start pose turned by 0.3 rad about a random axis and moved by 4 m (sigma, per axis)"""
    rng = np.random.default_rng(start_seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    q = S.quat_mul(np.concatenate([np.sin(0.15) * ax, [np.cos(0.15)]]), pose[:4])
    return np.concatenate([q, pose[4:] + rng.normal(size=3) * 4.0])


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,kernel,first", [(10, 40, "reg256", 3), (13, 1025, "reg512", 4), (15, 2100, "memory", 3)])
def test_device_pose_only_rejects_trials(orc, ctx, seed, n, kernel, first):
    """The reject rule of lm_ctrl.h and the table of trial dampings (lm6_trial_lambda, entries q >= 1) where they decide the result, in
    k_pose_only_reg<256> (fewer than 64 edges), k_pose_only_reg<512> and k_pose_only (the kernel follows from n: asserted): the start
    is metres from the optimum (_far_start), so every round -- each restarts from it -- opens with rejected trials and goes on from the
    first accepted one.  The premise comes from the oracle's own counts: the very first iteration takes `first` trial steps, all but
    the last rejected.  Chosen on the CPU, where the oracle's gain ratios of that iteration are -2.63, -1.78, 0.41 (40 edges), -4.32,
    -3.11, -0.036, 1.34 (1025) and -3.32, -2.30, 0.29 (2100), and every later one up to convergence is at least 0.018 from 0: no last
    bit decides one of these trials.  (At the minimum every round ends in rejected trials whose gain ratio is chi2 noise over scale +
    1e-3, as in every pose-only run; neither side moves by them.)  The oracle reaches the pose and the inliers it reaches from the
    near start (asserted), the device the oracle's within the bounds of test_device_pose_only_on_gauged_problems, with the same
    bytes on a second call."""
    assert kernel == ("reg256" if n <= 1024 else "reg512" if n <= 2048 else "memory") and (n < 64) == (seed == 10)
    p = S.gauge(ba_synth.make_pose_problem(seed=seed, n=n), *S.GAUGES["skew"])
    near = _args(p)
    a = dict(near, pose=_far_start(near["pose"]))
    assert np.linalg.norm(a["pose"][4:] - near["pose"][4:]) > 3.0
    r_good, r_pose, r_inl, (iterations, trials, first_iteration) = orc.pose_only_optimize(**a, counts=True)
    assert first_iteration == first and trials > iterations >= 20, (iterations, trials, first_iteration)
    n_good0, pose0, inl0 = orc.pose_only_optimize(**near)
    assert np.abs(r_pose - pose0).max() < 1e-8 and np.array_equal(r_inl, inl0) and r_good == n_good0     # it still converges
    n_good, pose, inl = ctx.pose_only_optimize(**a)
    print(f"pose-only n={n}: {first_iteration} trials in the first iteration, {trials} for {iterations} iterations in the oracle; "
          f"device vs oracle {np.abs(pose - r_pose).max():.2e}")
    assert np.abs(pose - r_pose).max() < 1e-6
    assert (inl != r_inl).sum() <= 1 and abs(n_good - r_good) <= 1
    assert not inl[p["outlier"]].any()
    again = ctx.pose_only_optimize(**a)
    assert again[0] == n_good and again[1].tobytes() == pose.tobytes() and np.array_equal(again[2], inl)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_kf,n_pt,n_fixed,gauge,path", [
    (3, 12, 400, 2, "skew", "registers"), (3, 12, 400, 2, "near_y", "registers"), (14, 48, 2000, 5, "skew", "lmbig"),
    (3, 12, 400, 2, "skew", "host_lm")])
def test_device_local_ba_on_gauged_problems(orc, monkeypatch, seed, n_kf, n_pt, n_fixed, gauge, path):
    """k_lm_linpoints' Jacobians (ba_edge_dev.h) and pose_oplus inside the register-resident Levenberg-Marquardt (k_lm: at most 42 free
    keyframes), the blocked one (k_lmbig: more than 42, asserted) and the host-driven loop (ORBFE_LBA_HOST_LM=1, read at orbfe_create: the
    same builders, k_lba's solve and k_lba_update's pose_oplus), every pose -- the fixed
    ones included -- with four large quaternion components (asserted).  Asserts of test_device_local_ba_matches_oracle."""
    from orb_slam2_ros2_amd._lib import Context
    pr, fixed = _problem(seed, n_kf, n_pt, n_fixed)
    pr = S.gauge(pr, *S.GAUGES[gauge])
    if gauge == "near_y":
        # the half turn of a trajectory: every rotation has trace <= 0 with R[1][1] the largest diagonal element, and w changes sign
        # along the arc (the keyframe next to the crossing has |w| = 0.005, so the floor on the components is lower here)
        _assert_general(pr["poses"], 0.003)
        assert all(S.trace_branch(q)[0] <= 0 and S.trace_branch(q)[1] == 1 for q in pr["poses"][:, :4])
        assert (pr["poses"][:, 3] < 0).any() and (pr["poses"][:, 3] > 0).any()
    else:
        _assert_general(pr["poses"])
    assert ((fixed == 0).sum() > 42) == (path == "lmbig")
    if path == "host_lm":
        monkeypatch.setenv("ORBFE_LBA_HOST_LM", "1")
    c = Context(640, 480, n_features=500, max_images=1)
    g = c.ba_local_optimize(pr, fixed)
    o = orc.ba_local_optimize(pr, fixed)
    print(f"local BA {path} {gauge}: iterations {tuple(g['iters'])}, poses {_pose_dist(g['poses'], o['poses']):.2e}, "
          f"points {np.abs(g['points'] - o['points']).max():.2e}")
    assert tuple(g["iters"]) == tuple(o["iters"])
    assert _pose_dist(g["poses"], o["poses"]) < 1e-7 and np.abs(g["points"] - o["points"]).max() < 1e-7
    assert np.array_equal(g["poses"][:n_fixed], pr["poses"][:n_fixed])
    assert (g["level"] != o["level"]).sum() <= 1 and (g["bad"] != o["bad"]).sum() <= 1
    assert np.allclose(g["chi2"], o["chi2"], rtol=1e-6, atol=1e-9)
    again = c.ba_local_optimize(pr, fixed)
    assert all(np.array_equal(again[k], g[k]) for k in ("poses", "points", "level", "chi2", "bad"))
    c.close()
