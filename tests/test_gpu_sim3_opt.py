"""orbfe_sim3_optimize and orbfe_debug_sim3_edges on the device against tests/sim3_opt_restatement.py (rules O1 .. O8 of DESIGN 4.22).

Bounds.  The edge probe: bit for bit -- errors, chi2 and the numeric Jacobians are + - x / sqrt only, correctly rounded on both sides.  The
optimiser: every entry of the estimate within 1e-6 of the restatement (the project's bound for a one-vertex optimiser against its fp64
restatement, tests/test_pose_only.py: the device differs by the order of its sums, its reciprocal-square-root 6x6 solve and sin / cos
ulps); flags and count equal exactly, which the seed qualification of tests/test_sim3_opt_host.py allows; the model the float cast of
the estimate.  Measured on an MI355X: see DESIGN 4.22."""
import ctypes

import numpy as np
import pytest

import sim3_opt_cases as K
import sim3_opt_restatement as R
import sim3_restatement as S

pytestmark = pytest.mark.gpu
EBADARG = 1


@pytest.fixture(scope="module")
def ctx():
    from orb_slam2_ros2_amd._lib import Context
    c = Context(640, 480, n_features=500, max_images=1)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_or_same_class(got, want, what):
    """finite values equal bit for bit; NaN where NaN, +inf where +inf, -inf where -inf"""
    got, want = np.asarray(got), np.asarray(want)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want)), what
    bad = np.nonzero(_bits(got)[fin] != _bits(want)[fin])[0]
    assert bad.size == 0, f"{what}: {bad.size} entries differ, first {got[fin][bad[0]]!r} vs {want[fin][bad[0]]!r}"


def test_debug_edges_equal_the_restatement_bit_for_bit(ctx):
    p = K.problem(11, 200, 20)
    P = R.Problem(*K.args(p)[:7])
    est0 = R.sim3_from_model(p["model"])
    final = tuple(K.reference(11, 200, 20)["est"])
    # a quarter turn about y after the start estimate: the pairs on one side of the axis end up behind the camera, and the translation
    # puts pair 0's mapped point exactly on z = 0 (r_z + (-r_z)): its first edge's error is +-inf or NaN
    h = float(np.sqrt(0.5))
    turn = R.sim3_mul((0.0, h, 0.0, h, 0.0, 0.0, 0.0, 1.0), est0)
    rz = float(R.quat_rotate(turn[:4], (P.Pm[0][:1], P.Pm[1][:1], P.Pm[2][:1]))[2][0])
    turn = turn[:6] + (-rz, 1.0)
    saw_behind = False
    for name, est in (("start", est0), ("final", final), ("turned", turn)):
        err, chi2, jac = ctx.debug_sim3_edges(*K.args(p)[:7], est)
        E = R.edge_errors(P, est)
        _same_or_same_class(err, E, f"errors at the {name} estimate")
        _same_or_same_class(chi2, R.edge_chi2(P, E), f"chi2 at the {name} estimate")
        _same_or_same_class(jac.reshape(-1, 4, 6), R.numeric_jacobian(P, est), f"Jacobians at the {name} estimate")
        if name == "turned":
            z = np.asarray(R.sim3_map(est, P.Pm)[2])
            saw_behind = z[0] == 0 and bool((z < 0).any()) and not np.isfinite(E[0, :2]).any()
    assert saw_behind


@pytest.mark.parametrize("seed, n, n_out", K.GPU_CASES, ids=[f"n{n}-out{o}" for _, n, o in K.GPU_CASES])
def test_optimiser_matches_the_restatement(ctx, seed, n, n_out):
    p = K.problem(seed, n, n_out)
    r = K.reference(seed, n, n_out)
    n_inl, model, flags, est = ctx.sim3_optimize(*K.args(p))
    d = float(np.abs(est - r["est"]).max())
    print(f"n {n}, {n_out} outliers, branch {r['branch']}: |est - restatement| max {d:.3e}; {n_inl} inliers")
    assert d < 1e-6
    assert n_inl == r["n_inliers"] and np.array_equal(flags, r["flags"].astype(bool))
    if r["branch"] in ("short", "few"):   # the early return: nothing moves
        assert n_inl == 0 and flags.all() and np.array_equal(model.view(np.uint32), p["model"].view(np.uint32))
    else:
        assert np.array_equal(model.view(np.uint32), R.sim3_to_model(tuple(est)).view(np.uint32))      # O2 on the device's own estimate
        assert np.abs(model - r["model"]).max() < 1e-6


def test_rejected_trials_at_twenty_four_pairs(ctx):
    """k_sim3_optimize's reject rule (lm_ctrl.h) on the smallest problem that goes through both rounds: 24 pairs, 2 of them outliers.
    The premise comes from the restatement alone: 30 trials for 14 iterations.  What it rejects are the trials at the minimum, whose
    gain ratio is chi2 noise over scale + 1e-3; no start model found makes it reject an earlier one and still leave 20 pairs after the
    first round (within 0.8 rad and 2.5 m of the optimum, and 96 starts turned by 0.3 to 0.6 rad and moved by 1 to 4 m per axis, at 24
    and 60 pairs: profiles/NOTES_r8.md).  So a last bit may decide such a trial, and neither side moves by it: the bound stays the
    neighbouring test's 1e-6 -- and a reject rule that computed a wrong lambda would pass here; the rule itself is held bit for bit by
    tests/test_lm_ctrl.py, and in this kernel's twin by test_device_pose_only_rejects_trials.  The same bytes on a second call."""
    case = (11, 24, 2)
    p, r = K.problem(*case), K.reference(*case)
    assert r["branch"] == "ten" and r["trials"] > r["iterations"] >= 6
    n_inl, model, flags, est = ctx.sim3_optimize(*K.args(p))
    d = float(np.abs(est - r["est"]).max())
    print(f"24 pairs: {r['trials']} trials for {r['iterations']} iterations in the restatement; |est - restatement| max {d:.3e}")
    assert d < 1e-6
    assert n_inl == r["n_inliers"] and np.array_equal(flags, r["flags"].astype(bool))
    assert np.array_equal(model.view(np.uint32), R.sim3_to_model(tuple(est)).view(np.uint32))
    again = ctx.sim3_optimize(*K.args(p))
    assert again[0] == n_inl and all(x.tobytes() == y.tobytes() for x, y in zip(again[1:], (model, flags, est)))


def test_early_return_touches_nothing(ctx):
    """fewer than 20 pairs left after the first round: the model's bytes stay, n_inliers is 0, every flag is 1 -- through the C call
    itself, with the outputs pre-filled"""
    from orb_slam2_ros2_amd import _lib
    for case in ((11, 25, 6), (11, 19, 0)):
        p = K.problem(*case)
        n, arrs = _lib.Context._sim3_pairs(*K.args(p)[:6])
        model = p["model"].copy()
        flags, ni = np.full(n, 7, np.uint8), ctypes.c_int32(-5)
        st = ctx.lib.orbfe_sim3_optimize(ctx.h, n, *(_lib.ptr(a) for a in arrs), *p["cam"], _lib.ptr(model), _lib.ptr(flags), ctypes.byref(ni), None)
        assert st == 0 and ni.value == 0 and (flags == 1).all() and model.tobytes() == p["model"].tobytes(), case


def test_same_call_twice_same_bytes(ctx):
    for case in ((11, 200, 20), (11, 600, 60)):
        a = ctx.sim3_optimize(*K.args(K.problem(*case)))
        b = ctx.sim3_optimize(*K.args(K.problem(*case)))
        assert a[0] == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:])), case
    p = K.problem(11, 200, 20)
    est = K.reference(11, 200, 20)["est"]
    a, b = ctx.debug_sim3_edges(*K.args(p)[:7], est), ctx.debug_sim3_edges(*K.args(p)[:7], est)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_chains_from_the_ransac_solver(ctx):
    """a Sim3Set on one of tests/sim3_restatement.py's scenes gives a model through orbfe_sim3_iterate; it goes straight into
    orbfe_sim3_optimize with the solver's own camera-frame points and projections, and the restatement gets the same result"""
    from orb_slam2_ros2_amd._lib import Sim3Set, sim3_engine
    sc = S.scene(np.random.default_rng(77), 150, outlier=0.1, noise=0.5)
    ref = S.Solver(*sc)
    off = np.array([0, 150], np.int64)
    sim3_engine(1)
    dev = Sim3Set(off, *sc, S.SIGMA2, S.CAM)
    ret, _, model, inl = dev.iterate(0, 100)
    dev.close()
    assert ret and model is not None and len(inl) >= 20
    # model = Rqp, tqp maps p's frame into q's: q plays pCurr (c), p plays pMatch (m)
    inv2 = lambda o: ((np.float32(1) / np.sqrt(np.asarray(S.SIGMA2, np.float32)[o])) ** 2).astype(np.float64)
    a = (ref.Q3[inl], ref.P3[inl], ref.Q2[inl], ref.P2[inl], inv2(sc[3][inl]), inv2(sc[2][inl]), ref.cam, model)
    r = R.optimize_sim3(*a)
    n_inl, m2, flags, est = ctx.sim3_optimize(*a)
    assert r["branch"] in ("five", "ten") and r["n_inliers"] >= 20
    assert n_inl == r["n_inliers"] and np.array_equal(flags, r["flags"].astype(bool)) and np.abs(est - r["est"]).max() < 1e-6
    assert np.array_equal(m2.view(np.uint32), R.sim3_to_model(tuple(est)).view(np.uint32))


def test_refusals_launch_nothing(ctx):
    from orb_slam2_ros2_amd import _lib
    p = K.problem(11, 25, 5)
    n, arrs = _lib.Context._sim3_pairs(*K.args(p)[:6])
    ptrs = [_lib.ptr(a) for a in arrs]
    flags, ni, est = np.full(n, 7, np.uint8), ctypes.c_int32(-5), np.zeros(8)
    call = ctx.lib.orbfe_sim3_optimize
    model = p["model"].copy()
    assert call(ctx.h, -1, *ptrs, *p["cam"], _lib.ptr(model), _lib.ptr(flags), ctypes.byref(ni), _lib.ptr(est)) == EBADARG
    assert call(ctx.h, n, *ptrs, *p["cam"], None, _lib.ptr(flags), ctypes.byref(ni), _lib.ptr(est)) == EBADARG
    for bad in (np.nan, np.inf):
        model = p["model"].copy()
        model[4] = bad
        keep = model.tobytes()
        assert call(ctx.h, n, *ptrs, *p["cam"], _lib.ptr(model), _lib.ptr(flags), ctypes.byref(ni), _lib.ptr(est)) == EBADARG
        assert model.tobytes() == keep
    assert ni.value == -5 and (flags == 7).all() and not est.any()                                     # no output was written
    err, chi, jac = np.zeros((n, 4)), np.zeros((n, 2)), np.zeros((n, 24))
    dbg = ctx.lib.orbfe_debug_sim3_edges
    assert dbg(ctx.h, -1, *ptrs, *p["cam"], _lib.ptr(est), _lib.ptr(err), _lib.ptr(chi), _lib.ptr(jac)) == EBADARG
    assert dbg(ctx.h, n, *ptrs, *p["cam"], None, _lib.ptr(err), _lib.ptr(chi), _lib.ptr(jac)) == EBADARG
    assert dbg(ctx.h, n, *ptrs, *p["cam"], _lib.ptr(est), _lib.ptr(err), _lib.ptr(chi), None) == EBADARG
    assert not err.any() and not chi.any() and not jac.any()
    # and the context still works
    assert ctx.sim3_optimize(*K.args(p))[0] == K.reference(11, 25, 5)["n_inliers"]


def test_dropin_over_minimal_types(ctx, tmp_path):
    """tests/cpp/test_sim3opt_dropin.cpp: dropin::OptimizeSim3 as the whole body of the reference function over stand-in classes -- the
    vbIsInlier filter (null, bad and not-in-map points; the second test asks the CURRENT point's isInMap again, so a matched point that
    is not in the map stays), cPc = Rcw cPw + tcw in float, the information from the octaves, the list and the model written back, the
    untouched early return, bFixedScale == false refused -- against the Python binding on the same arrays."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(9)
    cases, lines = [], []
    for n, n_out in ((120, 12), (25, 6)):
        p = K.problem(11, n, n_out)
        Rc, tc, Rm, tm = S.rot(rng), rng.normal(size=3), S.rot(rng), rng.normal(size=3)
        cPw = ((p["pc"].astype(float) - tc) @ Rc).astype(np.float32)
        mPw = ((p["pm"].astype(float) - tm) @ Rm).astype(np.float32)
        pose = lambda Rr, t: np.concatenate([Rr.reshape(9), t]).astype(np.float32)
        pose_c, pose_m = pose(Rc, tc), pose(Rm, tm)
        oc, om = rng.integers(0, 8, n), rng.integers(0, 8, n)
        cs, ms = np.zeros(n, int), np.zeros(n, int)
        if n > 100:
            cs[[3, 40, 77]] = [1, 2, 3]          # the current point null / bad / not in the map: the pair leaves
            ms[[5, 41, 90]] = [1, 2, 3]          # the matched point null / bad: the pair leaves; not in the map: it STAYS (:504)
        keep = (cs == 0) & (ms != 1) & (ms != 2)
        cases.append((pose_c, pose_m, p["model"], cPw, mPw, p["uv_c"], oc, p["uv_m"], om, cs, ms))
        inv2 = lambda o: np.array([np.float32(1) / np.float32(np.power(1.2, 2 * int(l))) for l in o], np.float32).astype(np.float64)
        pc = S.affine(1.0, pose_c[None, :9], cPw, pose_c[None, 9:]).reshape(-1, 3)
        pm = S.affine(1.0, pose_m[None, :9], mPw, pose_m[None, 9:]).reshape(-1, 3)
        n_inl, model, flags, _ = ctx.sim3_optimize(pc[keep], pm[keep], p["uv_c"][keep], p["uv_m"][keep], inv2(oc[keep]), inv2(om[keep]),
                                                   p["cam"], p["model"])
        early = n_inl == 0 and flags.all()
        kept = np.arange(n) if early else np.nonzero(keep)[0][flags]
        assert early == (n == 25) and (early or 50 < n_inl < keep.sum())
        lines.append(f"{n_inl} |" + "".join(f" {i}" for i in kept) + " |" + "".join(f" {int(v):08x}" for v in model.view(np.uint32)) + " 3f800000")
    inp = tmp_path / "in.txt"
    with open(inp, "w") as f:
        f.write(f"{len(cases)}\n")
        for pose_c, pose_m, model, cPw, mPw, uvc, oc, uvm, om, cs, ms in cases:
            for v in (pose_c, pose_m, model):
                f.write(" ".join(repr(float(x)) for x in v) + "\n")
            f.write(f"{len(cPw)}\n")
            for i in range(len(cPw)):
                f.write(" ".join(repr(float(x)) for x in (*cPw[i], *mPw[i])) + f" {float(uvc[i, 0])!r} {float(uvc[i, 1])!r} {int(oc[i])}"
                        f" {float(uvm[i, 0])!r} {float(uvm[i, 1])!r} {int(om[i])} {int(cs[i])} {int(ms[i])}\n")
    pkg = os.path.join(root, "orb_slam2_ros2_amd")
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(root, "tests", "cpp", "stubs"), "-I" + os.path.join(pkg, "host"),
                           "-I" + os.path.join(root, "include"), "-o", exe, os.path.join(root, "tests", "cpp", "test_sim3opt_dropin.cpp"), "-L" + pkg,
                           "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines() == lines + ["fixed-scale only: ok"]
