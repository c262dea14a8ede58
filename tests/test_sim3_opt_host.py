"""Optimizer::OptimizeSim3 without a GPU: the restatement (tests/sim3_opt_restatement.py, rules O1 .. O8 of DESIGN 4.22) on known
answers and on the 20-pair rule, the qualification of every problem the GPU tests use, the edge model header run by the host compiler
against the restatement bit for bit, the entry points' surface and refusals, and the drop-in against the reference's headers."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import sim3_opt_cases as K
import sim3_opt_restatement as R
from orb_slam2_ros2_amd import ba_synth

from test_sim3_host import NEEDS_REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. known answers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, n_out", [(200, 20), (600, 60), (64, 6)])
def test_restatement_recovers_the_pose_and_rejects_the_outliers(n, n_out):
    p = K.problem(11, n, n_out)
    r = K.reference(11, n, n_out)
    Rm, tm = r["model"][:9].reshape(3, 3).astype(float), r["model"][9:].astype(float)
    start = K.rot_angle(p["model"][:9].reshape(3, 3), p["truth_R"])
    assert start > math.radians(1.5) and np.abs(p["model"][9:] - p["truth_t"]).max() > 0.03          # the start is off by degrees / centimetres
    # noise of 0.5 px at octave 0 on ~n edges at 3 .. 12 m, focal length 520: well under a milliradian and a centimetre
    assert K.rot_angle(Rm, p["truth_R"]) < 1e-3 and np.abs(tm - p["truth_t"]).max() < 1e-2
    flags = r["flags"].astype(bool)
    assert not (flags & p["outlier"]).any()                                                            # every gross outlier is gone
    assert flags[~p["outlier"]].mean() > 0.98 and r["n_inliers"] == int(flags.sum())
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 4 * np.finfo(np.float32).eps and abs(np.linalg.det(Rm) - 1) < 1e-6
    assert r["branch"] == "ten" and r["est"][7] == 1.0 and r["est"][3] > 0


def test_the_20_pair_rule():
    p = K.problem(11, 25, 6)
    r = K.reference(11, 25, 6)
    assert r["branch"] == "few" and r["n_bad"] == 6 and r["n_inliers"] == 0
    assert np.array_equal(r["model"].view(np.uint32), p["model"].view(np.uint32)) and r["flags"].all()
    r = K.reference(11, 25, 5)
    assert r["branch"] == "ten" and r["n_bad"] == 5 and r["n_inliers"] == 20 and not (r["flags"].astype(bool) & K.problem(11, 25, 5)["outlier"]).any()
    r = K.reference(11, 30, 0)
    assert r["branch"] == "five" and r["n_bad"] == 0 and r["n_inliers"] == 30
    for n in (19, 0):
        p = K.problem(11, n, 0)
        r = K.reference(11, n, 0)
        assert r["branch"] == "short" and r["n_inliers"] == 0 and r["flags"].all() and len(r["flags"]) == n
        assert np.array_equal(r["model"].view(np.uint32), p["model"].view(np.uint32))


# ---- 2. the problems of the GPU tests ------------------------------------------------------------------------------------------------
def test_gpu_cases_are_qualified():
    """No chi2 within 1e-6 relative of 9.210 where the driver classifies (so the device must give equal flags), and the restatement with
    its edge sums in reversed order agrees with itself to 1e-7 in every entry of the estimate (so summation order is immaterial)."""
    worst_gap, worst_order = np.inf, 0.0
    for case in K.GPU_CASES:
        r = K.reference(*case)
        for chi in (r["chi2_a"], r["chi2_b"]):
            if chi is not None:
                c = chi[np.isfinite(chi)]
                if c.size:
                    worst_gap = min(worst_gap, float(np.abs(c / R.TH - 1).min()))
        rr = K.reference(*case, reverse=True)
        assert rr["branch"] == r["branch"] and np.array_equal(rr["flags"], r["flags"]), case
        d = float(np.abs(rr["est"] - r["est"]).max())
        worst_order = max(worst_order, d)
        assert d < 1e-7, (case, d)
    print(f"closest chi2 to the threshold: {worst_gap:.3e} relative; largest change of the estimate under reversed summation: {worst_order:.3e}")
    assert worst_gap > 1e-6
    branches = {K.reference(*c)["branch"] for c in K.GPU_CASES}
    assert branches == {"short", "few", "ten", "five"}


# ---- 3. the header, by the host compiler ---------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_sim3_edge_model_stand_alone(tmp_path):
    """tests/cpp/test_sim3_edge.cpp: sim3_edge_dev.h has no HIP in it for a host compiler, so the source lines the kernel inlines run
    here under the address and undefined-behaviour sanitizers (a stand-alone program; nothing of it is loaded into python).  Errors,
    chi2, Huber (both branches), inverse, product, exp (both theta branches and theta = 0) and the numeric Jacobians equal the
    restatement bit for bit: only + - x / sqrt are involved.  exp past the small-angle branch goes through sin / cos: 1e-15."""
    src = os.path.join(ROOT, "tests", "cpp", "test_sim3_edge.cpp")
    exe = str(tmp_path / "t")
    base = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "orb_slam2_ros2_amd", "csrc"), "-o", exe, src]
    mode = "address + undefined-behaviour sanitizers"
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        # only a g++ WITHOUT the sanitizers' runtimes (the link step cannot find libasan / libubsan) may run the program plain
        assert re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S* ?: No such file", r.stderr), r.stderr[-3000:]
        mode = "no sanitizer runtime on this machine: plain build"
        subprocess.check_call(base, timeout=300)
    print("test_sim3_edge.cpp:", mode)
    n = 48
    p = K.problem(11, n, 6)
    P = R.Problem(*K.args(p)[:7])
    est0 = R.sim3_from_model(p["model"])
    est1 = tuple(K.reference(11, 200, 20)["est"])
    behind = R.sim3_mul((0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 5.0, 1.0), est0)       # half a turn about y: most points land behind the camera
    general = R.sim3_mul(R.sim3_exp([0.7, -1.9, 0.4, 0.1, 0.2, -0.3]), est0)   # a large rotation (q.w small), s kept at 1
    scaled = est0[:7] + (1.25,)                                               # s != 1: map, inverse and product carry the scale
    ests = [est0, est1, behind, general, scaled]
    pairs = np.concatenate([np.stack(P.Pc, 1), np.stack(P.Pm, 1), P.uvc, P.uvm, P.wc[:, None], P.wm[:, None]], 1)
    chi = np.array([0.0, 1e-12, 3.0, 9.2, 9.21, 9.3, 250.0, 1e9, R.DELTA * R.DELTA, np.nextafter(R.DELTA * R.DELTA, 10.0)])
    dlt = np.full(chi.size, R.DELTA)
    small = [[0.0] * 6] + [[(s * 1e-9 if k == d else 0.0) for k in range(6)] for d in range(6) for s in (1, -1)] + \
            [[3e-6, -4e-6, 5e-6, 0.1, -0.2, 0.3], [9.9e-6, 0, 0, 1, 2, 3], [0, 0, 0, 0.5, -0.25, 2.0]]
    large = [[1.1e-5, 0, 0, 1, 2, 3], [0.01, -0.02, 0.03, 0.1, 0.2, 0.3], [0.3, 0.4, -1.2, -0.5, 0.7, 0.2], [2.0, -2.0, 1.0, 0.1, 0.0, -0.1],
             [3.1, 0.0, 0.0, 0.2, 0.2, 0.2], [0.0, 3.14159, 0.0, 0.3, -0.3, 0.3], [0.0, 0.0, -3.0, 1.0, 1.0, 1.0]]
    upd = small + large
    A = [est0, general, scaled, R.sim3_exp(large[2]), behind]
    B = [est1, scaled, general, est0, R.sim3_inverse(est0)]
    rng = np.random.default_rng(5)
    models = [p["model"].astype(np.float64)]
    for w in ([0.1, 0.2, 0.3], [3.0, 0.1, 0.0], [0.1, 3.0, 0.2], [0.0, 0.2, 3.1], [2.2, 2.2, 0.0]):     # the trace branch and all three others
        Rw = ba_synth._rot_from_rotvec(w)
        models.append(np.concatenate([Rw.reshape(9), rng.normal(size=3)]).astype(np.float32).astype(np.float64))
    blob = np.concatenate([[P.fx, P.fy, P.cx, P.cy], [len(ests)], np.ravel(ests), [n], pairs.ravel(), [chi.size], chi, dlt, [len(upd)],
                           np.ravel(upd), [len(A)], np.ravel(A), np.ravel(B), [len(models)], np.ravel(models)]).astype("<f8")
    blob.tofile(str(tmp_path / "in.bin"))
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout + r.stderr)[-2000:]
    res = np.fromfile(str(tmp_path / "out.bin"), "<f8")
    at = 0

    def take(*shape):
        nonlocal at
        k = int(np.prod(shape, dtype=int))
        out = res[at:at + k].reshape(shape)
        at += k
        return out
    saw_nonfinite = False
    for k, S in enumerate(ests):
        assert np.array_equal(_bits(take(8)), _bits(R.sim3_inverse(S))), f"inverse of estimate {k}"
        got = take(n, 30)
        E = R.edge_errors(P, S)
        C = R.edge_chi2(P, E)
        J = R.numeric_jacobian(P, S)
        saw_nonfinite |= not np.isfinite(J).all()
        for name, g, w in (("error", got[:, :4], E), ("chi2", got[:, 4:6], C), ("jacobian", got[:, 6:], J.reshape(n, 24))):
            fin = np.isfinite(w)
            assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(_bits(g)[fin], _bits(w)[fin]), f"{name} at estimate {k}"
        if k < 2:
            assert np.abs(J).max() > 10 and np.isfinite(J).all()
    hub = take(chi.size, 2)
    rho, drho = R.huber(chi)
    assert np.array_equal(_bits(hub[:, 0]), _bits(rho)) and np.array_equal(_bits(hub[:, 1]), _bits(drho))
    assert (drho == 1.0).sum() >= 5 and (drho < 1.0).sum() >= 4                                        # both branches
    exps = take(len(upd), 8)
    ops = take(len(upd), 8)
    for i, u in enumerate(upd):
        e, o = np.array(R.sim3_exp(u)), np.array(R.sim3_oplus(est0, u))
        if i < len(small):
            assert np.array_equal(_bits(exps[i]), _bits(e)) and np.array_equal(_bits(ops[i]), _bits(o)), f"exp / oplus of update {i}"
        else:
            assert np.allclose(exps[i], e, rtol=1e-15, atol=1e-15) and np.allclose(ops[i], o, rtol=1e-15, atol=1e-15), f"exp / oplus of update {i}"
    assert np.array_equal(exps[0], [0, 0, 0, 1, 0, 0, 0, 1])                                           # theta = 0
    muls = take(len(A), 8)
    for i in range(len(A)):
        assert np.array_equal(_bits(muls[i]), _bits(R.sim3_mul(A[i], B[i]))), f"product {i}"
    for i, m in enumerate(models):
        S = R.sim3_from_model(m)
        assert np.array_equal(_bits(take(8)), _bits(S)), f"from_model {i}"
        assert np.array_equal(take(12).astype(np.float32).view(np.uint32), R.sim3_to_model(S).view(np.uint32)), f"to_model {i}"
    assert at == res.size


# ---- 4. surface ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from orb_slam2_ros2_amd import _lib, Optimizer
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)                       # loading must not need a GPU
    for name in ("orbfe_sim3_optimize", "orbfe_debug_sim3_edges"):
        assert re.search(r"\borbfe_status\s+" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert "Optimizer.cc:464-619" in hdr
    assert callable(Optimizer.OptimizeSim3) and callable(_lib.Context.sim3_optimize) and callable(_lib.Context.debug_sim3_edges)


def test_refusals_need_no_context():
    """the argument checks come first: without a context every call is ORBFE_EBADARG, whatever else it carries"""
    from orb_slam2_ros2_amd import _lib
    lib = _lib.load()
    p = K.problem(11, 25, 5)
    n, arrs = _lib.Context._sim3_pairs(*K.args(p)[:6])
    model = p["model"].copy()
    flags, ni, est = np.zeros(n, np.uint8), ctypes.c_int32(7), np.zeros(8)
    st = lib.orbfe_sim3_optimize(None, n, *(_lib.ptr(a) for a in arrs), *p["cam"], _lib.ptr(model), _lib.ptr(flags), ctypes.byref(ni), _lib.ptr(est))
    assert st == 1 and ni.value == 7 and np.array_equal(model, p["model"])
    err, chi, jac = np.zeros((n, 4)), np.zeros((n, 2)), np.zeros((n, 24))
    st = lib.orbfe_debug_sim3_edges(None, n, *(_lib.ptr(a) for a in arrs), *p["cam"], _lib.ptr(est), _lib.ptr(err), _lib.ptr(chi), _lib.ptr(jac))
    assert st == 1


def test_synthetic_problem_is_what_it_says():
    p = ba_synth.make_sim3_problem(3, 120, 13, 0.5)
    assert p["outlier"].sum() == 13 and p["pc"].dtype == np.float32 and p["uv_m"].shape == (120, 2) and p["info_c"].dtype == np.float64
    assert (p["pc"][:, 2] > 1).all() and (p["pm"][:, 2] > 1).all()                                    # in front of both cameras
    assert len(np.unique(p["info_c"])) > 3 and len(np.unique(p["info_m"])) > 3                        # octave-dependent information
    P = R.Problem(*K.args(p)[:7])
    truth = np.concatenate([p["truth_R"].reshape(9), p["truth_t"]]).astype(np.float32)
    E = R.edge_errors(P, R.sim3_from_model(truth))
    big = np.abs(E).max(1) > 20
    assert np.array_equal(big, p["outlier"])                                                          # tens of pixels, and only there
    assert (np.abs(E[p["outlier"]][:, :2]).max(1) > 20).any() and (np.abs(E[p["outlier"]][:, 2:]).max(1) > 20).any()
    q = ba_synth.make_sim3_problem(3, 120, 13, 0.5)
    assert all(np.array_equal(p[k], q[k]) for k in p if isinstance(p[k], np.ndarray))                # deterministic


# ---- 5. the drop-in against the reference's classes ----------------------------------------------------------------------------------
@NEEDS_REF
def test_dropin_and_the_computeSim3_body_compile_against_the_reference_classes(tmp_path):
    """g++ -fsyntax-only of tests/cpp/ref_sim3opt_body.cpp: dropin::OptimizeSim3 as the body of Optimizer::OptimizeSim3 and the
    computeSim3 loop of INTEGRATION section 15, with the reference's Optimizer.h / LoopClosing.h / KeyFrame.h / MapPoint.h / Camera.h"""
    from test_reference_compile import _include_dir
    inc = _include_dir(str(tmp_path / "inc"), friend_line=True)
    stubs = os.path.join(ROOT, "tests", "cpp", "stubs")
    host = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + inc, "-I" + stubs, "-I" + os.path.join(stubs, "refgen"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "cpp", "ref_sim3opt_body.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
