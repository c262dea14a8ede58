"""Optimizer::optimizeEssentialGraph without a GPU: the edge model header (csrc/posegraph_edge_dev.h) against the restatement
(tests/essential_graph_restatement.py, rules G1 .. G8 of DESIGN 4.24) in a stand-alone program under the host sanitizers, the
restatement's own properties, the qualification of the GPU cases (tests/essential_graph_cases.py), and the entry points' argument checks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import essential_graph_cases as K
import essential_graph_restatement as R
import sim3_opt_restatement as s3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = 1 - 1e-5


def _log_d(S):
    Rm = s3.quat_to_rot(S[:4])
    return 0.5 * (Rm[0] + Rm[4] + Rm[8] - 1)


def edge_d(g, est):
    """d of Sim3::log (G4) of every edge at the estimates: which side of the switch its base evaluation takes"""
    G = R.Graph(est, g["fixed"], g["edges"], g["meas"])
    S = R.cols(est)
    return _log_d(s3.sim3_mul(s3.sim3_mul(G.C, R.take(S, G.v0)), s3.sim3_inverse(R.take(S, G.v1))))


def _build_program(tmp_path, name):
    src = os.path.join(ROOT, "tests", "cpp", name)
    exe = str(tmp_path / "t")
    base = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "orb_slam2_ros2_amd", "csrc"), "-o", exe, src]
    mode = "address + undefined-behaviour sanitizers"
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        # only a g++ WITHOUT the sanitizers' runtimes (the link step cannot find libasan / libubsan) may run the program plain
        assert re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S* ?: No such file", r.stderr), r.stderr[-3000:]
        mode = "no sanitizer runtime on this machine: plain build"
        subprocess.check_call(base, timeout=300)
    print(name + ":", mode)
    return exe


def test_edge_model_stand_alone(tmp_path):
    """tests/cpp/test_posegraph_edge.cpp: posegraph_edge_dev.h has no HIP in it for a host compiler, so the source lines the kernels
    inline run here under the address and undefined-behaviour sanitizers (a stand-alone program; nothing of it is loaded into python).
    58 edges of a realistic graph at its start estimates, on both sides of Sim3::log's switch.  Where the 25 evaluations of an edge stay
    on the small-angle side only + - x / sqrt are involved: errors, chi2 and both Jacobians equal the restatement bit for bit.  Past the
    switch they go through acos / sin / cos: errors within 1e-15 (DESIGN 4.22's sin / cos figure), relative to max(1, |e|); a Jacobian
    entry is a difference of two such errors times 1 / 2e-9, so within 2 * 1e-15 * 5e8 = 1e-6 on the same scale."""
    exe = _build_program(tmp_path, "test_posegraph_edge.cpp")
    g = K.make_graph(20, **K.REALISTIC)
    est, edges, meas = g["estimates"], g["edges"], g["meas"]
    ne = len(edges)
    assert ne >= 48
    rng = np.random.default_rng(5)
    angles = [0.0, 1e-9, 1e-4, 4.4e-3, 4.6e-3, 0.1, 1.0, 3.0]
    logs = []
    for a in angles:
        ax = rng.normal(size=3)
        w = ax / np.linalg.norm(ax) * a
        logs.append(s3.sim3_exp([float(w[0]), float(w[1]), float(w[2]), 0.3, -1.2, 2.5]))
    # W-like matrices whose pivots sit in every row order, with a right-hand side
    lus = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        M = np.eye(3)[list(perm)] * np.array([3.0, 2.0, 1.5]) + rng.normal(size=(3, 3)) * 0.2
        lus.append(np.concatenate([M, rng.normal(size=(3, 1))], 1))
    inp = np.concatenate([[len(est)], est.reshape(-1), [ne], np.concatenate([edges.astype(np.float64), meas], 1).reshape(-1),
                          [len(logs)], np.array(logs).reshape(-1), [len(lus)], np.array(lus).reshape(-1)]).astype("<f8")
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.tofile(fin)
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr[-3000:]
    out = np.fromfile(fout, "<f8")
    per = out[:ne * 151].reshape(ne, 151)
    err, chi2 = per[:, :6], per[:, 6]
    J = per[:, 7:79].reshape(ne, 2, 6, 6)
    J25 = per[:, 79:].reshape(ne, 2, 6, 6)
    assert J.tobytes() == J25.tobytes()                                     # the 25 evaluations pair up into the same columns
    G = R.Graph(est, np.zeros(len(est), np.uint8), edges, meas)
    E, J0, J1 = R.linearize(G, est)
    d = edge_d(g, est)
    pure, trig = d > SWITCH + 1e-7, d < SWITCH - 1e-7                       # (a perturbation of 1e-9 moves d by less than 1e-8)
    assert pure.sum() >= 10 and trig.sum() >= 10 and (pure | trig).all()
    assert err[pure].tobytes() == E[pure].tobytes() and chi2[pure].tobytes() == R.edge_chi2(E)[pure].tobytes()
    assert J[pure, 0].tobytes() == J0[pure].tobytes() and J[pure, 1].tobytes() == J1[pure].tobytes()
    scale = np.maximum(1.0, np.abs(E[trig]).max(1))
    de = np.abs(err[trig] - E[trig]).max(1) / scale
    dj = np.maximum(np.abs(J[trig, 0] - J0[trig]).max((1, 2)), np.abs(J[trig, 1] - J1[trig]).max((1, 2))) / scale
    print(f"{pure.sum()} small-angle edges bit-equal; {trig.sum()} edges through acos / sin / cos: errors {de.max():.2e}, Jacobians {dj.max():.2e}")
    assert de.max() <= 1e-15 and dj.max() <= 1e-6
    assert np.abs(chi2[trig] - R.edge_chi2(E)[trig]).max() <= 1e-14 * max(1.0, R.edge_chi2(E)[trig].max())
    got_log = out[ne * 151:ne * 151 + 6 * len(logs)].reshape(-1, 6)
    ref_log = R.sim3_log(R.cols(np.array(logs)))
    small = _log_d(R.cols(np.array(logs))) > SWITCH
    assert list(small) == [a < 4.5e-3 for a in angles]                      # both branches, and both sides next to the switch
    assert got_log[small].tobytes() == ref_log[small].tobytes()
    assert np.abs(got_log[~small] - ref_log[~small]).max() <= 1e-15 * max(1.0, np.abs(ref_log).max())
    got_lu = out[ne * 151 + 6 * len(logs):].reshape(-1, 3)
    for M, x in zip(lus, got_lu):
        ref = np.array([float(v) for v in R.lu3_solve([[M[i][j] for j in range(4)] for i in range(3)])])
        assert x.tobytes() == ref.tobytes() and np.abs(M[:, :3] @ x - M[:, 3]).max() < 1e-13


def test_exp_of_log_is_the_identity():
    """exp(log(S)) = S within 1e-12 wherever the two rules allow it: below theta = 1e-5 (both small-angle branches) and past Sim3::log's
    switch at 4.47e-3 rad.  Between the two, g2o's formulas themselves fall short, by two terms that are written down here instead of
    being hidden by the choice of angles:
      * log switches on d > 1 - 1e-5 and returns omega = deltaR / 2 = sin(theta) * axis there: the angle comes back short by theta -
        sin(theta) <= theta^3 / 6 (1.5e-8 at the switch), the translation by that times |t|;
      * exp (sim3_edge_dev.h, unchanged) takes A = (1 - cos(theta)) / theta^2 from theta = 1e-5 on: 1 - cos(theta) carries the rounding
        of cos near 1 (1.1e-16 absolute), so A is off by up to 2.2e-16 / theta^2 and A Omega t by 2.2e-16 |t| / theta (3e-11 at 1e-5).
    In that window the bound is 1e-12 + (theta^3 / 6 + 4.4e-16 / theta)(1 + |t|); the worst defects are printed."""
    rng = np.random.default_rng(9)
    worst_out = worst_in = 0.0
    for a in [0.0, 1e-9, 1e-6, 9e-6, 1.1e-5, 8e-5, 1e-3, 4.4e-3, 4.6e-3, 0.1, 1.0, 2.0, 3.0] * 5:
        ax = rng.normal(size=3)
        w = ax / np.linalg.norm(ax) * a
        S = s3.sim3_exp([float(w[0]), float(w[1]), float(w[2])] + [float(v) for v in rng.normal(size=3) * 2])
        back = s3.sim3_exp([float(v) for v in R.sim3_log(S)[0]])
        diff = max(abs(x - y) for x, y in zip(S, back))
        window = 1e-5 <= a < 4.47e-3
        bound = 1e-12 + ((a ** 3 / 6 + 4.4e-16 / a) * (1 + float(np.linalg.norm(S[4:7]))) if window else 0.0)
        assert diff <= bound, (a, diff, bound)
        if window:
            worst_in = max(worst_in, diff)
        else:
            worst_out = max(worst_out, diff)
    print(f"exp(log(S)) - S: {worst_out:.2e} outside the window, {worst_in:.2e} inside it")


@pytest.mark.parametrize("n", [2, 7, 99])
def test_drift_free_graph_does_not_move(n):
    g = K.make_graph(n, loop=None, drift=None)
    o = R.optimize(*K.args(g))
    assert o["chis"][0] < 1e-20 and np.abs(o["est"] - g["estimates"]).max() <= 1e-12
    if g["isolated"] is not None:
        assert o["est"][g["isolated"]].tobytes() == g["estimates"][g["isolated"]].tobytes()


@pytest.mark.parametrize("family, n", [("consistent", 2), ("consistent", 7), ("consistent", 99), ("realistic", 7), ("realistic", 99)])
def test_chi2_never_rises_and_falls_by_the_recorded_factor(family, n):
    if family == "consistent":
        o, factor = K.reference(n, K.CONV[n][0]), K.MIN_REDUCTION
    else:
        o, factor = R.optimize(*K.args(K.realistic(n))), K.MIN_REDUCTION_REALISTIC
    chis = o["chis"]
    assert all(b <= a for a, b in zip(chis, chis[1:])) and len(chis) == 1 + sum(o["accepts"])
    assert chis[-1] * factor <= chis[0], (chis[0], chis[-1])
    assert np.allclose(R.edge_chi2(R.errors(R.Graph(*K.args(K.graph(n) if family == "consistent" else K.realistic(n))), o["est"])).sum(), chis[-1], rtol=1e-9, atol=1e-30)


def test_cases_have_the_patterns():
    for n in K.SIZES:
        g = K.graph(n)
        e = [tuple(x) for x in g["edges"]]
        assert g["fixed"].sum() == 1 and len(g["fixed"]) - 1 == n and not g["fixed"][0]
        a, b = g["dup"]
        assert e[a] == e[b][::-1]                                           # one pair joined twice, in opposite orientation
        if n >= 3:
            assert g["isolated"] is not None and not any(g["isolated"] in x for x in e) and not g["fixed"][g["isolated"]]
        if n >= 7:
            d = edge_d(g, g["estimates"])
            assert (d > SWITCH).sum() >= 3 and (d < SWITCH).sum() >= 3      # both sides of Sim3::log's switch at the start
            assert any(g["fixed_v"] in x for x in e[len(e) - 3:])           # loop edges into the fixed vertex


@pytest.mark.parametrize("n", K.SIZES)
def test_gpu_cases_are_qualified(n):
    """the two tables of tests/essential_graph_cases.py (its module text says what they mean), recomputed"""
    k_adm, d_adm, k_conv, d_conv, a, b = K.qualify(n, max_iterations=K.CONV[n][0] + 1)
    print(f"n_free {n}: admitted {k_adm} iterations (difference {d_adm:.2e}), converged {k_conv} (difference {d_conv:.2e})")
    # (the spreads are rounding noise of the two runs: they may come out up to 3 x the recorded figure under another BLAS; the prefix
    #  lengths may not come out shorter)
    assert k_adm == K.ADM[n][0] and d_adm <= 3 * K.ADM[n][1] + 1e-15
    assert K.ADM[n][2] == (K.BOUND if K.ADM[n][1] <= K.QUAL_DIFF else 100 * K.ADM[n][1])
    assert k_conv >= K.CONV[n][0]
    k_conv = K.CONV[n][0]
    d_conv = float(np.abs(a["est_after"][k_conv - 1] - b["est_after"][k_conv - 1]).max())
    assert d_conv <= K.QUAL_DIFF and d_conv <= 3 * K.CONV[n][1] + 1e-15
    assert a["chis"][0] >= K.MIN_REDUCTION * a["chis"][sum(acc for acc, it in zip(a["accepts"], a["trial_iter"]) if it < k_conv)]


def test_header_declares_and_library_exports_the_entry_points():
    from orb_slam2_ros2_amd import _lib, Optimizer
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)                       # loading must not need a GPU
    for name in ("orbfe_pose_graph_optimize", "orbfe_debug_pose_graph_edges", "orbfe_debug_pose_graph_phases"):
        assert re.search(r"orbfe_status\s+" + name + r"\(", hdr), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert "typedef struct orbfe_pose_graph" in hdr and re.search(r"#define ORBFE_PG_MAX_FREE (\d+)", hdr).group(1) == "1024"
    assert callable(Optimizer.optimizeEssentialGraph) and callable(_lib.Context.pose_graph_optimize) and callable(_lib.Context.debug_pose_graph_edges)


def test_refusals_need_no_context():
    """the argument checks come first: without a context every call is ORBFE_EBADARG, whatever else it carries"""
    from orb_slam2_ros2_amd import _lib
    lib = _lib.load()
    g = K.graph(7)
    pg, keep = _lib.Context._pose_graph(*K.args(g))
    out, chi, stats = g["estimates"].copy(), np.zeros(len(g["edges"])), np.full(2, -3, np.int32)
    assert lib.orbfe_pose_graph_optimize(None, ctypes.byref(pg), 20, _lib.ptr(out), _lib.ptr(chi), _lib.ptr(stats)) == 1
    err, jac = np.zeros((len(chi), 6)), np.zeros((len(chi), 72))
    assert lib.orbfe_debug_pose_graph_edges(None, ctypes.byref(pg), _lib.ptr(err), _lib.ptr(chi), _lib.ptr(jac)) == 1
    assert (stats == -3).all() and not chi.any() and not err.any() and not jac.any() and out.tobytes() == g["estimates"].tobytes()


def test_dropin_builds_the_graph_over_minimal_types(tmp_path):
    """tests/cpp/test_essential_dropin.cpp up to the device call (`build`): the vertices (good keyframes, the corrected Sim3 where there
    is one, the loop keyframe fixed), the loop connections with the graphTh rule and its exception for the (current, loop) pair, bad
    keyframes skipped, the spanning tree / loop edges / covisibility >= 100 with sAlreadyConnected keyed by the ORDERED pair -- (5, 4)
    is not added twice, (4, 5) is --, the measurements from the uncorrected Sim3 where there is one, all bit for bit; and the refusals,
    before anything is launched or written.  The GPU suite runs the whole program."""
    text, sc = K.dropin_scene()
    inp = tmp_path / "in.txt"
    inp.write_text(text)
    exe = str(tmp_path / "t")
    subprocess.check_call(K.dropin_build_command(ROOT, exe), timeout=300)
    r = subprocess.run([exe, str(inp), "build"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    verts, edges = K.dropin_parse_graph(r.stdout)
    want_v, first, rest = K.dropin_expected_graph(sc)
    assert verts == want_v
    assert [v[0] for v in verts] == [0, 1, 2, 3, 4, 5, 8] and [v[1] for v in verts] == [0, 1, 0, 0, 0, 0, 0]
    assert sorted(edges[:len(first)]) == sorted(first) and edges[len(first):] == rest
    pairs = [e[:2] for e in edges]
    assert sorted(pairs[:2]) == [(5, 4), (8, 1)]                             # (8, 1): weight 0 < graphTh, kept as the (current, loop) pair
    assert (8, 2) not in pairs and (8, 7) not in pairs and pairs.count((5, 4)) == 1 and (4, 5) in pairs and (5, 1) in pairs
    assert (8, 5) in pairs and (8, 7) not in pairs and (3, 4) not in pairs   # covisibility 100 is in, 99 is out, a bad parent is skipped
    tail = [ln for ln in r.stdout.splitlines() if not ln.startswith(("v ", "e "))]
    assert tail == ["free scale: invalid_argument", "free scale, whole function: invalid_argument", "mfS != 1: invalid_argument",
                    "mfS != 1, uncorrected: invalid_argument", "no keyframe 0: runtime_error", "poses set: 0, map updated: 0"]


from test_sim3_host import NEEDS_REF  # noqa: E402


@NEEDS_REF
def test_dropin_compiles_as_the_body_of_the_reference_function(tmp_path):
    """g++ -fsyntax-only of tests/cpp/ref_essential_body.cpp: dropin::optimizeEssentialGraph as the one-line body of
    Optimizer::optimizeEssentialGraph, with the reference's Optimizer.h / KeyFrame.h / MapPoint.h / Map.h /
    Sim3Solver.h"""
    from test_reference_compile import _include_dir
    inc = _include_dir(str(tmp_path / "inc"), friend_line=True)
    stubs = os.path.join(ROOT, "tests", "cpp", "stubs")
    host = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + inc, "-I" + stubs, "-I" + os.path.join(stubs, "refgen"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "cpp", "ref_essential_body.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
