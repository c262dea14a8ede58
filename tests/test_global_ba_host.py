"""Optimizer::globalOptimization without a GPU: the restatement of the block-sparse path (tests/global_ba_restatement.py) against the
oracle's one optimize(n), the host-side symbolic structure (csrc/bsr_symbolic.h) in a stand-alone program under the host sanitizers
against the restatement's, the trajectory generator, and header / library / binding agreement."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import global_ba_restatement as R
from orb_slam2_ros2_amd import ba_synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (seed, keyframes, points per keyframe, loop keyframes, Huber, outliers): the three problems of the CPU check; the GPU suite runs the
# same three through the device
CPU_CASES = {"40_huber": (1, 40, 10, 3, True, 0.05), "40_plain": (2, 40, 10, 3, False, 0.0), "90_loop": (3, 90, 10, 3, True, 0.05)}


def trajectory(name):
    seed, n_kf, per_kf, loop, huber, outliers = CPU_CASES[name]
    pr = ba_synth.make_trajectory_problem(seed, n_kf, per_kf, loop=loop, huber=huber, outliers=outliers)
    fixed = np.zeros(n_kf, np.uint8)
    fixed[0] = 1
    return pr, fixed


def pose_dist(a, b):
    """max abs difference of (q, t) with the quaternion sign fixed"""
    s = np.sign((a[:, :4] * b[:, :4]).sum(1, keepdims=True))
    return max(np.abs(a[:, :4] - s * b[:, :4]).max(), np.abs(a[:, 4:] - b[:, 4:]).max())


@pytest.mark.parametrize("name", list(CPU_CASES))
def test_restatement_matches_the_oracle(orc, name):
    """One optimize(10) is orc.ba_local_optimize(iters1 = 10, iters2 = 0): the second round of zero iterations moves nothing.  The
    restatement with block-Jacobi PCG at tol = 1e-10 runs the same iterations and lands within 1e-7 (test_local_ba.py's bound for the same
    quantities; measured here 7.3e-11 on poses and 1.8e-9 on points at worst)."""
    pr, fixed = trajectory(name)
    o = orc.ba_local_optimize(pr, fixed, iters1=10, iters2=0)
    r = R.optimize(orc, pr, fixed, 10, tol=1e-10)
    dp, dx = pose_dist(r["poses"], o["poses"]), np.abs(r["points"] - o["points"]).max()
    trials, cg, rejected = r["cg_stats"]
    print(f"{name}: {r['iters']} iterations, {trials} trials, {cg} CG iterations; poses {dp:.2e}, points {dx:.2e}")
    assert r["iters"] == o["iters"][0] == 10 and o["iters"][1] == 0
    assert dp < 1e-7 and dx < 1e-7
    assert np.allclose(r["chi2"], o["chi2"], rtol=1e-6, atol=1e-9)
    assert rejected == 0 and cg <= trials * 24 * int((fixed == 0).sum())
    assert np.array_equal(r["poses"][0], pr["poses"][0])


def test_restatement_exact_solve_agrees(orc):
    """the same loop with a dense solve of the block-CSR system: what separates the two is the solver's tolerance alone"""
    pr, fixed = trajectory("40_huber")
    a, b = R.optimize(orc, pr, fixed, 10, exact=True), R.optimize(orc, pr, fixed, 10, tol=1e-10)
    assert a["iters"] == b["iters"] and pose_dist(a["poses"], b["poses"]) < 1e-8 and np.abs(a["points"] - b["points"]).max() < 1e-8


def test_trajectory_problem_is_what_it_says():
    pr = ba_synth.make_trajectory_problem(5, 90, 10)
    again = ba_synth.make_trajectory_problem(5, 90, 10)
    assert all(np.array_equal(pr[k], again[k]) for k in pr if isinstance(pr[k], np.ndarray))          # deterministic
    ek, ep = pr["edge_pose"], pr["edge_point"]
    assert pr["points"].shape == (900, 3) and pr["poses"].shape == (90, 7)
    per_point = np.bincount(ep, minlength=900)
    assert per_point.min() >= 2 and per_point.max() <= 8
    assert np.all(np.diff(ep) >= 0) and all(np.all(np.diff(ek[ep == p]) > 0) for p in range(0, 900, 37))  # point-major, keyframes ascending
    assert 0.75 < pr["is_stereo"].mean() < 0.85 and ((pr["meas"][:, 2] == -1.0) == (pr["is_stereo"] == 0)).all()
    assert np.array_equal(pr["poses"][0], [0, 0, 0, 1, 0, 0, 0])                                      # keyframe 0 at its true pose
    sigma = np.float32(1.2) ** np.arange(8, dtype=np.float32)
    assert set(np.unique(pr["info"])) <= set(((np.float32(1) / sigma) ** 2).astype(np.float64))      # 1 / sigma^2, both edge kinds
    assert set(np.unique(pr["huber_delta"])) == {float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815)))}
    assert (ba_synth.make_trajectory_problem(5, 90, 10, huber=False)["huber_delta"] == -1).all()
    # the reduced system is block-sparse: a band plus loop blocks between the last keyframes and the first ones
    slot, free = R.slots(90, np.eye(1, 90, 0, dtype=np.uint8)[0])
    sym = R.bsr_symbolic(free.size, 900, ek, ep, slot)
    rows = R.bsr_rows(sym["row_off"])
    fill = sym["col"].size / free.size ** 2
    # (a loop keyframe, at x <= 0.6 m, sees a point up to 0.62 * 7 m ahead of it, and so does a keyframe of the chain from the other side:
    #  x <= 0.6 + 2 * 4.3 m, keyframe 37 at most)
    far = np.abs(rows - sym["col"]) > 7
    assert 0.1 < fill < 0.25 and far.any() and (np.minimum(rows, sym["col"])[far] < 37).all() and (np.maximum(rows, sym["col"])[far] >= 86).all()


def _symbolic_cases():
    """(slot, edge_pose, edge_point, n_points) of small graphs with the patterns that matter"""
    out = {}
    # a pose that sees a point twice (pose 1, point 0), a fixed pose in the middle, a free keyframe with no edge (pose 4)
    out["twice_and_isolated"] = (np.array([0, 1, -1, 2, 3]), np.array([0, 1, 1, 2, 3, 0, 3, 1]), np.array([0, 0, 0, 0, 1, 1, 1, 2]), 3)
    # two components that share no point: keyframes {0, 1, 2} on points {0, 1}, keyframes {3, 4} on points {2, 3}
    out["two_components"] = (np.arange(5), np.array([0, 1, 2, 1, 3, 4, 4, 3]), np.array([0, 0, 1, 1, 2, 2, 3, 3]), 4)
    # nothing free | no edge at all
    out["all_fixed"] = (np.array([-1, -1]), np.array([0, 1]), np.array([0, 0]), 1)
    out["no_edges"] = (np.array([0, 1, 2]), np.zeros(0, np.int64), np.zeros(0, np.int64), 2)
    pr = ba_synth.make_trajectory_problem(7, 40, 6)
    slot, _ = R.slots(40, np.eye(1, 40, 0, dtype=np.uint8)[0])
    out["trajectory"] = (slot, pr["edge_pose"], pr["edge_point"], 240)
    return out


@pytest.fixture(scope="module")
def symbolic_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bsr") / "t")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "orb_slam2_ros2_amd", "csrc"), "-o", exe,
            os.path.join(ROOT, "tests", "cpp", "test_bsr_symbolic.cpp")]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        # only a g++ WITHOUT the sanitizers' runtimes (the link step cannot find libasan / libubsan) may run the program plain
        assert re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S* ?: No such file", r.stderr), r.stderr[-3000:]
        subprocess.check_call(base, timeout=300)
    return exe


@pytest.mark.parametrize("name", ["twice_and_isolated", "two_components", "all_fixed", "no_edges", "trajectory"])
def test_symbolic_header_matches_the_restatement(symbolic_program, name):
    """csrc/bsr_symbolic.h is pure C++: a stand-alone program (nothing of it is loaded into python) builds the structure under the
    address and undefined-behaviour sanitizers; every array equals the restatement's."""
    slot, ek, ep, n_points = _symbolic_cases()[name]
    nf = int((slot >= 0).sum())
    text = f"{slot.size} {n_points} {ek.size}\n" + " ".join(str(int(s)) for s in slot) + "\n" + "\n".join(f"{int(a)} {int(b)}" for a, b in zip(ek, ep)) + "\n"
    r = subprocess.run([symbolic_program], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = {ln.split()[0]: np.array(ln.split()[1:], np.int64) for ln in r.stdout.splitlines()}
    want = R.bsr_symbolic(nf, n_points, ek, ep, slot)
    for key in ("row_off", "col", "twin", "low", "low_row", "pair_off"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["pairs"].reshape(-1, 2), want["pairs"])
    # the rules themselves, on the program's output
    rows = R.bsr_rows(got["row_off"])
    col = got["col"]
    assert got["row_off"].size == nf + 1 and all(np.all(np.diff(col[rows == i]) > 0) and i in col[rows == i] for i in range(nf))
    assert np.array_equal(rows[got["twin"]], col) and np.array_equal(col[got["twin"]], rows)
    assert np.array_equal(got["low"], np.flatnonzero(rows >= col))
    covis = {(i, i) for i in range(nf)}
    for p in range(n_points):
        s = [int(slot[k]) for k in ek[ep == p] if slot[k] >= 0]
        covis |= {(a, b) for a in s for b in s}
    assert set(zip(rows.tolist(), col.tolist())) == covis
    if name == "twice_and_isolated":
        l = list(zip(got["low_row"], col[got["low"]])).index((1, 1))
        assert [tuple(x) for x in got["pairs"].reshape(-1, 2)[got["pair_off"][l]:got["pair_off"][l + 1]]] == [(1, 1), (1, 2), (2, 1), (2, 2), (7, 7)]
        assert col[rows == 3].tolist() == [3]                                   # the free keyframe with no edge keeps its diagonal block
    if name == "two_components":
        assert not ((rows < 3) & (col >= 3)).any()


def test_header_library_and_binding_agree():
    from orb_slam2_ros2_amd import _lib, Optimizer
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)                       # loading must not need a GPU
    for name in ("orbfe_ba_global_optimize", "orbfe_debug_ba_reduced_bsr", "orbfe_debug_bsr_pcg", "orbfe_debug_ba_global_phases"):
        assert re.search(r"orbfe_status\s+" + name + r"\(", hdr), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert re.search(r"#define ORBFE_ABI_VERSION (\d+)", hdr).group(1) == "4" and lib.orbfe_abi_version() == 4
    assert int(re.search(r"#define ORBFE_GBA_DENSE_MAX_FREE (\d+)", hdr).group(1)) == _lib.GBA_DENSE_MAX_FREE
    m = re.search(r"typedef struct orbfe_ba_global_options \{(.*?)\} orbfe_ba_global_options;", hdr, re.S)
    assert re.findall(r"(int32_t|double)\s+(\w+);", m.group(1)) == [("int32_t", "solver"), ("double", "pcg_tol"), ("int32_t", "pcg_max_iter")]
    assert [(f[0], f[1]) for f in _lib.BaGlobalOptions._fields_] == [("solver", ctypes.c_int32), ("pcg_tol", ctypes.c_double),
                                                                     ("pcg_max_iter", ctypes.c_int32)]
    m = re.search(r"typedef struct orbfe_ba_global_out \{(.*?)\} orbfe_ba_global_out;", hdr, re.S)
    assert re.findall(r"\*\s*(\w+);", m.group(1)) == [f[0] for f in _lib.BaGlobalOut._fields_] == ["poses", "points", "chi2", "iterations", "cg_stats"]
    assert callable(Optimizer.globalOptimization) and callable(_lib.Context.ba_global_optimize)
    assert callable(_lib.Context.debug_ba_reduced_bsr) and callable(_lib.Context.debug_bsr_pcg)


def test_refusals_need_no_context():
    """the argument checks come first: without a context every call is ORBFE_EBADARG and writes nothing"""
    from orb_slam2_ros2_amd import _lib
    lib = _lib.load()
    pr, fixed = trajectory("40_huber")
    bp, keep, (nk, npt, E) = _lib.Context._ba_problem(None, pr)
    poses, points = np.full((nk, 7), -3.0), np.full((npt, 3), -3.0)
    o = _lib.BaGlobalOut(_lib.ptr(poses).value, _lib.ptr(points).value, None, None, None)
    assert lib.orbfe_ba_global_optimize(None, ctypes.byref(bp), _lib.ptr(fixed), 10, None, None, ctypes.byref(o)) == 1
    x, it, ok = np.full(6, -3.0), ctypes.c_int32(-3), ctypes.c_int32(-3)
    ro, col, blk, rhs = np.array([0, 1], np.int32), np.zeros(1, np.int32), np.eye(6).reshape(1, 36), np.ones(6)
    assert lib.orbfe_debug_bsr_pcg(None, 1, _lib.ptr(ro), _lib.ptr(col), _lib.ptr(blk), _lib.ptr(rhs), 0.0, 0, _lib.ptr(x), ctypes.byref(it), ctypes.byref(ok)) == 1
    nnzb = ctypes.c_int32(-3)
    assert lib.orbfe_debug_ba_reduced_bsr(None, ctypes.byref(bp), _lib.ptr(fixed), 0.0, 0, ctypes.byref(nnzb), _lib.ptr(ro), None, None, None) == 1
    assert (poses == -3).all() and (points == -3).all() and (x == -3).all() and it.value == ok.value == nnzb.value == -3


@pytest.mark.parametrize("use_rk", [False, True])
def test_dropin_builds_the_graph_over_minimal_types(tmp_path, use_rk):
    """tests/cpp/test_global_ba_dropin.cpp up to the device call (`build`): null and bad keyframes and map points are skipped, and so are
    observers that are gone, bad or not in vpKfs; only keyframe 0 is fixed; the map points go in vpMps order; every edge carries
    getScaledFactorInv2 (mono edges too -- the stand-in's getScaledFactorInv returns -1e30) and a Huber delta only with bUseRk; a map
    point without a usable observation is still a vertex.  The GPU suite runs the whole program."""
    import global_ba_dropin_scene as S
    text, want = S.scene(use_rk)
    inp = tmp_path / "in.txt"
    inp.write_text(text)
    exe = str(tmp_path / "t")
    subprocess.check_call(S.build_command(ROOT, exe), timeout=300)
    r = subprocess.run([exe, str(inp), "build"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    got = S.parse(r.stdout)
    pr = got["problem"]
    assert got["camera"] == S.CAMERA
    assert got["kf_ids"] == want["kf_ids"] == [0, 1, 2, 3, 4, 7] and got["fixed"] == [1, 0, 0, 0, 0, 0]
    assert pr["poses"].tobytes() == want["poses"].tobytes()
    assert got["lm_index"] == want["lm_index"] and S.BAD_MP not in got["lm_index"] and len(got["lm_index"]) == want["n_mp"] - 1
    assert pr["points"].tobytes() == want["points"].tobytes()
    assert np.all(np.diff(pr["edge_point"]) >= 0)                                # vpMps order, a map point's observations together
    n_edges = 0
    for v, p in enumerate(got["lm_index"]):
        rows = sorted((got["kf_ids"][int(k)], int(st)) + tuple(m) + (i, h) for k, st, m, i, h in
                      zip(pr["edge_pose"][pr["edge_point"] == v], pr["is_stereo"][pr["edge_point"] == v], pr["meas"][pr["edge_point"] == v].tolist(),
                          pr["info"][pr["edge_point"] == v], pr["huber_delta"][pr["edge_point"] == v]))
        assert rows == want["edges"][p], p
        n_edges += len(rows)
    assert n_edges == pr["edge_pose"].size > 100
    assert want["edges"][S.BARE_MP] == [] and want["edges"][S.ORPHAN_MP] == [] and S.BARE_MP in got["lm_index"] and S.ORPHAN_MP in got["lm_index"]
    assert (pr["is_stereo"] == 0).any() and (pr["info"] > 0).all() and set(pr["info"]) <= set(S.INV_SIGMA2.astype(np.float64))
    assert set(pr["huber_delta"]) == ({S.DELTA_MONO, S.DELTA_STEREO} if use_rk else {-1.0})
    assert ((pr["huber_delta"] == S.DELTA_STEREO) == (pr["is_stereo"] != 0)).all() or not use_rk


from test_sim3_host import NEEDS_REF  # noqa: E402


@NEEDS_REF
def test_dropin_compiles_as_the_body_of_the_reference_function(tmp_path):
    """g++ -fsyntax-only of tests/cpp/ref_global_ba_body.cpp: dropin::globalOptimization as the one-line body of
    Optimizer::globalOptimization, with the reference's Optimizer.h / KeyFrame.h / MapPoint.h / Camera.h"""
    from test_reference_compile import _include_dir
    inc = _include_dir(str(tmp_path / "inc"), friend_line=True)
    stubs = os.path.join(ROOT, "tests", "cpp", "stubs")
    host = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + inc, "-I" + stubs, "-I" + os.path.join(stubs, "refgen"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "cpp", "ref_global_ba_body.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
