"""The restatement of Sim3Solver + Ransac<Sim3Ret> (tests/sim3_restatement.py) on its own: modelFunc against an independent Kabsch, the
triplet draws and the budget against g++-compiled copies, one scene for each of S1-S7 with the driver asserting that the path was taken,
and the surface: the C header, the drop-in against the reference's declarations, creation order and the lazy set."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sim3_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src/ORB_SLAM2"
NEEDS_REF = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "ORB_SLAM2")) or shutil.which("g++") is None,
                               reason="needs the reference tree and g++")


def gxx(tmp_path, src, name="t"):
    (tmp_path / f"{name}.cpp").write_text(src)
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, str(tmp_path / f"{name}.cpp")], timeout=300)
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=300).stdout.split()


def solver(seed, N, outlier=0.0, noise=0.5, **kw):
    return S.Solver(*S.scene(np.random.default_rng(seed), N, outlier=outlier, noise=noise), **kw)


# ---- 1. the restatement's numerics -------------------------------------------------------------------------------------------------
def kabsch(P, Q):
    """least-squares rigid motion Q = R P + t in float64 by SVD (Kabsch / Umeyama without scale): independent of Horn's quaternion"""
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    cp, cq = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((P - cp).T @ (Q - cq))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return np.concatenate([R.reshape(9), cq - R @ cp])


def test_model_func_equals_kabsch():
    """This checks the restatement, not the code under test.  Over the 800 samples below (3, 4, 10 and 60 pairs of 40 scenes, depths
    2 .. 20 m) the largest |difference| of any of the 12 model entries measured on the CPU is 3.27e-5 (float32 arithmetic on
    coordinates up to 20 m against float64); the bound is 4 x that."""
    worst = 0.0
    for seed in range(40):
        rng = np.random.default_rng(seed)
        sol = S.Solver(*S.scene(rng, 60, outlier=0.0, noise=0.5))
        for k in (3, 4, 10, 60):
            for _ in range(5):
                idx = rng.choice(60, k, replace=False)
                m = S.model_func(sol.P3[idx][None], sol.Q3[idx][None])[0]
                worst = max(worst, float(np.abs(m - kabsch(sol.P3[idx], sol.Q3[idx])).max()))
    print("largest |model - kabsch|:", worst)
    assert worst <= 4 * 3.27e-5


def test_triplet_draws_equal_libstdcxx(tmp_path):
    out = gxx(tmp_path, r"""
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>
int main() {
  std::default_random_engine generator;
  for (int mnN = 3; mnN <= 2000; ++mnN) {
    std::uniform_int_distribution<std::size_t> distribution(0, mnN - 1);
    std::vector<std::size_t> v;
    while (v.size() != 3) {
      std::size_t r = distribution(generator);
      if (std::find(v.begin(), v.end(), r) == v.end()) v.push_back(r);
    }
    std::printf("%zu %zu %zu\n", v[0], v[1], v[2]);
  }
}""")
    e = S.Engine()
    want = [i for N in range(3, 2001) for i in S.random_sample(e, N, 3)]
    assert list(map(int, out)) == want


def test_budget_with_min_set_3_equals_compiled_expression(tmp_path):
    out = gxx(tmp_path, r"""
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <emmintrin.h>
static int cvRound(double v) { return _mm_cvtsd_si32(_mm_set_sd(v)); }
int main() {
  const int nMinSet = 3, nMaxIterations = 100;
  const float fRatio = 0.4, fProb = 0.99;
  for (int mnN = 0; mnN <= 3000; ++mnN) {
    int mnMinInlier = std::max((float)nMinSet, mnN * fRatio);
    float r = (float)mnMinInlier / mnN;
    int it;
    if (r >= 1) it = 0;
    else it = std::min(nMaxIterations, cvRound(std::log(1 - fProb) / std::log(1 - std::pow(r, nMinSet))));
    std::printf("%d %d\n", mnMinInlier, it);
  }
}""")
    got = [v for N in range(3001) for v in S.ransac_params(N, min_set=3)]
    assert list(map(int, out)) == got


# ---- 2. S1 - S7, each on a scene that reaches it -----------------------------------------------------------------------------------
class Spy(S.Solver):
    """records the list every refine receives"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.refine_lists = []

    def model(self, idx):
        self.refine_lists.append(list(idx))
        return super().model(idx)


def test_s1_min_set_is_three_and_the_other_parameters_are_honoured():
    with pytest.raises(AssertionError):
        solver(1, 60, params=(4, 100, 0.4, 0.99))
    a, b = solver(1, 60), solver(1, 60, params=(3, 7, 0.5, 0.9))
    assert (a.min_inlier, a.max_it) == S.ransac_params(60, 3) == (24, 70)
    assert (b.min_inlier, b.max_it) == S.ransac_params(60, 3, 7, 0.5, 0.9) == (30, 7)
    e = S.Engine()
    a.iterate(e, 1)
    f = S.Engine()
    S.random_sample(f, 60, 3)                                                      # one draw is three indices
    assert e.state == f.state


def test_s2_the_list_is_cleared_refine_success_returns_refined_fallback_returns_unrefined():
    # a refine success: the list refine received is the hypothesis's own (no duplicates, ascending) and the result is refine's
    s = Spy(*S.scene(np.random.default_rng(1), 100, outlier=0.1))
    ret, no_more, model, lst = s.iterate(S.Engine(), 5, None, [7, 7, 7])
    assert ret and s.stats["refine_success"] == 1
    assert all(l == sorted(set(l)) for l in s.refine_lists) and lst == s.check(model) and 7 in lst and lst.count(7) == 1
    assert np.array_equal(model, s.model(s.refine_lists[-1]))
    # the fallback: the best hypothesis's own list and model, not refine's
    s = Spy(*S.scene(np.random.default_rng(3), 60, outlier=0.5, noise=1.5))
    e = S.Engine()
    log = S.loop_closing_loop(lambda p, n: s.iterate(e, n), 1, 5)
    assert s.stats["refine_failed"] >= 1 and s.stats["fallback_best"] >= 1 and s.stats["refine_success"] == 0
    ret, no_more, model, lst = log[-1][1]
    assert ret and lst == s.best_list and lst in s.refine_lists and model is s.best_model and lst == s.check(model)


def test_s3_a_successful_refine_does_not_spend_the_budget():
    s = solver(1, 100, outlier=0.1)
    e = S.Engine()
    ret, no_more, model, lst = s.iterate(e, 5)
    assert ret and s.stats["refine_success"] == 1 and len(lst) > s.min_inlier
    f = S.Engine()
    for _ in range(s.cur + 1):
        S.random_sample(f, 100, 3)
    assert e.state == f.state and s.cur < 5                                        # the draw is spent, the iteration is not


def test_s4_the_best_model_persists_and_needs_more_than_min_inlier():
    s = solver(3, 60, outlier=0.5, noise=1.5)
    e = S.Engine()
    seen_best = False
    fallbacks = 0
    for call in range(200):
        best_before = s.best
        ret, no_more, model, lst = s.iterate(e, 1)
        if s.best != best_before:
            assert s.best > s.min_inlier and s.best > best_before                  # only a count above mnMinInlier sets it
            seen_best = True
        if seen_best:
            assert ret                                                             # every later call returns true ..
            if model is s.best_model:
                assert lst == s.best_list                                          # .. with the best model and its list
                fallbacks += 1
        else:
            assert not ret
        if no_more:
            break
    assert seen_best and fallbacks >= 2 and s.stats["fallback_best"] == fallbacks and no_more
    ret, no_more, model, lst = s.iterate(e, 5, None, [])                           # the budget is spent: still the best model
    assert ret and no_more and model is s.best_model and s.stats["zero_budget"] == 1


def test_s5_small_problems():
    for N in (0, 2):
        s = solver(1, N)
        assert s.iterate(S.Engine(), 5) == (False, True, None, []) and s.stats["too_few"] == 1
    s = solver(1, 3)
    assert (s.min_inlier, s.max_it) == (3, 0)
    e = S.Engine()
    assert s.iterate(e, 5) == (False, True, None, []) and e.state == 1 and s.stats["zero_budget"] == 1 and s.stats["failed"] == 1
    # bNoMore is only ever set: a call with budget left reports False, and the caller's flag stays whatever it was
    s = solver(1, 60, outlier=1.0)
    assert s.iterate(S.Engine(), 5)[1] is False


def test_s6_the_arguments_end_as_the_reference_leaves_them():
    entry_model, entry_list = np.arange(12, dtype=np.float32), [5, 1, 1]
    for N in (2, 3):                                                               # nothing ran: untouched
        r = solver(1, N).iterate(S.Engine(), 5, entry_model, entry_list)
        assert r[2] is entry_model and r[3] == entry_list
    # a failed call: the last hypothesis's model and its own inliers, whatever came in
    s = solver(2, 60, outlier=1.0)
    e = S.Engine()
    ret, no_more, model, lst = s.iterate(e, 4, entry_model, entry_list)
    assert not ret and s.stats["failed"] == 1
    f = S.Engine()
    for _ in range(4):
        last = S.random_sample(f, 60, 3)
    assert np.array_equal(model, s.model(last)) and lst == s.check(model)
    # a scene with failed refines: every call that returns true returns a hypothesis's own list (one that refine received) and its model
    s = Spy(*S.scene(np.random.default_rng(3), 60, outlier=0.5, noise=1.5))
    e = S.Engine()
    log = S.loop_closing_loop(lambda p, n: s.iterate(e, n), 1, 5)
    assert s.stats["refine_failed"] >= 1 and any(r[0] for _, r in log)
    assert all(r[3] in s.refine_lists and r[3] == s.check(r[2]) for _, r in log if r[0])


def test_s7_its_own_engine_three_indices_a_draw():
    a, b = solver(1, 60, outlier=1.0), solver(2, 40, outlier=1.0)
    e = S.Engine()
    a.iterate(e, 3)
    b.iterate(e, 2)
    f = S.Engine()
    for N in (60, 60, 60, 40, 40):
        idx = S.random_sample(f, N, 3)
        assert len(set(idx)) == 3 and all(0 <= i < N for i in idx)
    assert e.state == f.state and a.stats["failed"] == 1 and b.stats["failed"] == 1
    # apart from PnP's: the library keeps two states (the device test drives both); here, the two entry points exist
    from orb_slam2_ros2_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "orbfe_sim3_engine") and hasattr(lib, "orbfe_pnp_engine")


def test_loop_closing_loop_counts_every_path():
    """the driver over a mixed set: every counter the other tests rely on moves"""
    sols = [solver(1, 100, outlier=0.1), solver(3, 60, outlier=0.5, noise=1.5), solver(2, 60, outlier=1.0), solver(1, 2), solver(1, 3)]
    e = S.Engine()
    log = S.loop_closing_loop(lambda p, n: sols[p].iterate(e, n), len(sols), 5, accept=lambda p, m, inl: False)
    tot = {k: sum(s.stats[k] for s in sols) for k in sols[0].stats}
    assert all(tot[k] > 0 for k in ("refine_success", "fallback_best", "failed", "too_few", "zero_budget", "refine_failed")), tot
    assert len(log) == sum(tot[k] for k in ("refine_success", "fallback_best", "failed", "too_few"))


# ---- 3. surface --------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = ["orbfe_sim3_create", "orbfe_sim3_destroy", "orbfe_sim3_iterate", "orbfe_sim3_engine", "orbfe_sim3_stats", "orbfe_sim3_profile"]


def test_header_declares_and_library_exports_the_entry_points(tmp_path):
    from orb_slam2_ros2_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)                       # loading must not need a GPU
    for name in ENTRY_POINTS:
        assert re.search(r"\b(orbfe_status|void)\s+" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert "#define ORBFE_ABI_VERSION 4" in hdr and lib.orbfe_abi_version() == 4
    assert ctypes.sizeof(_lib.Sim3Params) == 16
    # the header compiles stand-alone, as C and as C++
    for lang, std in (("c", "-std=c11"), ("c++", "-std=c++17")):
        tu = tmp_path / ("tu." + ("c" if lang == "c" else "cpp"))
        tu.write_text('#include "orbfe.h"\nint main(void) { orbfe_sim3_params p = {3, 100, 0.4f, 0.99f}; return p.min_set - 3; }\n')
        r = subprocess.run(["gcc", "-x", lang, std, "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(tu)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]


def test_refusals_need_no_device():
    """argument checks come before the device is looked for"""
    from orb_slam2_ros2_amd import _lib
    (posP, posQ, octP, octQ, poseP, poseQ) = S.scene(np.random.default_rng(1), 10)
    off = np.array([0, 10], np.int64)
    with pytest.raises(_lib.OrbfeError) as e:
        _lib.Sim3Set(off, posP, posQ, octP, octQ, poseP, poseQ, S.SIGMA2, S.CAM, (4, 100, 0.4, 0.99))
    assert e.value.status == 1 and "min_set" in str(e.value)
    with pytest.raises(_lib.OrbfeError) as e:
        _lib.Sim3Set(off, posP, posQ, octP + 8, octQ, poseP, poseQ, S.SIGMA2, S.CAM)
    assert e.value.status == 1 and "octave" in str(e.value)
    with pytest.raises(_lib.OrbfeError) as e:
        _lib.sim3_engine(0)
    assert e.value.status == 1
    old = _lib.sim3_engine(12345)
    assert _lib.sim3_engine(old) == 12345 and _lib.sim3_engine() == old


@NEEDS_REF
def test_dropin_and_the_computeSim3_body_compile_against_the_reference_classes(tmp_path):
    """g++ -fsyntax-only of tests/cpp/ref_sim3_body.cpp: orbfe_sim3_dropin.hpp as the Sim3SolverT of sim3Candidates and the computeSim3
    body of INTEGRATION section 14, with the reference's LoopClosing.h / KeyFrame.h / MapPoint.h / Camera.h / Sim3Solver.h"""
    from test_reference_compile import _include_dir
    inc = _include_dir(str(tmp_path / "inc"), friend_line=True)
    stubs = os.path.join(ROOT, "tests", "cpp", "stubs")
    host = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + inc, "-I" + stubs, "-I" + os.path.join(stubs, "refgen"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "cpp", "ref_sim3_body.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


def test_dropin_creation_order_and_lazy_set(tmp_path):
    """tests/cpp/test_sim3_dropin.cpp up to the first iterate (`create-only`): the vbChoose filter, creation order as problem order, and
    nothing uploaded before an iterate -- which is why this part runs without a device.  The GPU suite runs the whole program."""
    specs = [(1, 12, 0.0), (2, 0, 0.0), (3, 30, 0.5)]
    inp = tmp_path / "in.txt"
    with open(inp, "w") as f:
        f.write(f"{len(specs)}\n")
        for seed, N, outl in specs:
            posP, posQ, octP, octQ, poseP, poseQ = S.scene(np.random.default_rng(seed), N, outlier=outl)
            f.write(f"{N}\n" + " ".join(repr(float(v)) for v in (*poseP, *poseQ)) + "\n")
            for i in range(N):
                f.write(" ".join(repr(float(v)) for v in (*posP[i], *posQ[i])) + f" {int(octP[i])} {int(octQ[i])}\n")
    pkg = os.path.join(ROOT, "orb_slam2_ros2_amd")
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), "-I" + os.path.join(pkg, "host"),
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_sim3_dropin.cpp"), "-L" + pkg,
                           "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    r = subprocess.run([exe, str(inp), "create-only"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["created", "3"], (r.stdout + r.stderr)[-2000:]
