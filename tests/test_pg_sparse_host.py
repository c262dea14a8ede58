"""The block-sparse pose-graph solver without a GPU: the symbolic phase (csrc/pg_symbolic.h) and the 6x6 block arithmetic the
kernel shares with the host (csrc/pg_chol_dev.h) in a stand-alone program under the host sanitizers, against a plain restatement of
elimination tree and fill (tests/essential_graph_sparse_cases.symbolic) and against numpy; the far-edge family's generator and its
qualification table; the header, the library and the binding."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import essential_graph_cases as K
import essential_graph_sparse_cases as S
import sim3_opt_restatement as s3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/cpp/test_pg_symbolic.cpp: a stand-alone program with its own main; nothing of it is loaded into python"""
    exe = str(tmp_path_factory.mktemp("pgs") / "t")
    base = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "orb_slam2_ros2_amd", "csrc"),
            "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_pg_symbolic.cpp")]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        # only a g++ WITHOUT the sanitizers' runtimes (the link step cannot find libasan / libubsan) may run the program plain
        assert re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S* ?: No such file", r.stderr), r.stderr[-3000:]
        subprocess.check_call(base, timeout=300)
    return exe


def _run(program, nb, pairs, system=None):
    text = [f"{nb} {len(pairs)} {0 if system is None else len(system[0])}"] + [f"{i} {j}" for i, j in pairs]
    if system is not None:
        low_row, low_col, blocks, rhs = system
        text += [f"{r} {c} " + " ".join(repr(float(v)) for v in b) for r, c, b in zip(low_row, low_col, blocks)]
        text.append(" ".join(repr(float(v)) for v in rhs))
    r = subprocess.run([program], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, (r.stdout[-500:] + r.stderr)[-3000:])
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        out[w[0]] = np.array([float.fromhex(v) for v in w[1:]]) if w[0] in ("L", "x") else np.array(w[1:], np.int64)
    return out


def _patterns():
    rng = np.random.default_rng(11)
    out = {
        "one row": (1, []),
        "two rows": (2, [(1, 0)]),
        "tridiagonal": (3, [(1, 0), (2, 1)]),
        "12 with a far block": (12, [(k + 1, k) for k in range(11)] + [(11, 0)]),
        "rows with no off-diagonal block": (5, [(1, 0), (3, 1)]),
        "hub first": (40, [(k, 0) for k in range(1, 40)]),
        "hub last": (40, [(39, k) for k in range(39)]),
        "either orientation, twice": (6, [(0, 3), (3, 0), (5, 1), (1, 5), (2, 1), (0, 3)]),
    }
    for n in (7, 12, 99, 257):
        out[f"far-edge family {n}"] = S.lower_pattern(S.graph(n))
    for k, (nb, density) in enumerate(((9, 0.3), (30, 0.1), (64, 0.05), (150, 0.02))):
        m = rng.random((nb, nb)) < density
        out[f"random {nb}"] = (nb, [(int(i), int(j)) if rng.random() < 0.5 else (int(j), int(i)) for i in range(nb) for j in range(i) if m[i, j]])
    return out


@pytest.mark.parametrize("name", list(_patterns()))
def test_symbolic_and_host_factorisation(program, name):
    """the structure against the restatement, array by array, and its rules; then Hpp-shaped numbers through the header's block
    arithmetic over that structure: the factor against numpy.linalg.cholesky, the solution against numpy.linalg.solve.  Bound: 1e-12
    relative to the largest entry (diagonally dominant systems, condition numbers of a few hundred: measured 2e-15)."""
    nb, pairs = _patterns()[name]
    low = sorted({(max(i, j), min(i, j)) for i, j in pairs})
    parent, rows = S.symbolic(nb, low)
    low_row, low_col, blocks, A, rhs = S.spd_system(nb, low, seed=5)
    got = _run(program, nb, pairs, (low_row, low_col, blocks, rhs))
    col_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    assert np.array_equal(got["parent"], parent) and np.array_equal(got["col_off"], col_off)
    assert np.array_equal(got["row"], np.concatenate(rows)) if nb else True
    mc, ss = int(got["max_col"][0]), int(got["search_steps"][0])
    assert mc == max(len(r) for r in rows) and 2 ** ss >= mc and (ss == 0 or 2 ** (ss - 1) < mc)
    # the rules themselves, on the program's output: the diagonal first, rows ascending; parent = the first row below the diagonal; the
    # rows of a column below its parent are rows of the parent's column; every block of the matrix has its place
    for k in range(nb):
        r = got["row"][col_off[k]:col_off[k + 1]]
        assert r[0] == k and np.all(np.diff(r) > 0)
        assert got["parent"][k] == (r[1] if len(r) > 1 else -1)
        if len(r) > 2:
            p = r[1]
            assert set(r[2:]) <= set(got["row"][col_off[p]:col_off[p + 1]])
    for (i, j), p in zip(pairs, got["pos"]):
        i, j = max(i, j), min(i, j)
        assert col_off[j] < p < col_off[j + 1] and got["row"][p] == i
    if name == "hub first":
        assert col_off[-1] == 40 * 41 // 2                                      # the factor fills completely
    if name in ("hub last", "tridiagonal", "two rows"):
        assert col_off[-1] == nb + len(low)                                     # no fill
    if name == "far-edge family 257":
        assert col_off[-1] > nb + len(low) and got["max_col"][0] == 8
    # the numbers
    assert got["ok"][0] == 1
    Lref = np.linalg.cholesky(A)
    scale = np.abs(Lref).max()
    worst = 0.0
    for k in range(nb):
        for q in range(col_off[k], col_off[k + 1]):
            i = got["row"][q]
            B = got["L"][36 * q:36 * q + 36].reshape(6, 6)
            want = Lref[6 * i:6 * i + 6, 6 * k:6 * k + 6]
            d = np.abs(np.tril(B) - want) if i == k else np.abs(B - want)      # (above a diagonal block's diagonal nothing is defined)
            worst = max(worst, float(d.max()))
    xs = np.linalg.solve(A, rhs)
    dx = float(np.abs(got["x"] - xs).max())
    print(f"{name}: {col_off[-1]} blocks, longest column {got['max_col'][0]}; max |L - numpy| {worst:.2e} of {scale:.2e}, max |x - numpy| {dx:.2e}")
    assert worst <= 1e-12 * scale and dx <= 1e-12 * max(1.0, np.abs(xs).max())


def test_host_factorisation_reports_a_bad_pivot(program):
    nb, low = 12, [(k + 1, k) for k in range(11)] + [(11, 0)]
    low_row, low_col, blocks, A, rhs = S.spd_system(nb, low, seed=3)
    for bad in (-1.0, float("nan"), 0.0):
        b = blocks.copy()
        b[nb - 1, 35] = bad if bad != 0.0 else -1e6                             # the last diagonal entry of the system
        assert _run(program, nb, low, (low_row, low_col, b, rhs))["ok"][0] == 0


def test_far_edge_family():
    """the generator: the existing family untouched in front, far edges between non-fixed vertices behind it, one pair in both
    orientations, every measurement the relative pose of `true`; the chain replayed here reproduces the existing generator's
    measurements bit for bit; 1025 block rows have the counts the issue states"""
    for n in S.SIZES + (S.BIG,):
        g, g0 = S.graph(n), K.make_graph(n)
        ne0 = len(g0["edges"])
        assert np.array_equal(g["edges"][:ne0], g0["edges"]) and g["meas"][:ne0].tobytes() == g0["meas"].tobytes()
        assert g["estimates"].tobytes() == g0["estimates"].tobytes() and g["far"] == list(range(ne0, len(g["edges"])))
        for (a, b), m in zip(g["edges"], g["meas"]):
            C = s3.sim3_mul(tuple(g["true"][b]), s3.sim3_inverse(tuple(g["true"][a])))
            assert np.array(C[:7] + (1.0,)).tobytes() == m.tobytes()
        fx = g["fixed"].astype(bool)
        for e in g["far"]:
            a, b = g["edges"][e]
            assert not fx[a] and not fx[b] and g["isolated"] not in (a, b)
        if n >= 12:
            e = [tuple(x) for x in g["edges"][g["far"]]]
            assert len(e) >= 3 and e[1] == e[0][::-1]
        nb, pairs = S.lower_pattern(g)
        rows = S.symbolic(nb, pairs)[1]
        if n >= 7:
            assert sum(len(r) for r in rows) > nb + len(pairs)                  # the factor has fill
        if n == S.BIG:
            assert (len(pairs), sum(len(r) - 1 for r in rows), max(len(r) - 1 for r in rows)) == (3068, 7132, 7)
            nb0, pairs0 = S.lower_pattern(g0)
            assert sum(len(r) - 1 for r in S.symbolic(nb0, pairs0)[1]) == len(pairs0) == 3064   # the existing family: no fill at all


def test_closed_form_minimum_has_zero_error():
    import essential_graph_restatement as R
    for n in (12, 99):
        g = S.graph(n)
        want = S.closed_form_minimum(g)
        assert R.edge_chi2(R.errors(R.Graph(*K.args(g)), want)).sum() < 1e-25
        assert want[g["isolated"]].tobytes() == g["estimates"][g["isolated"]].tobytes()
        ref = S.reference(n, S.CONV[n][0])
        assert np.abs(S.align_sign(ref["est"], want) - want).max() < 1e-12      # and the restatement converges to it


@pytest.mark.parametrize("n", S.SIZES + (S.BIG,))
def test_far_edge_cases_are_qualified(n):
    """the tables of tests/essential_graph_sparse_cases.py recomputed with essential_graph_cases.qualify(), by that module's convention:
    the bound is 1e-6 where the restatement's own spread is <= 1e-8, otherwise 100 x the spread.  At 1025 one iteration is run (two
    restatement runs of 6 s each): its spread admits it; what the second iteration does there is in the cases module."""
    k_max = 1 if n == S.BIG else S.CONV[n][0] + 1
    k_adm, d_adm, k_conv, d_conv, a, b = S.qualify(n, k_max)
    print(f"n_free {n}: admitted {k_adm} iterations (difference {d_adm:.2e}), converged {k_conv} (difference {d_conv:.2e})")
    # (the spreads are rounding noise of the two runs: they may come out up to 3 x the recorded figure under another BLAS; the prefix
    #  lengths may not come out shorter)
    assert k_adm == S.ADM[n][0] and d_adm <= 3 * S.ADM[n][1] + 1e-15
    assert S.ADM[n][2] == (K.BOUND if S.ADM[n][1] <= K.QUAL_DIFF else 100 * S.ADM[n][1])
    if n == S.BIG:
        return
    assert k_conv >= S.CONV[n][0]
    k_conv = S.CONV[n][0]
    d_conv = float(np.abs(a["est_after"][k_conv - 1] - b["est_after"][k_conv - 1]).max())
    assert d_conv <= K.QUAL_DIFF and d_conv <= 3 * S.CONV[n][1] + 1e-15
    assert a["chis"][0] >= S.MIN_REDUCTION * a["chis"][sum(acc for acc, it in zip(a["accepts"], a["trial_iter"]) if it < k_conv)]


def test_header_library_and_binding_agree():
    from orb_slam2_ros2_amd import _lib, Optimizer
    import inspect
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)                       # loading must not need a GPU
    for name in ("orbfe_pose_graph_optimize_ex", "orbfe_debug_pg_sparse_solve"):
        assert re.search(r"orbfe_status\s+" + name + r"\(", hdr), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert "typedef struct orbfe_pose_graph_options" in hdr
    assert re.search(r"#define ORBFE_ABI_VERSION (\d+)", hdr).group(1) == "4" and lib.orbfe_abi_version() == 4
    assert re.search(r"#define ORBFE_PG_MAX_FREE (\d+)", hdr).group(1) == "1024" and _lib.PG_MAX_FREE == 1024
    assert int(re.search(r"#define ORBFE_PG_SPARSE_MIN_FREE (\d+)", hdr).group(1)) >= 8
    assert "solver" in inspect.signature(_lib.Context.pose_graph_optimize).parameters
    assert "solver" in inspect.signature(Optimizer.optimizeEssentialGraph).parameters
    shim = open(os.path.join(ROOT, "orb_slam2_ros2_amd", "host", "orbfe_shim.hpp")).read()
    dropin = open(os.path.join(ROOT, "orb_slam2_ros2_amd", "host", "orbfe_essential_dropin.hpp")).read()
    assert "orbfe_pose_graph_optimize_ex(" in shim and re.search(r"optimizeEssentialGraph\(solverContext\(2\)[^;]*nullptr, 0\);", dropin)


def test_ex_refusals_need_no_context():
    """the argument checks come first: without a context every call is ORBFE_EBADARG, whatever else it carries"""
    from orb_slam2_ros2_amd import _lib
    lib = _lib.load()
    g = S.graph(7)
    pg, keep = _lib.Context._pose_graph(*K.args(g))
    out, chi, stats = g["estimates"].copy(), np.zeros(len(g["edges"])), np.full(4, -3, np.int32)
    for solver in (0, 1, 2, 7):
        opt = _lib.PoseGraphOptions(solver)
        assert lib.orbfe_pose_graph_optimize_ex(None, ctypes.byref(pg), 20, ctypes.byref(opt), _lib.ptr(out), _lib.ptr(chi), _lib.ptr(stats)) == 1
    rows, x, ok = np.zeros(1, np.int32), np.zeros(6), ctypes.c_int32(-5)
    assert lib.orbfe_debug_pg_sparse_solve(None, 1, 1, _lib.ptr(rows), _lib.ptr(rows), _lib.ptr(np.eye(6)), _lib.ptr(x), _lib.ptr(x), ctypes.byref(ok), None) == 1
    assert (stats == -3).all() and not chi.any() and out.tobytes() == g["estimates"].tobytes() and ok.value == -5
