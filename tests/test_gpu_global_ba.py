"""orbfe_ba_global_optimize on the device: the conjugate-gradient solver alone (orbfe_debug_bsr_pcg, the systems and bounds of
tests/global_ba_cases.py), the block-CSR reduced system of one linearisation (orbfe_debug_ba_reduced_bsr) against the oracle's blocks,
and the optimiser against the oracle's one optimize(n)."""
import numpy as np
import pytest

import global_ba_cases as K
import global_ba_restatement as R
from orb_slam2_ros2_amd import ba_synth
from test_global_ba_host import CPU_CASES, pose_dist, trajectory

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from orb_slam2_ros2_amd._lib import Context
    c = Context(640, 480, n_features=500, max_images=1)
    yield c
    c.close()


# ---- the solver alone ---------------------------------------------------------------------------------------------------------------
def test_reference_converges_on_every_case():
    """the yardstick itself: the restatement's PCG converges on the whole table within the default cap of 4 * 6 * nb"""
    for case in K.TABLE:
        res, it, ok = K.reference(*case)
        assert ok == 1 and it <= 24 * K.pattern(case[0])[0] and res < 1e-9, (case, res, it, ok)


@pytest.mark.parametrize("shape,cond,scale", K.TABLE, ids=[f"{s}-{c:g}-{np.log2(x):+.0f}" for s, c, x in K.TABLE])
def test_pcg_meets_the_restatements_residual(ctx, shape, cond, scale):
    row_off, col, blocks, b = K.system(shape, cond, scale)
    x, it, ok = ctx.debug_bsr_pcg(row_off, col, blocks, b, tol=K.TOL)
    res = R.true_residual(row_off, col, blocks, b, x)
    ref_res, ref_it, _ = K.reference(shape, cond, scale)
    print(f"{shape} cond {cond:g} scale 2^{np.log2(scale):+.0f}: device {it} iterations, residual {res:.3e}; restatement {ref_it}, {ref_res:.3e}; "
          f"bound {K.residual_bound():.3e}")
    assert ok == 1 and np.isfinite(x).all()
    assert res <= K.residual_bound()
    assert it <= K.ITER_FACTOR * ref_it
    x1, it1, _ = ctx.debug_bsr_pcg(*K.system(shape, cond, 1.0), tol=K.TOL)
    assert it1 == it and x1.tobytes() == x.tobytes()                                # a relative stop: the iterates do not know the scale


def test_pcg_repeat_call_is_bit_identical(ctx):
    s = K.system("band", 1e6, 1.0)
    a, b = ctx.debug_bsr_pcg(*s, tol=K.TOL), ctx.debug_bsr_pcg(*s, tol=K.TOL)
    assert a[1] == b[1] and a[2] == b[2] == 1 and a[0].tobytes() == b[0].tobytes()


def test_pcg_zero_right_hand_side(ctx):
    row_off, col, blocks, b = K.system("star", 1e2, 1.0)
    x, it, ok = ctx.debug_bsr_pcg(row_off, col, blocks, np.zeros_like(b))
    assert ok == 1 and it == 0 and not x.any()


def test_pcg_indefinite_diagonal_block(ctx):
    row_off, col, blocks, b = K.system("star", 1e2, 1.0)
    rows = R.bsr_rows(row_off)
    q = int(np.flatnonzero((rows == 5) & (col == 5))[0])
    for value in (-1.0, 0.0, np.nan):
        bad = blocks.copy()
        bad[q, 2, 2] = value
        x, it, ok = ctx.debug_bsr_pcg(row_off, col, bad, b)
        assert ok == 0 and it == 0 and not x.any()
    assert ctx.debug_bsr_pcg(row_off, col, blocks, b)[2] == 1                       # the context is none the worse for it


def test_pcg_iteration_cap(ctx):
    s = K.system("band", 1e6, 1.0)
    x, it, ok = ctx.debug_bsr_pcg(*s, tol=K.TOL, max_iter=1)
    assert ok == 0 and it == 1 and np.isfinite(x).all() and x.any()
    ref = R.pcg(*s, K.TOL, 1)
    assert ref[2] == 0 and np.allclose(x, ref[0], rtol=1e-9, atol=1e-12 * np.abs(ref[0]).max())


def test_pcg_indefinite_system_breaks_down(ctx):
    """positive definite diagonal blocks, an indefinite matrix: p.Sp <= 0 stops the iteration, ok = 0"""
    row_off, col = np.array([0, 2, 4], np.int32), np.array([0, 1, 0, 1], np.int32)
    blocks = np.array([np.eye(6), 3 * np.eye(6), 3 * np.eye(6), np.eye(6)])
    x, it, ok = ctx.debug_bsr_pcg(row_off, col, blocks, np.concatenate([np.ones(6), -np.ones(6)]))
    assert ok == 0 and R.pcg(row_off, col, blocks, np.concatenate([np.ones(6), -np.ones(6)]))[2] == 0


def test_pcg_refuses_a_malformed_structure(ctx):
    from orb_slam2_ros2_amd._lib import OrbfeError
    blocks, b = np.array([np.eye(6), np.eye(6)]), np.ones(6)
    for row_off, col in (([0, 2], [0, 1]), ([0, 2], [0, 0]), ([0, 2], [0, -1])):
        with pytest.raises(OrbfeError):
            ctx.debug_bsr_pcg(np.array(row_off, np.int32), np.array(col, np.int32), blocks, b)


# ---- structure and values of the reduced system -------------------------------------------------------------------------------------
def test_reduced_bsr_structure_and_values(ctx, orc):
    pr = ba_synth.make_trajectory_problem(11, 60, 10, loop=3)
    fixed = np.zeros(60, np.uint8)
    fixed[:2] = 1
    lam = 0.37
    g = ctx.debug_ba_reduced_bsr(pr, fixed, lam)
    slot, free = R.slots(60, fixed)
    sym = R.bsr_symbolic(free.size, pr["points"].shape[0], pr["edge_pose"], pr["edge_point"], slot)
    assert np.array_equal(g["row_off"], sym["row_off"]) and np.array_equal(g["col"], sym["col"])
    rows = R.bsr_rows(g["row_off"])
    covis = {(i, i) for i in range(free.size)}
    for p in range(pr["points"].shape[0]):
        s = [int(slot[k]) for k in pr["edge_pose"][pr["edge_point"] == p] if slot[k] >= 0]
        covis |= {(a, b) for a in s for b in s}
    assert set(zip(rows.tolist(), g["col"].tolist())) == covis                      # the diagonal and both triangles among them
    assert any(abs(i - j) > 20 for i, j in covis)                                    # the loop blocks are there
    for q in range(g["col"].size):                                                   # symmetric to the bit
        assert g["blocks"][q].tobytes() == np.ascontiguousarray(g["blocks"][sym["twin"][q]].T).tobytes()
    sysm = orc.ba_build_system(pr["poses"], pr["points"], pr["edge_pose"], pr["edge_point"], pr["meas"], pr["is_stereo"], pr["info"],
                               pr["huber_delta"], pr["fx"], pr["fy"], pr["cx"], pr["cy"], pr["bf"], fixed)
    blocks, rhs = R.reduced_bsr(sym, sysm, lam, pr["edge_pose"], pr["edge_point"], slot, free)
    atol = 1e-12 * np.abs(sysm["Hpp"][free] + lam * np.eye(6)).max()
    print(f"blocks: max abs difference {np.abs(g['blocks'] - blocks).max():.3e} (atol {atol:.3e}); rhs {np.abs(g['rhs'] - rhs).max():.3e}")
    assert np.allclose(g["blocks"], blocks, rtol=1e-9, atol=atol)
    assert np.allclose(g["rhs"], rhs, rtol=1e-9, atol=1e-12 * np.abs(sysm["bp"]).max())


# ---- the optimiser --------------------------------------------------------------------------------------------------------------------
def _big():
    """171 free keyframes + 6 fixed: the size test_local_ba.py runs through the oracle"""
    pr = ba_synth.make_trajectory_problem(34, 177, 8, loop=3)
    fixed = np.zeros(177, np.uint8)
    fixed[:6] = 1
    truth = ba_synth.make_trajectory_problem(34, 177, 8, loop=3, with_truth=True)["poses_true"]
    pr["poses"][:6] = truth[:6]                                                      # the gauge: fixed keyframes sit at their true poses
    return pr, fixed


def _problem(name):
    return _big() if name == "177_six_fixed" else trajectory(name)


@pytest.mark.parametrize("name", list(CPU_CASES) + ["177_six_fixed"])
def test_sparse_solver_matches_the_oracle(ctx, orc, name):
    pr, fixed = _problem(name)
    g = ctx.ba_global_optimize(pr, fixed, 10, solver=2)
    o = orc.ba_local_optimize(pr, fixed, iters1=10, iters2=0)
    dp, dx = pose_dist(g["poses"], o["poses"]), np.abs(g["points"] - o["points"]).max()
    print(f"{name}: {g['iters']} iterations, cg_stats {tuple(g['cg_stats'])}; poses {dp:.2e}, points {dx:.2e}, "
          f"chi2 {np.abs(g['chi2'] - o['chi2']).max():.2e}")
    assert g["iters"] == o["iters"][0]
    assert dp < 1e-7 and dx < 1e-7
    assert np.allclose(g["chi2"], o["chi2"], rtol=1e-6, atol=1e-9)
    assert np.array_equal(g["poses"][fixed != 0], pr["poses"][fixed != 0])
    trials, cg, rejected = g["cg_stats"]
    assert trials >= g["iters"] and rejected == 0 and 0 < cg <= trials * 24 * int((fixed == 0).sum())
    again = ctx.ba_global_optimize(pr, fixed, 10, solver=2)
    assert all(np.array_equal(again[k], g[k]) for k in ("poses", "points", "chi2", "cg_stats")) and again["iters"] == g["iters"]


def test_sparse_solver_point_seen_twice_and_keyframe_without_edges(ctx, orc):
    """what the pair lists and the always-present diagonal are for: 25 observations doubled (a pose that sees a point twice puts four
    pairs into its diagonal block) and a free keyframe that lost all its edges (its block row is lambda I, its right-hand side 0)"""
    pr, fixed = trajectory("40_huber")
    keep = pr["edge_pose"] != 7
    twice = np.flatnonzero(keep)[::40][:25]
    pr = dict(pr)
    for k in ("edge_pose", "edge_point", "meas", "is_stereo", "info", "huber_delta"):
        pr[k] = np.concatenate([pr[k][keep], pr[k][twice]])
    pr["meas"][-25:, :2] += 0.25
    assert not (pr["edge_pose"] == 7).any()
    g = ctx.ba_global_optimize(pr, fixed, 10, solver=2)
    o = orc.ba_local_optimize(pr, fixed, iters1=10, iters2=0)
    dp, dx = pose_dist(g["poses"], o["poses"]), np.abs(g["points"] - o["points"]).max()
    print(f"seen twice, one keyframe bare: {g['iters']} iterations; poses {dp:.2e}, points {dx:.2e}")
    assert g["iters"] == o["iters"][0] and dp < 1e-7 and dx < 1e-7 and np.allclose(g["chi2"], o["chi2"], rtol=1e-6, atol=1e-9)
    assert np.array_equal(g["poses"][7], pr["poses"][7]) and g["cg_stats"][2] == 0      # nothing pulls on the bare keyframe


def test_dense_solver_is_the_local_ba(ctx):
    pr, fixed = trajectory("90_loop")
    g = ctx.ba_global_optimize(pr, fixed, 10, solver=1)
    l = ctx.ba_local_optimize(pr, fixed, 10, 0)
    assert g["iters"] == l["iters"][0] and not g["cg_stats"].any()
    assert all(g[k].tobytes() == l[k].tobytes() for k in ("poses", "points", "chi2"))


@pytest.mark.parametrize("n_free", [1000, 1001])
def test_auto_solver_follows_the_rule(ctx, n_free):
    from orb_slam2_ros2_amd import _lib, Optimizer
    assert _lib.GBA_DENSE_MAX_FREE == 1000                                           # the rule is a function of n_free alone
    pr = ba_synth.make_trajectory_problem(21, n_free + 1, 10, loop=3)
    fixed = np.zeros(n_free + 1, np.uint8)
    fixed[0] = 1
    named = 1 if n_free <= _lib.GBA_DENSE_MAX_FREE else 2
    a, b = Optimizer.globalOptimization(ctx, pr, fixed, 10), ctx.ba_global_optimize(pr, fixed, 10, solver=named)
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("poses", "points", "chi2", "cg_stats")) and a["iters"] == b["iters"]
    assert bool(a["cg_stats"].any()) == (named == 2)


@pytest.mark.parametrize("solver", [1, 2])
def test_stop_flag_set_before_the_call(ctx, solver):
    pr, fixed = trajectory("40_huber")
    g = ctx.ba_global_optimize(pr, fixed, 10, solver=solver, stop=np.ones(1, np.uint8))
    assert g["iters"] == 0 and np.array_equal(g["poses"], pr["poses"]) and np.array_equal(g["points"], pr["points"])


def test_all_keyframes_fixed_moves_only_points(ctx, orc):
    pr, _ = trajectory("40_huber")
    fixed = np.ones(40, np.uint8)
    g = ctx.ba_global_optimize(pr, fixed, 10, solver=2)
    o = orc.ba_local_optimize(pr, fixed, iters1=10, iters2=0)
    assert np.array_equal(g["poses"], pr["poses"]) and not np.array_equal(g["points"], pr["points"])
    assert g["iters"] == o["iters"][0] and np.abs(g["points"] - o["points"]).max() < 1e-7 and g["cg_stats"][1] == 0


def test_no_edges_returns_the_inputs_and_bad_arguments_are_refused(ctx):
    from orb_slam2_ros2_amd._lib import OrbfeError
    pr, fixed = trajectory("40_huber")
    e = dict(pr)
    for k in ("edge_pose", "edge_point", "is_stereo", "info", "huber_delta"):
        e[k] = pr[k][:0]
    e["meas"] = pr["meas"][:0]
    for solver in (0, 1, 2):
        g = ctx.ba_global_optimize(e, fixed, 10, solver=solver)
        assert np.array_equal(g["poses"], pr["poses"]) and np.array_equal(g["points"], pr["points"])
    bad = dict(pr)
    bad["edge_point"] = pr["edge_point"].copy()
    bad["edge_point"][3] = pr["points"].shape[0]
    for call in (lambda: ctx.ba_global_optimize(bad, fixed, 10, solver=2), lambda: ctx.ba_global_optimize(pr, fixed, 10, solver=3),
                 lambda: ctx.ba_global_optimize(pr, fixed, -1, solver=2), lambda: ctx.debug_ba_reduced_bsr(bad, fixed, 1.0)):
        with pytest.raises(OrbfeError):
            call()


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_dropin_over_minimal_types(ctx, tmp_path):
    """tests/cpp/test_global_ba_dropin.cpp, the whole function: the graph the drop-in builds goes through the Python binding in the same
    way; mTcwGBA and mPGBA of every vertex are that result as float, and nothing that is no vertex gets either."""
    import os
    import subprocess
    import global_ba_dropin_scene as S
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text, want = S.scene(True)
    inp = tmp_path / "in.txt"
    inp.write_text(text)
    exe = str(tmp_path / "t")
    subprocess.check_call(S.build_command(root, exe), timeout=300)
    r = subprocess.run([exe, str(inp), "full"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    got = S.parse(r.stdout)
    g = ctx.ba_global_optimize(got["problem"], np.array(got["fixed"], np.uint8), 10)
    assert g["iters"] == 10 and got["kf_ids"] == want["kf_ids"]
    for k in range(want["n_kf"]):
        T = got["gba"][k]
        if k not in got["kf_ids"]:
            assert T is None                                                         # the bad keyframe, the one that is not in vpKfs
            continue
        p = g["poses"][got["kf_ids"].index(k)]
        assert np.allclose(T[:3, :3], _rot(p[:4]), rtol=0, atol=2e-6) and np.allclose(T[:3, 3], p[4:], rtol=0, atol=2e-6)
        assert T[3].tolist() == [0, 0, 0, 1]
    assert np.array_equal(got["gba"][0][:3, 3], np.zeros(3, np.float32))            # keyframe 0 is fixed: where it was
    moved = 0
    for m in range(want["n_mp"]):
        if m not in got["lm_index"]:
            assert got["pgba"][m] is None                                            # the bad map point
            continue
        v = got["lm_index"].index(m)
        assert got["pgba"][m].tobytes() == g["points"][v].astype(np.float32).tobytes()
        moved += int(not np.array_equal(got["pgba"][m], got["problem"]["points"][v].astype(np.float32)))
    for m in (S.BARE_MP, S.ORPHAN_MP):                                               # no usable observation: a vertex that stays put
        assert got["pgba"][m].tobytes() == got["problem"]["points"][got["lm_index"].index(m)].astype(np.float32).tobytes()
    assert moved >= 30


def test_a_starved_solver_rejects_its_trials(ctx):
    """pcg_max_iter = 1: a trial whose system one iteration does not solve is rejected as a bad pivot would be and leaves the estimates
    where they were; lambda grows with every rejection until the damped system is block-diagonal enough for one iteration, so the run
    goes on -- slower, never wrong."""
    pr, fixed = trajectory("40_huber")
    g = ctx.ba_global_optimize(pr, fixed, 10, solver=2, pcg_max_iter=1)
    trials, cg, rejected = g["cg_stats"]
    print(f"starved: {g['iters']} iterations, {trials} trials, {rejected} rejected by the solver")
    assert rejected >= 1 and cg == trials > rejected and 1 <= g["iters"] <= 10
    assert np.isfinite(g["poses"]).all() and np.isfinite(g["points"]).all() and np.array_equal(g["poses"][0], pr["poses"][0])
    again = ctx.ba_global_optimize(pr, fixed, 10, solver=2, pcg_max_iter=1)
    assert all(np.array_equal(again[k], g[k]) for k in ("poses", "points", "chi2", "cg_stats"))
