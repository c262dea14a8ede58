"""The g2o part of Optimizer::OptimizeLocalMap (Optimizer.cc:336-391): oracle known answers (CPU) and the device solver against the
oracle (GPU).  north_star asks for 1e-4 on BA pose residuals; device and oracle run the same Levenberg-Marquardt trajectory and
differ by summation order only, so 1e-7 is asserted on poses and points."""
import numpy as np
import pytest

from orb_slam2_ros2_amd import ba_synth


def _problem(seed, n_kf, n_pt, n_fixed=2):
    pr = ba_synth.make_problem(seed=seed, n_kf=n_kf, n_pt=n_pt, with_truth=True)
    fixed = np.zeros(n_kf, np.uint8)
    fixed[:n_fixed] = 1
    pr["poses"][:n_fixed] = pr["poses_true"][:n_fixed]      # the gauge: fixed keyframes sit at their true poses
    return pr, fixed


def _pose_dist(a, b):
    """max abs difference of (q, t) with the quaternion sign fixed"""
    s = np.sign((a[:, :4] * b[:, :4]).sum(1, keepdims=True))
    return max(np.abs(a[:, :4] - s * b[:, :4]).max(), np.abs(a[:, 4:] - b[:, 4:]).max())


def test_oracle_local_ba_converges_and_excludes_the_planted_outliers(orc):
    pr, fixed = _problem(3, 12, 400)
    r = orc.ba_local_optimize(pr, fixed)
    assert tuple(r["iters"]) == (5, 10)
    assert _pose_dist(r["poses"], pr["poses_true"]) < 0.75 * _pose_dist(pr["poses"], pr["poses_true"])
    assert np.median(np.abs(r["points"] - pr["points_true"])) < 0.75 * np.median(np.abs(pr["points"] - pr["points_true"]))
    assert np.array_equal(r["poses"][:2], pr["poses"][:2])                    # setFixed(true)
    e0 = orc.ba_eval_edges(pr["poses"], pr["points"], pr["edge_pose"], pr["edge_point"], pr["meas"], pr["is_stereo"], pr["info"],
                           pr["huber_delta"], pr["fx"], pr["fy"], pr["cx"], pr["cy"], pr["bf"])
    assert np.median(r["chi2"]) < 0.2 * np.median(e0["chi2"])
    # level 1 = the edges the first round could not explain; every surviving gross outlier (35 px) is among them
    th = np.where(pr["is_stereo"] != 0, 7.815, 5.991)
    assert r["level"].sum() > 0 and (r["chi2"][r["level"] == 0] > 50 * th[r["level"] == 0]).sum() == 0
    assert np.array_equal(r["bad"].astype(bool), (r["chi2"] > th) | (r["bad"].astype(bool) & (r["chi2"] <= th)))
    assert np.allclose(np.linalg.norm(r["poses"][:, :4], axis=1), 1, atol=1e-12) and (r["poses"][:, 3] >= 0).all()


def test_oracle_local_ba_degenerate_inputs(orc):
    pr, fixed = _problem(4, 6, 60)
    # zero iterations: nothing moves, but the classification and the final test still run
    r = orc.ba_local_optimize(pr, fixed, iters1=0, iters2=0)
    assert np.array_equal(r["poses"], pr["poses"]) and np.array_equal(r["points"], pr["points"]) and tuple(r["iters"]) == (0, 0)
    # every keyframe fixed: only the points move (structure-only BA)
    allf = np.ones(6, np.uint8)
    r = orc.ba_local_optimize(pr, allf)
    assert np.array_equal(r["poses"], pr["poses"]) and not np.array_equal(r["points"], pr["points"])
    # no edges at all
    e = dict(pr)
    for k in ("edge_pose", "edge_point", "is_stereo", "info", "huber_delta"):
        e[k] = pr[k][:0]
    e["meas"] = pr["meas"][:0]
    r = orc.ba_local_optimize(e, fixed)
    assert np.array_equal(r["poses"], pr["poses"]) and np.array_equal(r["points"], pr["points"])


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_kf,n_pt,n_fixed", [(3, 12, 400, 2), (5, 30, 1500, 5), (6, 60, 3000, 20), (7, 8, 100, 8)])
def test_device_local_ba_matches_oracle(orc, seed, n_kf, n_pt, n_fixed):
    from orb_slam2_ros2_amd._lib import Context
    from orb_slam2_ros2_amd import Optimizer
    pr, fixed = _problem(seed, n_kf, n_pt, n_fixed)
    ctx = Context(640, 480, n_features=500, max_images=1)
    g = Optimizer.OptimizeLocalMap(ctx, pr, fixed)
    o = orc.ba_local_optimize(pr, fixed)
    assert tuple(g["iters"]) == tuple(o["iters"])
    assert _pose_dist(g["poses"], o["poses"]) < 1e-7 and np.abs(g["points"] - o["points"]).max() < 1e-7
    assert np.array_equal(g["poses"][:n_fixed], pr["poses"][:n_fixed])
    assert (g["level"] != o["level"]).sum() <= 1 and (g["bad"] != o["bad"]).sum() <= 1   # an edge exactly on a threshold may flip
    assert np.allclose(g["chi2"], o["chi2"], rtol=1e-6, atol=1e-9)
    again = ctx.ba_local_optimize(pr, fixed)
    assert all(np.array_equal(again[k], g[k]) for k in ("poses", "points", "level", "chi2", "bad"))   # fixed summation orders
    ctx.close()


@pytest.mark.gpu
def test_device_local_ba_host_driven_loop_agrees(monkeypatch):
    """ORBFE_LBA_HOST_LM=1: round 2's host-driven Levenberg-Marquardt loop (still the path when a pose observes a point twice) against
    the default (control on the device): same iterations, results to rounding -- the factorisation kernels differ.  (The switch is read
    at orbfe_create.)"""
    from orb_slam2_ros2_amd._lib import Context
    pr, fixed = _problem(6, 60, 3000, 20)
    ctx = Context(640, 480, n_features=500, max_images=1)
    ref = ctx.ba_local_optimize(pr, fixed)
    ctx.close()
    monkeypatch.setenv("ORBFE_LBA_HOST_LM", "1")
    ctx = Context(640, 480, n_features=500, max_images=1)
    got = ctx.ba_local_optimize(pr, fixed)
    ctx.close()
    assert tuple(got["iters"]) == tuple(ref["iters"])
    assert np.abs(got["poses"] - ref["poses"]).max() < 1e-9 and np.abs(got["points"] - ref["points"]).max() < 1e-9
    assert (got["level"] != ref["level"]).sum() <= 1


def _assert_matches_oracle(g, o, pr, fixed):
    """the asserts of test_device_local_ba_matches_oracle"""
    n_fixed = int(fixed.sum())
    assert tuple(g["iters"]) == tuple(o["iters"])
    assert _pose_dist(g["poses"], o["poses"]) < 1e-7 and np.abs(g["points"] - o["points"]).max() < 1e-7
    assert np.array_equal(g["poses"][:n_fixed], pr["poses"][:n_fixed])
    assert (g["level"] != o["level"]).sum() <= 1 and (g["bad"] != o["bad"]).sum() <= 1   # an edge exactly on a threshold may flip
    assert np.allclose(g["chi2"], o["chi2"], rtol=1e-6, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_free,n_pt,n_fixed", [(31, 43, 1500, 4), (32, 100, 2000, 5), (33, 101, 2000, 5), (34, 171, 2500, 6)])
def test_device_local_ba_host_driven_loop_sizes(orc, monkeypatch, seed, n_free, n_pt, n_fixed):
    """ORBFE_LBA_HOST_LM=1 at the sizes the host-driven loop's two solvers were built for: the LDS-resident Cholesky up to its limit of 100
    free keyframes (43, 100), the panel solver past it (101; 171: 1026 unknowns, the 1024-thread row loops take a second trip).  Which
    solver runs is a function of the inputs alone: the switch and the number of free keyframes.  (The switch is read at orbfe_create.)"""
    from orb_slam2_ros2_amd._lib import Context
    pr, fixed = _problem(seed, n_free + n_fixed, n_pt, n_fixed)
    assert (fixed == 0).sum() == n_free and (n_free <= 100) == (n_free in (43, 100))     # <= 100: k_lba_chol_solve, else the panel solver
    monkeypatch.setenv("ORBFE_LBA_HOST_LM", "1")
    ctx = Context(640, 480, n_features=500, max_images=1)
    g = ctx.ba_local_optimize(pr, fixed)
    again = ctx.ba_local_optimize(pr, fixed)
    ctx.close()
    _assert_matches_oracle(g, orc.ba_local_optimize(pr, fixed), pr, fixed)
    assert all(np.array_equal(again[k], g[k]) for k in ("poses", "points", "level", "chi2", "bad"))   # fixed summation orders


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_free,n_pt,n_fixed", [(35, 45, 1500, 4), (36, 105, 2000, 5)])
def test_device_local_ba_duplicate_edges_past_42_and_100(orc, seed, n_free, n_pt, n_fixed):
    """How production reaches the host-driven loop and its solvers: a pose that observes a point twice (no environment switch).  45 free
    keyframes: past the register-resident solver of the device-side control, the LDS solver here; 105: the panel solver."""
    from orb_slam2_ros2_amd._lib import Context
    pr, fixed = _problem(seed, n_free + n_fixed, n_pt, n_fixed)
    pr, fixed = _mutate(pr, fixed, "duplicate_edges", np.random.default_rng(seed))
    obs = np.stack([pr["edge_pose"], pr["edge_point"]], 1)
    assert len(np.unique(obs, axis=0)) < len(obs)             # the premise: at least one pose observes a point twice
    assert (fixed == 0).sum() == n_free
    ctx = Context(640, 480, n_features=500, max_images=1)
    g = ctx.ba_local_optimize(pr, fixed)
    ctx.close()
    _assert_matches_oracle(g, orc.ba_local_optimize(pr, fixed), pr, fixed)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["device_control", "host_lm", "duplicate_edges"])
def test_device_local_ba_rejects_trials(orc, monkeypatch, path):
    """The reject rule of lm_ctrl.h in the control kernel (k_lm_ctrl) and in the host loop (lm_host.h; reached by ORBFE_LBA_HOST_LM=1
    and, as production reaches it, by a pose that observes a point twice) on 4 keyframes and 40 points whose start is 3 m (sigma) from
    the optimum: 8 iterations of the first round, none of the second.  The premise comes from the oracle's own count: 12 trials for the
    8 iterations (10 with the doubled edges).  Chosen on the CPU so that no gain ratio of the oracle's run is within 0.4 of 0: no last
    bit decides a trial.  Asserts of test_device_local_ba_matches_oracle, and the same bytes on a second call."""
    from orb_slam2_ros2_amd._lib import Context
    pr, fixed = _problem(2, 4, 40, 1)
    pr["points"] = pr["points"] + np.random.default_rng(2).normal(size=pr["points"].shape) * 3.0
    if path == "duplicate_edges":
        pr, fixed = _mutate(pr, fixed, "duplicate_edges", np.random.default_rng(2))
        obs = np.stack([pr["edge_pose"], pr["edge_point"]], 1)
        assert len(np.unique(obs, axis=0)) < len(obs)
    o = orc.ba_local_optimize(pr, fixed, 8, 0)
    assert (tuple(o["iters"]), tuple(o["trials"])) == ((8, 0), (10 if path == "duplicate_edges" else 12, 0))
    if path == "host_lm":
        monkeypatch.setenv("ORBFE_LBA_HOST_LM", "1")
    ctx = Context(640, 480, n_features=500, max_images=1)
    g = ctx.ba_local_optimize(pr, fixed, 8, 0)
    again = ctx.ba_local_optimize(pr, fixed, 8, 0)
    ctx.close()
    print(f"local BA {path}: poses {_pose_dist(g['poses'], o['poses']):.2e}, points {np.abs(g['points'] - o['points']).max():.2e}")
    _assert_matches_oracle(g, o, pr, fixed)
    assert all(np.array_equal(again[k], g[k]) for k in ("poses", "points", "level", "chi2", "bad"))


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_kf,n_pt,n_fixed", [(14, 48, 2000, 5), (15, 74, 3000, 10), (11, 155, 2500, 5), (12, 101, 1500, 0), (13, 310, 4000, 10)])
def test_device_local_ba_beyond_100_free_keyframes(orc, seed, n_kf, n_pt, n_fixed):
    """Optimizer::OptimizeLocalMap takes every keyframe covisible with the current one (getConnectedKfs(0), Optimizer.cc:232): no bound.
    Past 42 free keyframes the reduced system is factorised by the blocked multi-workgroup Cholesky (k_lmbig.hip, fp64 MFMA) under the
    same device-side control: 43 (the first size past the register-resident solver), 64, 150, 101 with no fixed frame (the gauge is
    free, as g2o would run it) and 300 free keyframes."""
    from orb_slam2_ros2_amd._lib import Context
    pr, fixed = _problem(seed, n_kf, n_pt, n_fixed)
    assert (fixed == 0).sum() > 42
    ctx = Context(640, 480, n_features=500, max_images=1)
    g = ctx.ba_local_optimize(pr, fixed)
    o = orc.ba_local_optimize(pr, fixed)
    assert tuple(g["iters"]) == tuple(o["iters"])
    assert _pose_dist(g["poses"], o["poses"]) < 1e-7 and np.abs(g["points"] - o["points"]).max() < 1e-7
    assert (g["level"] != o["level"]).sum() <= 1 and (g["bad"] != o["bad"]).sum() <= 1
    again = ctx.ba_local_optimize(pr, fixed)
    assert all(np.array_equal(again[k], g[k]) for k in ("poses", "points", "level", "chi2", "bad"))
    ctx.close()


@pytest.mark.gpu
def test_device_local_ba_edge_cases(orc):
    from orb_slam2_ros2_amd._lib import Context, OrbfeError
    pr, fixed = _problem(4, 6, 60)
    ctx = Context(640, 480, n_features=500, max_images=1)
    g = ctx.ba_local_optimize(pr, fixed, 0, 0)
    o = orc.ba_local_optimize(pr, fixed, iters1=0, iters2=0)
    assert np.array_equal(g["poses"], pr["poses"]) and np.array_equal(g["level"], o["level"]) and np.array_equal(g["bad"], o["bad"])
    allf = np.ones(6, np.uint8)
    g, o = ctx.ba_local_optimize(pr, allf), orc.ba_local_optimize(pr, allf)
    assert np.array_equal(g["poses"], pr["poses"]) and np.abs(g["points"] - o["points"]).max() < 1e-7
    bad = dict(pr)
    bad["edge_pose"] = pr["edge_pose"].copy()
    bad["edge_pose"][3] = 99
    with pytest.raises(OrbfeError):
        ctx.ba_local_optimize(bad, fixed)
    ctx.close()


def _mutate(pr, fixed, kind, rng):
    """structural corner cases of the graph the reference can produce"""
    pr = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in pr.items()}
    fixed = fixed.copy()
    E = len(pr["edge_pose"])
    if kind == "mono_only":
        pr["is_stereo"][:] = 0
        pr["meas"][:, 2] = -1.0
        pr["info"][:] = np.sqrt(pr["info"])                      # quirk Q9: mono edges carry invSigma
        pr["huber_delta"][:] = float(np.float32(np.sqrt(5.991)))
    elif kind == "free_pose_without_edges":
        k = int(np.flatnonzero(fixed == 0)[0])
        keep = pr["edge_pose"] != k
        for name in ("edge_pose", "edge_point", "meas", "is_stereo", "info", "huber_delta"):
            pr[name] = pr[name][keep]
    elif kind == "points_seen_by_fixed_poses_only":
        # make some points fixed-only by removing their free-pose edges
        victims = np.unique(pr["edge_point"])[:25]
        keep = ~(np.isin(pr["edge_point"], victims) & (fixed[pr["edge_pose"]] == 0))
        for name in ("edge_pose", "edge_point", "meas", "is_stereo", "info", "huber_delta"):
            pr[name] = pr[name][keep]
    elif kind == "duplicate_edges":
        dup = rng.integers(0, E, 50)
        for name in ("edge_pose", "edge_point", "meas", "is_stereo", "info", "huber_delta"):
            pr[name] = np.concatenate([pr[name], pr[name][dup]])
    elif kind == "far_start":
        pr["poses"][fixed == 0, 4:] += rng.normal(0, 0.15, ((fixed == 0).sum(), 3))     # several rejected LM trials
    return pr, fixed


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mono_only", "free_pose_without_edges", "points_seen_by_fixed_poses_only", "duplicate_edges", "far_start"])
def test_device_local_ba_structural_cases(orc, kind):
    from orb_slam2_ros2_amd._lib import Context
    rng = np.random.default_rng(11)
    pr, fixed = _problem(9, 10, 300, 3)
    pr, fixed = _mutate(pr, fixed, kind, rng)
    ctx = Context(640, 480, n_features=500, max_images=1)
    g = ctx.ba_local_optimize(pr, fixed)
    o = orc.ba_local_optimize(pr, fixed)
    assert tuple(g["iters"]) == tuple(o["iters"]), kind
    assert _pose_dist(g["poses"], o["poses"]) < 1e-7 and np.abs(g["points"] - o["points"]).max() < 1e-7, kind
    assert (g["level"] != o["level"]).sum() <= 1 and (g["bad"] != o["bad"]).sum() <= 1
    ctx.close()


@pytest.mark.gpu
def test_device_local_ba_stop_flag(orc):
    """`bool& isStop` (LocalMapping::mbAbortBA, written by the Tracking thread, Optimizer.cc:230, :333, :338): the control kernel polls a
    host-mapped byte the call mirrors the caller's flag into.  Raised before the call: no iteration starts, no classification, no second
    round (`if (!isStop)`), the final chi2 test still runs.  Raised WHILE the call runs: the optimisation ends within one trial."""
    import threading

    from orb_slam2_ros2_amd._lib import Context
    pr, fixed = _problem(21, 30, 1500, 10)
    ctx = Context(640, 480, n_features=500, max_images=1)
    stop = np.ones(1, np.uint8)
    g = ctx.ba_local_optimize(pr, fixed, 5, 10, stop=stop)
    o = orc.ba_local_optimize(pr, fixed, iters1=0, iters2=0)
    assert g["iters"].tolist() == [0, 0] and not g["level"].any()
    assert np.array_equal(g["poses"], pr["poses"]) and np.array_equal(g["points"], pr["points"]) and np.array_equal(g["bad"], o["bad"])
    # WHILE it runs, asserted unconditionally: a window of 300 free keyframes (one trial ~1.2 ms on the blocked solver, the call by itself
    # tens of milliseconds: `alone` measures both), the flag raised by a second thread a third of that time into the call -- long after
    # the first iteration has started, long before Levenberg-Marquardt would end by itself (ten rejected trials in a row)
    import time
    big, fixed_b = _problem(13, 310, 4000, 10)
    ctx.ba_local_optimize(big, fixed_b, 1, 0)                      # warm-up: buffers of this size, first launches
    t0 = time.perf_counter()
    alone = ctx.ba_local_optimize(big, fixed_b, 3000, 0)           # how far Levenberg-Marquardt goes by itself
    t_alone = time.perf_counter() - t0
    assert alone["iters"][0] >= 8 and t_alone > 0.012, (alone["iters"], t_alone)   # the premise: a long call
    stop[0] = 0
    entered, returned, seen = threading.Event(), threading.Event(), {}

    def raiser():
        entered.wait()
        time.sleep(t_alone / 3)
        seen["before_return"] = not returned.is_set()
        stop[0] = 1
    th = threading.Thread(target=raiser)
    th.start()
    entered.set()
    t0 = time.perf_counter()
    g = ctx.ba_local_optimize(big, fixed_b, 3000, 3000, stop=stop)
    t_stopped = time.perf_counter() - t0
    returned.set()
    th.join()
    assert seen["before_return"], "the call returned before the flag was raised: the premise of the test does not hold"
    # the flag came mid-run: iterations had started, the round ended early (within a trial or two of the flag: well before 3000 + 3000
    # iterations' worth of time), no classification, no second round
    assert np.isfinite(g["poses"]).all() and np.isfinite(g["points"]).all()
    assert 1 <= g["iters"][0] < alone["iters"][0], (g["iters"], alone["iters"])
    assert g["iters"][1] == 0 and not g["level"].any()
    assert t_stopped < t_alone, (t_stopped, t_alone)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_kf,n_fixed", [(3, 2), (44, 2), (45, 2), (10, 10), (10, 0)])
def test_device_local_ba_around_the_device_lm_limit(orc, n_kf, n_fixed):
    """1, 42 (the last size of the register-resident Cholesky), 43 (the first of the blocked solver of k_lmbig.hip, under the same
    device-side control), no free and no fixed keyframe at all: same iteration counts and trajectory as the oracle."""
    from orb_slam2_ros2_amd._lib import Context
    pr, fixed = _problem(20 + n_kf, n_kf, 300, n_fixed)
    ctx = Context(640, 480, n_features=500, max_images=1)
    g = ctx.ba_local_optimize(pr, fixed)
    o = orc.ba_local_optimize(pr, fixed)
    ctx.close()
    assert tuple(g["iters"]) == tuple(o["iters"])
    assert _pose_dist(g["poses"], o["poses"]) < 1e-6 and np.abs(g["points"] - o["points"]).max() < 1e-6
