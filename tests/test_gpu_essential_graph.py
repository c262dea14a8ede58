"""orbfe_pose_graph_optimize and orbfe_debug_pose_graph_edges on the device against tests/essential_graph_restatement.py (rules G1 .. G8 of
DESIGN 4.24).

Bounds.  The edge probe: bit for bit where an edge's 25 evaluations stay on the small-angle side of Sim3::log's switch -- errors, chi2
and both numeric Jacobians are + - x / sqrt only, correctly rounded on both sides; through acos / sin / cos the errors within 1e-15 of
max(1, |e|) and a Jacobian entry, a difference of two such errors times 1 / 2e-9, within 1e-6 of it (the bounds of the header's
stand-alone test).  The optimiser: every estimate entry within the bound tests/essential_graph_cases.py records for the case and the
iteration count (1e-6, or 100 x the restatement's own spread where that exceeds 1e-8), iteration and trial counts equal, chi2 of every
edge within 1e-6 relative + 1e-12; the module text of the cases says what is compared at which count and why."""
import ctypes

import numpy as np
import pytest

import essential_graph_cases as K
import essential_graph_restatement as R
from test_essential_graph_host import SWITCH, edge_d

pytestmark = pytest.mark.gpu

EBADARG, EBADSIZE = 1, 2


@pytest.fixture(scope="module")
def ctx():
    from orb_slam2_ros2_amd._lib import Context
    c = Context(640, 480, n_features=500, max_images=1)
    yield c
    c.close()


def _chi2_at(g, est):
    return R.edge_chi2(R.errors(R.Graph(*K.args(g)), est))


def test_debug_edges_against_the_restatement(ctx):
    """three estimates of the 101-vertex case: the start (edges on both sides of the switch), after one iteration, converged (every
    edge on the small-angle side)"""
    g = K.graph(101)
    ref = K.reference(101, K.CONV[101][0])
    G = R.Graph(*K.args(g))
    seen_pure = seen_trig = 0
    for name, est in (("start", g["estimates"]), ("one iteration", ref["est_after"][0]), ("converged", ref["est"])):
        err, chi2, jac = ctx.debug_pose_graph_edges(est, g["fixed"], g["edges"], g["meas"])
        E, J0, J1 = R.linearize(G, est)
        C2 = R.edge_chi2(E)
        d = edge_d(g, est)
        pure = d > SWITCH + 1e-7    # (a perturbation of 1e-9 moves d by less than 1e-8: all 25 evaluations on the small-angle side)
        trig = ~pure                # some or all evaluations through acos / sin / cos (the branch is chosen by arithmetic alone)
        assert err[pure].tobytes() == E[pure].tobytes() and chi2[pure].tobytes() == C2[pure].tobytes(), name
        assert jac[pure, 0].tobytes() == J0[pure].tobytes() and jac[pure, 1].tobytes() == J1[pure].tobytes(), name
        fx = g["fixed"].astype(bool)
        assert not jac[fx[g["edges"][:, 0]], 0].any() and not jac[fx[g["edges"][:, 1]], 1].any()     # a fixed vertex has no Jacobian
        seen_pure += int(pure.sum())
        if trig.any():
            scale = np.maximum(1.0, np.abs(E[trig]).max(1))
            de = np.abs(err[trig] - E[trig]).max(1) / scale
            dj = np.maximum(np.abs(jac[trig, 0] - J0[trig]).max((1, 2)), np.abs(jac[trig, 1] - J1[trig]).max((1, 2))) / scale
            same = err[trig].tobytes() == E[trig].tobytes() and jac[trig, 0].tobytes() == J0[trig].tobytes() and jac[trig, 1].tobytes() == J1[trig].tobytes()
            print(f"{name}: {pure.sum()} small-angle edges bit-equal; {trig.sum()} through acos / sin / cos: errors {de.max():.2e}, "
                  f"Jacobians {dj.max():.2e}, bit-equal {same}")
            assert de.max() <= 1e-15 and dj.max() <= 1e-6, name
            assert np.abs(chi2[trig] - C2[trig]).max() <= 1e-14 * max(1.0, C2[trig].max())
            seen_trig += int(trig.sum())
    assert seen_pure >= 300 and seen_trig >= 3


REJECTING = dict(seed=6, drift=(0.05, 0.2), loop=(3.0, 6.0), noise=0.1, consistent=False)
REJECTING_SPREAD = 1.93e-6


def test_rejected_trials_on_eight_vertices(ctx):
    """The reject rule of the host loop (lm_host.h) on the dense solver: 7 free vertices joined by measurements that disagree (noise
    0.1, a loop correction of 3 rad), 3 iterations.  The premise comes from the restatement alone: 7 trials for 3 iterations, 4 of them
    rejected, and no gain ratio within 1e-3 of 0 (the smallest is 0.0115), so no last bit decides a trial.  The restatement's own spread
    between its two summation orders is 1.93e-6 here (recomputed below), past the 1e-8 under which the cases' rule gives 1e-6: the
    bound is 100 x the spread, as tests/essential_graph_cases.py sets it for such a case.  Counts equal, chi2 as the neighbouring test,
    the same bytes on a second call."""
    g = K.make_graph(7, **REJECTING)
    a, b = R.optimize(*K.args(g), iterations=3), R.optimize(*K.args(g), iterations=3, reverse=True)
    assert (a["iterations"], a["trials"]) == (3, 7) and a["accepts"].count(False) == 4 and a["accepts"] == b["accepts"]
    assert min(abs(r) for r in a["rhos"]) >= K.QUAL_RHO and a["chis"][-1] < a["chis"][0]
    spread = float(np.abs(a["est"] - b["est"]).max())
    assert K.QUAL_DIFF < spread <= 3 * REJECTING_SPREAD
    est, chi2, stats = ctx.pose_graph_optimize(*K.args(g), iterations=3, solver=1)
    diff = float(np.abs(est - a["est"]).max())
    print(f"8 vertices, 4 of 7 trials rejected: max |estimate - restatement| {diff:.2e} (restatement's spread {spread:.2e}); stats {stats}")
    assert stats[:3] == (3, 7, 1)
    assert diff <= 100 * REJECTING_SPREAD
    c_ref = _chi2_at(g, est)
    assert np.abs(chi2 - c_ref).max() <= 1e-6 * max(1.0, c_ref.max()) + 1e-12
    again = ctx.pose_graph_optimize(*K.args(g), iterations=3, solver=1)
    assert again[0].tobytes() == est.tobytes() and again[1].tobytes() == chi2.tobytes() and again[2] == stats


@pytest.mark.parametrize("n", K.SIZES)
def test_optimiser_matches_the_restatement(ctx, n):
    g = K.graph(n)
    ref = K.reference(n, 20)
    for what, k, bound in (("admitted", K.ADM[n][0], K.ADM[n][2]), ("converged", K.CONV[n][0], K.BOUND)):
        want, its, trials = K.prefix(ref, k)
        est, chi2, stats = ctx.pose_graph_optimize(*K.args(g), iterations=k)
        diff = float(np.abs(est - want).max())
        c_ref = _chi2_at(g, want)
        print(f"n_free {n}, {what} ({k} iterations): max |estimate - restatement| {diff:.2e} (bound {bound:.2e}); stats {stats} vs {(its, trials)}; "
              f"chi2 {chi2.sum():.3e} vs {c_ref.sum():.3e}")
        assert diff <= bound, what
        assert stats == (its, trials), what
        assert (np.abs(chi2 - c_ref) <= 1e-6 * np.abs(c_ref) + 1e-12).all(), what
        assert est[g["fixed_v"]].tobytes() == g["estimates"][g["fixed_v"]].tobytes()
        if g["isolated"] is not None:
            assert est[g["isolated"]].tobytes() == g["estimates"][g["isolated"]].tobytes()           # no edge: not a bit moves
        assert chi2.tobytes() == _bits_of_debug_chi2(ctx, g, est)
    # optimize(20), the reference's call: the counts are noise at the minimum (cases module), the estimates and chi2 are not
    est, chi2, stats = ctx.pose_graph_optimize(*K.args(g), iterations=20)
    print(f"n_free {n}, 20 iterations: max |estimate - restatement| {np.abs(est - ref['est']).max():.2e}; stats {stats} vs "
          f"{(ref['iterations'], ref['trials'])}; chi2 {chi2.sum():.3e} vs {ref['chi2'].sum():.3e}")
    assert np.abs(est - ref["est"]).max() <= K.BOUND
    assert (np.abs(chi2 - ref["chi2"]) <= 1e-6 * np.abs(ref["chi2"]) + 1e-12).all()
    assert 1 <= stats[0] <= 20 and stats[0] <= stats[1] <= 10 * stats[0]


def _bits_of_debug_chi2(ctx, g, est):
    """chi2_out is the chi2 of every edge AT estimates_out: the probe at those estimates gives the same bytes"""
    return ctx.debug_pose_graph_edges(est, g["fixed"], g["edges"], g["meas"])[1].tobytes()


def test_duplicate_pair_in_opposite_orientation(ctx):
    """the pair joined twice, (a, b) and (b, a), alone with a fixed third vertex: both edges add into the same off-diagonal block, one
    of them transposed"""
    import sim3_opt_restatement as s3
    g = K.graph(7)
    a, b = g["dup"]
    va, vb = (int(v) for v in g["edges"][a])
    f = next(v for v in (0, 3, 5) if v not in (va, vb))                                              # the third vertex: fixed here
    assert tuple(g["edges"][b]) == (vb, va)
    est = g["estimates"][[va, vb, f]]
    tie = s3.sim3_mul(s3.sim3_exp([0.02, -0.01, 0.03, 0.1, 0.0, -0.1]), s3.sim3_mul(tuple(est[2]), s3.sim3_inverse(tuple(est[0]))))
    args = (est, np.array([0, 0, 1], np.uint8), np.array([[0, 1], [1, 0], [0, 2]], np.int32), np.array([g["meas"][a], g["meas"][b], tie]))
    ref = R.optimize(*args, iterations=2)
    est, chi2, stats = ctx.pose_graph_optimize(*args, iterations=2)
    assert np.abs(est - ref["est"]).max() <= K.BOUND and stats == (ref["iterations"], ref["trials"])
    assert (np.abs(chi2 - ref["chi2"]) <= 1e-6 * np.abs(ref["chi2"]) + 1e-12).all()
    assert ref["chis"][-1] < 1e-3 * ref["chis"][0]                                                    # (and it did optimise)


def test_same_call_twice_same_bytes_and_launch_geometry(ctx, monkeypatch):
    for n in (7, 101):
        a = ctx.pose_graph_optimize(*K.args(K.graph(n)), iterations=K.CONV[n][0])
        b = ctx.pose_graph_optimize(*K.args(K.graph(n)), iterations=K.CONV[n][0])
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2], n
    # the one launch-geometry knob: k_pg_build's waves per workgroup (ORBFE_PG_WAVES, read at every call)
    g = K.graph(101)
    monkeypatch.setenv("ORBFE_PG_WAVES", "1")
    c = ctx.pose_graph_optimize(*K.args(g), iterations=K.CONV[101][0])
    d1 = ctx.debug_pose_graph_edges(*K.args(g))
    monkeypatch.setenv("ORBFE_PG_WAVES", "3")
    d3 = ctx.debug_pose_graph_edges(*K.args(g))
    monkeypatch.delenv("ORBFE_PG_WAVES")
    d4 = ctx.debug_pose_graph_edges(*K.args(g))
    assert c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes() and c[2] == a[2]
    assert all(x.tobytes() == y.tobytes() == z.tobytes() for x, y, z in zip(d1, d3, d4))


def test_nothing_to_do_returns_the_input(ctx):
    g = K.graph(7)
    est0 = g["estimates"]
    for what, args, its in (("all fixed", (est0, np.ones(len(est0), np.uint8), g["edges"], g["meas"]), 20),
                            ("no edges", (est0, g["fixed"], np.zeros((0, 2), np.int32), np.zeros((0, 8))), 20),
                            ("no iterations", K.args(g), 0)):
        est, chi2, stats = ctx.pose_graph_optimize(*args, iterations=its)
        assert est.tobytes() == est0.tobytes() and stats == (0, 0), what
    empty = ctx.pose_graph_optimize(np.zeros((0, 8)), np.zeros(0, np.uint8), np.zeros((0, 2), np.int32), np.zeros((0, 8)))
    assert empty[0].shape == (0, 8) and empty[2] == (0, 0)
    g0 = K.make_graph(7, loop=None, drift=None)                                                       # drift-free: nothing moves
    est, chi2, stats = ctx.pose_graph_optimize(*K.args(g0))
    assert chi2.sum() < 1e-20 and np.abs(est - g0["estimates"]).max() <= 1e-12


def test_refusals_leave_the_outputs_untouched(ctx):
    from orb_slam2_ros2_amd import _lib
    g = K.graph(7)
    nv, ne = len(g["estimates"]), len(g["edges"])
    out, chi, stats = np.full((nv, 8), 7.0), np.full(ne, 7.0), np.full(2, -3, np.int32)
    call = ctx.lib.orbfe_pose_graph_optimize

    def run(est=g["estimates"], fixed=g["fixed"], edges=g["edges"], meas=g["meas"], its=20, patch=None, o=out):
        pg, keep = _lib.Context._pose_graph(est, fixed, edges, meas)
        if patch:
            patch(pg)
        return call(ctx.h, ctypes.byref(pg), its, _lib.ptr(o), _lib.ptr(chi), _lib.ptr(stats))

    def with_entry(a, i, j, v):
        a = a.copy()
        a[i, j] = v
        return a

    assert run(patch=lambda pg: setattr(pg, "estimates", None)) == EBADARG                           # NULL arrays with a count
    assert run(patch=lambda pg: setattr(pg, "fixed", None)) == EBADARG
    assert run(patch=lambda pg: setattr(pg, "edge_v1", None)) == EBADARG
    assert run(patch=lambda pg: setattr(pg, "meas", None)) == EBADARG
    assert run(o=None) == EBADARG
    assert call(ctx.h, None, 20, _lib.ptr(out), _lib.ptr(chi), _lib.ptr(stats)) == EBADARG
    assert run(patch=lambda pg: setattr(pg, "n_vertices", -1)) == EBADARG                             # negative counts
    assert run(patch=lambda pg: setattr(pg, "n_edges", -1)) == EBADARG
    assert run(its=-1) == EBADARG
    assert run(edges=with_entry(g["edges"], 3, 0, nv)) == EBADARG                                     # an index out of range
    assert run(edges=with_entry(g["edges"], 3, 1, -1)) == EBADARG
    assert run(edges=with_entry(g["edges"], 3, 1, g["edges"][3, 0])) == EBADARG                       # v0 == v1
    for bad in (np.nan, np.inf, -np.inf):                                                             # entries that are not finite
        assert run(est=with_entry(g["estimates"], 2, 5, bad)) == EBADARG
        assert run(meas=with_entry(g["meas"], 4, 1, bad)) == EBADARG
    assert run(est=with_entry(g["estimates"], 1, 7, 1.25)) == EBADARG                                 # s != 1
    assert run(meas=with_entry(g["meas"], 0, 7, 0.5)) == EBADARG
    # more non-fixed vertices than the documented bound
    from orb_slam2_ros2_amd._lib import PoseGraph  # noqa: F401
    big_n = 1024 + 2
    big = np.tile(g["estimates"][:1], (big_n, 1))
    big_fixed = np.zeros(big_n, np.uint8)
    big_fixed[0] = 1
    big_out = np.full((big_n, 8), 7.0)
    assert run(est=big, fixed=big_fixed, edges=g["edges"][:1], meas=g["meas"][:1], o=big_out) == EBADSIZE
    assert (out == 7.0).all() and (chi == 7.0).all() and (stats == -3).all() and (big_out == 7.0).all()
    err, jac = np.zeros((ne, 6)), np.zeros((ne, 72))
    pg, keep = _lib.Context._pose_graph(*K.args(g))
    dbg = ctx.lib.orbfe_debug_pose_graph_edges
    assert dbg(ctx.h, ctypes.byref(pg), None, _lib.ptr(chi), _lib.ptr(jac)) == EBADARG
    assert dbg(ctx.h, ctypes.byref(pg), _lib.ptr(err), _lib.ptr(chi), None) == EBADARG
    assert not err.any() and not jac.any() and (chi == 7.0).all()
    # and the context still works
    est, _, stats2 = ctx.pose_graph_optimize(*K.args(g), iterations=2)
    assert stats2 == K.prefix(K.reference(7, 20), 2)[1:]


def test_dropin_over_minimal_types(ctx, tmp_path):
    """tests/cpp/test_essential_dropin.cpp, the whole function: the graph the drop-in builds goes through the Python binding in the same
    edge order; the poses written back are ConvertG2o2Sim3(estimate * estimate_0^-1) as (R, t / s), the map points are corrected through
    the loop reference keyframe where the point's loop keyframe is the current one (and that reference is reset), through the
    reference keyframe otherwise, bad points and points whose keyframe is bad or missing stay; all bit for bit."""
    import os
    import subprocess
    import sim3_opt_restatement as s3
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text, sc = K.dropin_scene()
    inp = tmp_path / "in.txt"
    inp.write_text(text)
    exe = str(tmp_path / "t")
    subprocess.check_call(K.dropin_build_command(root, exe), timeout=300)
    r = subprocess.run([exe, str(inp), "full"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    verts, edges = K.dropin_parse_graph(r.stdout)
    vid = {v[0]: k for k, v in enumerate(verts)}
    est, _, stats = ctx.pose_graph_optimize(np.array([v[2] for v in verts]), np.array([v[1] for v in verts], np.uint8),
                                            np.array([[vid[a], vid[b]] for a, b, _ in edges], np.int32), np.array([e[2] for e in edges]))
    assert stats[0] >= 3
    f32 = np.float32
    inv0 = s3.sim3_inverse(tuple(est[vid[0]]))
    want, Sinv = [], {}
    for i in sc["ids"]:
        if i in sc["bad"]:
            m, n_set = sc["model"][i], 0
        else:
            m, n_set = s3.sim3_to_model(s3.sim3_mul(tuple(est[vid[i]]), inv0)), 1
            Rm, t = m[:9].reshape(3, 3), m[9:]
            Rt = Rm.T
            Sinv[i] = (Rt, np.array([-f32(1.0) * ((Rt[r, 0] * t[0] + Rt[r, 1] * t[1]) + Rt[r, 2] * t[2]) for r in range(3)], f32))
        want.append(f"kf {i} {n_set} " + " ".join(f"{int(v):08x}" for v in np.asarray(m, f32).view(np.uint32)))

    def apply(Rm, t, p):
        return np.array([f32(1.0) * ((Rm[r, 0] * p[0] + Rm[r, 1] * p[1]) + Rm[r, 2] * p[2]) + t[r] for r in range(3)], f32)

    for bad, pos, ref, lk, lr in sc["mps"]:
        p = np.asarray(pos, f32)
        kf = lr if lk == sc["curr"] else ref
        moved = not bad and kf >= 0 and kf not in sc["bad"]
        if moved:
            before = sc["corrected"][kf] if kf in sc["corrected"] else sc["model"][kf]
            p = apply(*Sinv[kf], apply(before[:9].reshape(3, 3), before[9:], p))
        keeps_ref = lr >= 0 and (bad or lk != sc["curr"])
        want.append("mp " + " ".join(f"{int(v):08x}" for v in p.view(np.uint32)) + f" {int(moved)} {int(moved)} {int(keeps_ref)}")
    want.append("map updated: 1")
    got = [ln for ln in r.stdout.splitlines() if not ln.startswith(("v ", "e "))]
    assert got == want
