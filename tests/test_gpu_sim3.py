"""The Sim3 RANSAC sets on the device (orbfe_sim3_*, _lib.Sim3Set) against the restatement of Sim3Solver + Ransac<Sim3Ret>
(tests/sim3_restatement.py): ret, no_more, the model as float bits, the inlier list and the Sim3 engine's state equal after every
iterate call -- under LoopClosing::computeSim3's loop shape, at the sizes where the kernel changes path (no point, fewer than a sample,
a zero budget, one mask word / its edges / several), under call patterns that break the prediction (which is what shows that speculation
never changes a result), on hand-made degenerate correspondences, and through the drop-in over minimal types."""
import os
import subprocess

import numpy as np
import pytest

import pnp_restatement as P
import sim3_restatement as S
from orb_slam2_ros2_amd._lib import OrbfeError, PnPSet, Sim3Set, pnp_engine, sim3_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EBADARG, ECAPACITY = 1, 4
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)


def make_set(specs):
    """specs: per problem (seed, N, outlier, noise) -> the arrays of Sim3Set and the per-problem scenes"""
    scenes = [S.scene(np.random.default_rng(seed), N, outlier=out, noise=noise) for seed, N, out, noise in specs]
    return pack(scenes), scenes


def pack(scenes):
    sizes = [len(sc[0]) for sc in scenes]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cat = lambda k, shape, dt: (np.concatenate([np.asarray(sc[k], dt).reshape(shape) for sc in scenes]) if scenes
                                else np.zeros(shape, dt).reshape(shape)[:0])
    return (off, cat(0, (-1, 3), np.float32), cat(1, (-1, 3), np.float32), cat(2, (-1,), np.int32), cat(3, (-1,), np.int32),
            cat(4, (-1, 12), np.float32), cat(5, (-1, 12), np.float32))


class Pair:
    """one set on the device and its restatement, driven together; every call compares everything"""

    def __init__(self, scenes, eng, params=None):
        self.arrays = pack(scenes)
        self.dev = Sim3Set(*self.arrays, S.SIGMA2, S.CAM, params)
        self.ref = [S.Solver(*sc, params=params or (3, 100, 0.4, 0.99)) for sc in scenes]
        self.eng = eng
        self.calls = 0

    def iterate(self, p, n, model=None, inliers=()):
        r = self.ref[p].iterate(self.eng, n, model, list(inliers))
        d = self.dev.iterate(p, n, model, np.asarray(inliers, np.int32))
        what = f"call {self.calls}: problem {p}, n {n}"
        assert d[0] == r[0] and d[1] == r[1], what
        if r[2] is None:
            assert d[2] is None, what
        else:
            assert d[2] is not None, what
            assert np.array_equal(d[2].view(np.uint32), np.asarray(r[2], np.float32).view(np.uint32)), what
        assert d[3].tolist() == list(r[3]), what
        assert sim3_engine() == self.eng.state, what
        self.calls += 1
        return d[0], d[1], d[2], d[3].tolist()

    def stat(self, key):
        return sum(r.stats[key] for r in self.ref)

    def close(self):
        self.dev.close()


@pytest.fixture
def engine():
    sim3_engine(1)
    yield S.Engine(1)


def scenes_of(specs):
    return make_set(specs)[1]


SIZES = [0, 2, 3, 4, 5, 63, 64, 65, 129, 300]


def test_sizes_where_the_kernel_changes_path(engine):
    pair = Pair(scenes_of([(100 + i, N, 0.3, 0.5) for i, N in enumerate(SIZES)]), engine)
    log = S.loop_closing_loop(pair.iterate, len(SIZES), 5)
    assert pair.stat("too_few") == 2 and pair.stat("zero_budget") >= 1            # N = 0 and 2; N = 3 has a budget of 0
    assert pair.stat("refine_success") > 0 and all(r[1] for _, r in log[-1:])
    launches, hyps = pair.dev.stats()
    assert launches >= 1 and hyps >= sum(r.n_hyp for r in pair.ref)
    pair.close()


@pytest.mark.parametrize("n_problems", [1, 3, 20])
@pytest.mark.parametrize("n", [1, 3, 5, 100])
def test_loop_closing_loop_bit_exact(engine, n_problems, n):
    rng = np.random.default_rng(n_problems * 1000 + n)
    specs = [(int(rng.integers(1 << 30)), int(rng.choice([5, 40, 70, 129])), float(rng.choice([0.2, 0.6, 1.0])), 0.5) for _ in range(n_problems)]
    pair = Pair(scenes_of(specs), engine, params=(3, 20, 0.4, 0.99))
    log = S.loop_closing_loop(pair.iterate, n_problems, n, lambda p, m, inl: p == n_problems - 1 and len(inl) * 2 >= len(pair.ref[p].P3))
    assert len(log) > 0
    pair.close()


def test_all_fail_set_is_one_launch(engine):
    pair = Pair(scenes_of([(i, 60, 1.0, 0.5) for i in range(20)]), engine)
    log = S.loop_closing_loop(pair.iterate, 20, 5)
    assert not any(r[0] for _, r in log) and all(r[1] for _, r in log[-20:])
    assert pair.stat("failed") == len(log) and pair.stat("refine_success") == 0 and pair.stat("fallback_best") == 0
    assert pair.dev.stats() == (1, sum(r.max_it for r in pair.ref))
    # the budgets are spent: further calls need no device
    for p in (0, 7, 19):
        assert pair.iterate(p, 5)[:2] == (False, True)
    assert pair.dev.stats()[0] == 1
    pair.close()


def test_a_problem_never_called_costs_one_more_launch(engine):
    """computeSim3 discards a candidate after its solver is made (too few matches pass vbChoose) and never iterates it: problems 1 and 4
    stay in the set uncalled.  The first round leaves the schedule once at each of them, and the schedule made there omits it: one launch
    more per such problem, not one per round (14 rounds here)."""
    pair = Pair(scenes_of([(i, 60, 1.0, 0.5) for i in range(6)]), engine)
    used = [0, 2, 3, 5]
    log = S.loop_closing_loop(lambda i, n: pair.iterate(used[i], n), len(used), 5)
    assert len(log) == 4 * 14 and not any(r[0] for _, r in log)
    assert pair.dev.stats()[0] == 3
    # a left-out problem that is called after all is served like any other
    assert pair.iterate(4, 5)[:2] == (False, False) and pair.iterate(1, 100)[:2] == (False, True)
    pair.close()


def test_refine_success_in_the_first_call(engine):
    pair = Pair(scenes_of([(1, 100, 0.1, 0.5), (2, 100, 1.0, 0.5)]), engine)
    ret, no_more, model, inl = pair.iterate(0, 5)
    assert ret and not no_more and len(inl) > pair.ref[0].min_inlier
    assert pair.stat("refine_success") == 1 and pair.ref[0].cur < 5               # S3: the success did not spend its iteration
    pair.close()


def test_fallback_best_return(engine):
    # a scene whose first passing hypothesis fails its refine (found by search over seeds; the driver asserts that the path is taken)
    pair = Pair(scenes_of([(3, 60, 0.5, 1.5)]), engine)
    log = S.loop_closing_loop(pair.iterate, 1, 5)
    assert pair.stat("refine_failed") >= 1 and pair.stat("fallback_best") >= 1 and pair.stat("refine_success") == 0
    first = next(i for i, (_, r) in enumerate(log) if r[0])
    assert all(r[0] for _, r in log[first:])                                        # S4: it persists
    pair.close()


def test_success_after_a_failed_refine(engine):
    pair = Pair(scenes_of([(3, 100, 0.3, 2.0)]), engine)
    S.loop_closing_loop(pair.iterate, 1, 5)
    assert pair.stat("refine_failed") >= 1 and pair.stat("refine_success") >= 1
    pair.close()


def test_broken_predictions_two_sets_and_an_independent_pnp_engine(engine):
    rng = np.random.default_rng(77)
    mk = lambda s: scenes_of([(s * 100 + i, int(rng.choice([2, 3, 5, 40, 65, 129])), float(rng.choice([0.2, 0.55, 1.0])), 1.0) for i in range(6)])
    a, b = Pair(mk(1), engine), Pair(mk(2), engine)
    pnp_engine(1)
    pe = P.Engine(1)
    x, u, o, _, _ = P.scene(np.random.default_rng(5), 60, outlier=0.5)
    pnp_dev = PnPSet(np.array([0, 60], np.int64), x, u, o, P.SIGMA2, P.CAM)
    pnp_ref = P.Solver(x, u, o, P.SIGMA2, P.CAM)
    last = {}
    for step in range(120):
        pair = a if rng.uniform() < 0.5 else b
        p = int(rng.integers(0, 6))
        n = int(rng.choice([1, 3, 5, 100]))
        model, inl = (None, [])
        if rng.uniform() < 0.3 and (id(pair), p) in last:
            model, inl = last[(id(pair), p)]
        if rng.uniform() < 0.05:                                                    # an engine reset between calls
            s = int(rng.integers(1, 2147483646))
            sim3_engine(s)
            engine.state = s
        if rng.uniform() < 0.1:                                                     # a PnP call in between: its own engine
            before = sim3_engine()
            r = pnp_ref.iterate(pe, 3)
            d = pnp_dev.iterate(0, 3)
            assert d[0] == r[0] and d[1] == r[1] and d[4].tolist() == list(r[3])
            assert pnp_engine() == pe.state and sim3_engine() == before
        before = pnp_engine()
        ret, nm, model2, inl2 = pair.iterate(p, n, model, inl)
        assert pnp_engine() == before
        if model2 is not None:
            last[(id(pair), p)] = (model2, inl2)
    assert pe.state != engine.state
    for x_ in (a, b):
        x_.close()
    pnp_dev.close()


def hand_made(P3, Q3):
    """correspondences given in the cameras' frames: identity poses, octave 0"""
    n = len(P3)
    return (np.asarray(P3, np.float32), np.asarray(Q3, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), IDENT.copy(), IDENT.copy())


def test_hand_made_collinear_points(engine):
    s = np.array([1.0, 2.0, 3.5, 4.0, 6.0])
    line = np.array([0.1, -0.2, 3.0]) + s[:, None] * np.array([0.3, 0.1, 1.0])
    pair = Pair([hand_made(line, line + np.array([0.05, 0.0, 0.1]))], engine)
    # every sample is collinear and every call succeeds at its first hypothesis, which spends no budget (S3): a fixed number of calls
    for n in (1, 5, 3, 100):
        ret, no_more, model, inl = pair.iterate(0, n)
        assert ret and not no_more and inl == [0, 1, 2, 3, 4]
    assert pair.ref[0].n_hyp == 1 + 5 + 3 + 19 and pair.ref[0].cur == 0 and pair.stat("refine_success") == 4
    pair.close()


def test_hand_made_identical_points_give_the_identity_rotation(engine):
    Pp = np.tile([0.5, -0.25, 4.0], (5, 1))
    Qq = np.tile([0.75, 0.25, 4.5], (5, 1))
    pair = Pair([hand_made(Pp, Qq)], engine)
    ret, no_more, model, inl = pair.iterate(0, 1)
    # N is all zero, the Jacobi takes no sweep: the first eigenvector is (1, 0, 0, 0), R = I and t = Oq - Op
    assert np.array_equal(model[:9], IDENT[:9]) and np.array_equal(model[9:], np.array([0.25, 0.5, 0.5], np.float32))
    assert ret and inl == [0, 1, 2, 3, 4]
    pair.close()


def test_hand_made_point_at_z_zero_is_a_nan_inlier(engine):
    rng = np.random.default_rng(9)
    pts = np.stack([rng.uniform(-1, 1, 8), rng.uniform(-1, 1, 8), rng.uniform(3, 9, 8)], 1)
    pts[5] = 0.0                                                                     # maps to (0, 0, 0): 0 / 0 in Camera::project
    pair = Pair([hand_made(pts, pts)], engine)
    ret, no_more, model, inl = pair.iterate(0, 1)
    # Q = P: N's first row is (trace, 0, 0, 0), so the model is exactly the identity whatever the sample
    assert np.array_equal(model, IDENT)
    assert np.isnan(S.project(pair.ref[0].P3[5:6], S.CAM)).all()
    assert ret and 5 in inl and inl == list(range(8))
    pair.close()


def test_capacity_and_refusals(engine):
    scenes = scenes_of([(1, 100, 0.1, 0.5)])
    pair = Pair(scenes, engine)
    with pytest.raises(OrbfeError) as e:
        pair.dev.iterate(0, 5, cap=10)
    assert e.value.status == ECAPACITY and sim3_engine() == 1                        # nothing changed ..
    ret, _, _, inl = pair.iterate(0, 5)                                             # .. so the call still equals the restatement's
    assert ret and len(inl) > 10
    for bad in (-1, 1):
        with pytest.raises(OrbfeError) as e:
            pair.dev.iterate(bad, 5)
        assert e.value.status == EBADARG
    for state in (0, 2147483647):
        with pytest.raises(OrbfeError) as e:
            sim3_engine(state)
        assert e.value.status == EBADARG
    arrays = pair.arrays
    with pytest.raises(OrbfeError) as e:                                             # S1: no other min set
        Sim3Set(*arrays, S.SIGMA2, S.CAM, (4, 100, 0.4, 0.99))
    assert e.value.status == EBADARG
    with pytest.raises(OrbfeError) as e:                                             # an octave beyond the levels
        Sim3Set(*arrays, S.SIGMA2[:3], S.CAM)
    assert e.value.status == EBADARG
    pair.close()


def test_dropin_over_minimal_types(tmp_path):
    """tests/cpp/test_sim3_dropin.cpp: the drop-in Sim3Solver, driven by computeSim3's loop, writes its records; the Python binding on
    the same data and engine must write the same"""
    (off, pp, pq, op, oq, tp, tq), scenes = make_set([(1, 60, 0.5, 0.5), (2, 3, 0.0, 0.5), (3, 129, 0.7, 0.5), (4, 12, 0.2, 0.5),
                                                      (5, 2, 0.0, 0.5), (6, 65, 1.0, 0.5)])
    inp = tmp_path / "in.txt"
    with open(inp, "w") as f:
        f.write(f"{len(off) - 1}\n")
        for k, (a, b) in enumerate(zip(off[:-1], off[1:])):
            f.write(f"{b - a}\n")
            f.write(" ".join(repr(float(v)) for v in (*tp[k], *tq[k])) + "\n")
            for i in range(a, b):
                f.write(" ".join(repr(float(v)) for v in (*pp[i], *pq[i])) + f" {int(op[i])} {int(oq[i])}\n")
    pkg = os.path.join(ROOT, "orb_slam2_ros2_amd")
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), "-I" + os.path.join(pkg, "host"),
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_sim3_dropin.cpp"), "-L" + pkg,
                           "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    sim3_engine(1)
    dev = Sim3Set(off, pp, pq, op, oq, tp, tq, S.SIGMA2, S.CAM)
    lines = []

    def it(p, n):
        d = dev.iterate(p, n)
        model = "-" if d[2] is None else " ".join(f"{int(v):08x}" for v in d[2].view(np.uint32))
        lines.append(f"{p} {int(d[0])} {int(d[1])} {model} |" + "".join(f" {i}" for i in d[3].tolist()))
        return d
    S.loop_closing_loop(it, len(off) - 1, 5)
    dev.close()
    assert r.stdout.strip().splitlines() == lines
