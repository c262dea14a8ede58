"""The EPnP RANSAC sets on the device (orbfe_pnp_*, _lib.PnPSet) against the restatement of PnPSolver + Ransac<PnPRet>
(tests/pnp_restatement.py): ret, no_more, the pose as float bits, the inlier list (duplicates included) and the process-wide engine
state equal after every iterate call -- under Tracking's loop shape, under adversarial call patterns (which is what shows that
speculation never changes a result), at 30 x 1000 points, from two threads, and through the drop-in over minimal types."""
import copy
import os
import subprocess
import threading

import numpy as np
import pytest

import pnp_restatement as P
from orb_slam2_ros2_amd._lib import PnPSet, pnp_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_set(seed, sizes, outliers=None, degenerate=None):
    rng = np.random.default_rng(seed)
    xs, us, os_ = [], [], []
    for i, n in enumerate(sizes):
        out = rng.uniform(0, 0.9) if outliers is None else outliers[i]
        deg = None if degenerate is None else degenerate[i]
        x, u, o, _, _ = P.scene(rng, n, outlier=out, degenerate=deg)
        xs.append(x)
        us.append(u)
        os_.append(o)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cat = lambda a, k: np.concatenate(a) if len(a) and sum(map(len, a)) else np.zeros((0, k), np.float32)
    return off, cat(xs, 3), cat(us, 2), np.concatenate(os_).astype(np.int32) if sum(sizes) else np.zeros(0, np.int32)


class Pair:
    """one set on the device and its restatement, driven together; every call compares everything"""

    def __init__(self, seed, sizes, eng, **kw):
        self.off, self.xyz, self.uv, self.oc = make_set(seed, sizes, **kw)
        self.dev = PnPSet(self.off, self.xyz, self.uv, self.oc, P.SIGMA2, P.CAM)
        self.ref = [P.Solver(self.xyz[a:b], self.uv[a:b], self.oc[a:b], P.SIGMA2, P.CAM) for a, b in zip(self.off[:-1], self.off[1:])]
        self.eng = eng
        self.calls = 0

    def iterate(self, p, n, pose=None, inliers=()):
        r = self.ref[p].iterate(self.eng, n, None if pose is None else (np.asarray(pose[0], np.float32).reshape(9),
                                                                      np.asarray(pose[1], np.float32)), list(inliers))
        d = self.dev.iterate(p, n, pose, np.asarray(inliers, np.int32))
        what = f"call {self.calls}: problem {p}, n {n}"
        assert d[0] == r[0] and d[1] == r[1], what
        if r[2] is None:
            assert d[2] is None, what
        else:
            assert d[2] is not None, what
            assert np.array_equal(d[2].reshape(9).view(np.uint32), r[2][0].view(np.uint32)), what
            assert np.array_equal(d[3].view(np.uint32), r[2][1].view(np.uint32)), what
        assert d[4].tolist() == list(r[3]), what
        assert pnp_engine() == self.eng.state, what
        self.calls += 1
        return d[0], d[1], (None if d[2] is None else (d[2], d[3])), d[4].tolist()

    def close(self):
        self.dev.close()


def accept_half(pair):
    return lambda p, pose, inl: len(set(inl)) * 2 >= pair.off[p + 1] - pair.off[p]


@pytest.fixture
def engine():
    pnp_engine(1)
    yield P.Engine(1)


MIX = [3, 4, 5, 12, 60, 400]


@pytest.mark.parametrize("seed", range(6))
def test_tracking_loop_bit_exact(engine, seed):
    rng = np.random.default_rng(1000 + seed)
    sizes = [int(rng.choice(MIX)) for _ in range(8)]
    deg = [rng.choice([None, None, "collinear", "repeat"]) for _ in range(8)]
    pair = Pair(seed, sizes, engine, degenerate=deg)
    log = P.tracking_loop(pair.iterate, 8, 5, accept_half(pair))
    assert len(log) > 0
    launches, hyps = pair.dev.stats()
    assert launches >= 1 and hyps >= sum(r.n_hyp for r in pair.ref)
    pair.close()


def test_adversarial_calls_and_two_sets_on_one_engine(engine):
    rng = np.random.default_rng(77)
    a = Pair(11, [int(rng.choice(MIX)) for _ in range(8)], engine)
    b = Pair(12, [int(rng.choice(MIX)) for _ in range(8)], engine)
    last = {}
    for step in range(160):
        pair = a if rng.uniform() < 0.5 else b
        p = int(rng.integers(0, 8))
        n = int(rng.choice([1, 3, 5, 7, 100]))
        pose, inl = None, []
        if rng.uniform() < 0.3 and (id(pair), p) in last:
            pose, inl = last[(id(pair), p)]
            inl = list(inl[: int(rng.integers(0, len(inl) + 1))])
        elif rng.uniform() < 0.1:
            N = pair.off[p + 1] - pair.off[p]
            inl = rng.integers(0, max(N, 1), int(rng.integers(0, 6))).tolist() if N else []
        if rng.uniform() < 0.05:
            s = int(rng.integers(1, 2147483646))
            pnp_engine(s)
            engine.state = s
        ret, nm, pose2, inl2 = pair.iterate(p, n, pose, inl)
        if pose2 is not None:
            last[(id(pair), p)] = (pose2, inl2)
    a.close()
    b.close()


def test_launch_counts(engine):
    # a failing relocalisation: 20 candidates of pure outliers, every budget spent -> one launch sequence
    pair = Pair(5, [200] * 20, engine, outliers=[1.0] * 20)
    log = P.tracking_loop(pair.iterate, 20, 5, accept_half(pair))
    assert all(r[1] for _, r in log[-20:])
    assert pair.dev.stats()[0] == 1
    pair.close()
    # a success in some round r: at most two
    for k in range(3):
        outl = [1.0] * 10
        outl[3 + k] = 0.1
        pair = Pair(40 + k, [200] * 10, engine, outliers=outl)
        log = P.tracking_loop(pair.iterate, 10, 5, accept_half(pair))
        assert log[-1][0] == 3 + k and log[-1][1][0]
        assert pair.dev.stats()[0] <= 2
        pair.close()


def test_thirty_by_a_thousand(engine):
    rng = np.random.default_rng(3)
    pair = Pair(30, [1000] * 30, engine, outliers=list(rng.uniform(0.5, 0.95, 30)))
    P.tracking_loop(pair.iterate, 30, 5, accept_half(pair))
    pair.close()


def test_two_threads_two_sets_engine_consistent():
    """each thread drives its own set; the lock serialises whole calls, so some interleaving of the two call lists, replayed on the
    restatement from the initial engine, gives every recorded result"""
    pnp_engine(1)
    sets = []
    for seed in (21, 22):
        off, xyz, uv, oc = make_set(seed, [60, 12, 400, 5, 60, 60], outliers=[0.6] * 6)
        sets.append((off, xyz, uv, oc))
    logs = [[], []]

    def run(i):
        off, xyz, uv, oc = sets[i]
        dev = PnPSet(off, xyz, uv, oc, P.SIGMA2, P.CAM)

        def it(p, n):
            r = dev.iterate(p, n)
            logs[i].append((p, n, r))
            return r[0], r[1], r[2], r[4]
        P.tracking_loop(it, len(off) - 1, 5)
        dev.close()

    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not any(t.is_alive() for t in th)
    ref = [[P.Solver(xyz[a:b], uv[a:b], oc[a:b], P.SIGMA2, P.CAM) for a, b in zip(off[:-1], off[1:])] for off, xyz, uv, oc in sets]
    final = pnp_engine()

    def same(r, d):
        if r[0] != d[0] or r[1] != d[1] or list(r[3]) != d[4].tolist() or (r[2] is None) != (d[2] is None):
            return False
        return r[2] is None or (np.array_equal(r[2][0].view(np.uint32), d[2].reshape(9).view(np.uint32)) and
                                np.array_equal(r[2][1].view(np.uint32), d[3].view(np.uint32)))

    # depth-first over interleavings: a call may give the same result from several engine states (P4 returns the best model whatever
    # it drew), so a wrong early choice shows only later
    def search(at, state, refs):
        if at[0] == len(logs[0]) and at[1] == len(logs[1]):
            return state == final
        for i in (0, 1):
            if at[i] == len(logs[i]):
                continue
            p, n, d = logs[i][at[i]]
            trial = copy.deepcopy(refs[i][p])
            e = P.Engine(state)
            if same(trial.iterate(e, n), d):
                nr = [list(refs[0]), list(refs[1])]
                nr[i][p] = trial
                na = list(at)
                na[i] += 1
                if search(na, e.state, nr):
                    return True
        return False

    import sys
    sys.setrecursionlimit(10000)
    assert search([0, 0], 1, ref), "no interleaving of the two threads' calls explains their results"


def test_dropin_over_minimal_types(tmp_path):
    """tests/cpp/test_pnp_dropin.cpp: the drop-in PnPSolver, driven by Tracking's loop, writes its records; the Python binding on the
    same data and engine must write the same"""
    off, xyz, uv, oc = make_set(8, [60, 4, 400, 12, 60, 3, 60, 200], outliers=[0.5, 0, 0.7, 0.2, 0.9, 0, 0.3, 0.6])
    inp = tmp_path / "in.txt"
    with open(inp, "w") as f:
        f.write(f"{len(off) - 1}\n")
        for a, b in zip(off[:-1], off[1:]):
            f.write(f"{b - a}\n")
            for i in range(a, b):
                f.write(" ".join(repr(float(v)) for v in (*xyz[i], *uv[i])) + f" {int(oc[i])}\n")
    pkg = os.path.join(ROOT, "orb_slam2_ros2_amd")
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), "-I" + os.path.join(pkg, "host"),
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_pnp_dropin.cpp"), "-L" + pkg,
                           "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    # the same loop through the Python binding, in a fresh engine
    pnp_engine(1)
    dev = PnPSet(off, xyz, uv, oc, P.SIGMA2, P.CAM)
    lines = []

    def it(p, n):
        d = dev.iterate(p, n)
        pose = "-" if d[2] is None else " ".join(f"{int(v):08x}" for v in np.concatenate([d[2].reshape(9), d[3]]).view(np.uint32))
        lines.append(f"{p} {int(d[0])} {int(d[1])} {pose} |" + "".join(f" {i}" for i in d[4].tolist()))
        return d[0], d[1], d[2], d[4]
    P.tracking_loop(it, len(off) - 1, 5)
    dev.close()
    assert r.stdout.strip().splitlines() == lines
