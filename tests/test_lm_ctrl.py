"""The Levenberg-Marquardt controller (csrc/lm_ctrl.h) without a GPU: tests/cpp/test_lm_ctrl.cpp, a stand-alone program under the host
sanitizers (nothing of it is loaded into python), runs the header on the tables written here; every field it returns is compared bit for
bit with the restatement below, which is g2o's OptimizationAlgorithmLevenberg::solve read off its source plus the project's one rule on
top of it (a failed linear solve gives rho = -1).  Both sides take the cube from the C library's pow, so the tolerance is zero."""
import ctypes
import ctypes.util
import math

import numpy as np
import pytest

from test_essential_graph_host import _build_program

DBL_MAX = np.finfo(np.float64).max
RETRY, NEXT_ITERATION, TERMINATE = 0, 1, 2
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.pow.restype = ctypes.c_double
_libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]
f8 = np.float64


def begin(lam, ni, cur, qmax, chi, it, maxdiag):
    """the head of solve(): _currentChi = activeRobustChi2; at iteration 0 lambda = tau * max |diag| and ni = 2; qmax = 0"""
    if it == 0:
        lam, ni = f8(1e-5) * f8(maxdiag), f8(2)
    return lam, ni, f8(chi), 0


def decide(lam, ni, cur, qmax, trial_chi, scale, ok, stopped):
    """one pass of solve()'s do-while body, its loop condition and the Terminate test behind it -> the state, accepted, next"""
    with np.errstate(all="ignore"):
        lam, ni, cur = f8(lam), f8(ni), f8(cur)
        temp = f8(trial_chi) if ok else DBL_MAX
        rho = (cur - temp) / (f8(scale) + f8(1e-3))
        if not ok:
            rho = f8(-1.0)
        accepted = bool(rho > 0 and np.isfinite(temp))
        if accepted:
            alpha = f8(1.0) - f8(_libm.pow(float(f8(2) * rho - f8(1)), 3.0))
            alpha = f8(2.0 / 3.0) if f8(2.0 / 3.0) < alpha else alpha      # std::min(alpha, 2 / 3)
            factor = alpha if f8(1.0 / 3.0) < alpha else f8(1.0 / 3.0)     # std::max(1 / 3, alpha)
            lam, ni, cur = lam * factor, f8(2), temp
        else:
            lam, ni = lam * ni, ni * f8(2)
            if not np.isfinite(lam):
                return lam, ni, cur, qmax, accepted, TERMINATE             # break before qmax++
        qmax += 1
        if rho < 0 and qmax < 10 and not stopped:
            return lam, ni, cur, qmax, accepted, RETRY
        if qmax == 10 or rho == 0 or not np.isfinite(lam):
            return lam, ni, cur, qmax, accepted, TERMINATE
        return lam, ni, cur, qmax, accepted, NEXT_ITERATION


def scale6(x, lam, b):
    with np.errstate(all="ignore"):
        s = f8(0)
        for j in range(6):
            s = s + f8(x[j]) * (f8(lam) * f8(x[j]) + f8(b[j]))
        return s


def optimize(iterations, chi0, maxdiag, trials):
    """SparseOptimizer::optimize over a replayed table: rows (it, qmax, lambda, accepted, next, the trial's lambda)"""
    rows, at = [], 0
    lam, ni, cur, qmax, est_chi = f8(0), f8(2), f8(0), 0, f8(chi0)
    for it in range(iterations):
        lam, ni, cur, qmax = begin(lam, ni, cur, qmax, est_chi, it, maxdiag)
        while True:
            if at == len(trials):
                return rows
            t = trials[at]
            at += 1
            used = lam
            lam, ni, cur, qmax, acc, nxt = decide(lam, ni, cur, qmax, t[0], scale6(t[2:8], lam, t[8:14]), t[1] != 0, False)
            if acc:
                est_chi = f8(t[0])
            rows.append([it, qmax, lam, float(acc), nxt, used])
            if nxt != RETRY:
                break
        if nxt == TERMINATE:
            break
    return rows


def _gain(rho):
    """a decide case whose gain ratio is rho (to a few ulp): current_chi = 1 + 10 rho against a trial chi2 of 1 and scale + 1e-3 = 10"""
    return [1, 3.0, 8.0, 1.0 + 10.0 * rho, 2, 1.0, 10.0 - 1e-3, 1, 0]


# label -> op lambda ni current_chi qmax a b c d (tests/cpp/test_lm_ctrl.cpp)
CASES = {
    "accept, alpha clamped to 2/3 (small gain)": _gain(0.1),
    "accept, alpha just above the 2/3 clamp": _gain(0.84),
    "accept, alpha just below the 2/3 clamp": _gain(0.85),
    "accept, alpha just above the 1/3 floor": _gain(0.93),
    "accept, alpha just below the 1/3 floor": _gain(0.95),
    "accept, gain ratio far above 1": _gain(50.0),
    "accept with the stop flag set": [1, 3.0, 8.0, 10.0, 2, 1.0, 9.999, 1, 1],
    "rho exactly 0": [1, 3.0, 8.0, 5.0, 2, 5.0, 1.0, 1, 0],
    "reject with retry": [1, 3.0, 8.0, 5.0, 2, 6.0, 1.0, 1, 0],
    "reject at qmax 9": [1, 3.0, 8.0, 5.0, 9, 6.0, 1.0, 1, 0],
    "failed solve, the step looks good": [1, 3.0, 8.0, 5.0, 2, 1.0, 1.0, 0, 0],
    "failed solve at qmax 9": [1, 3.0, 8.0, 5.0, 9, 1.0, 1.0, 0, 0],
    "failed solve, current_chi infinite": [1, 3.0, 8.0, math.inf, 2, 1.0, 1.0, 0, 0],
    "failed solve, current_chi NaN": [1, 3.0, 8.0, math.nan, 2, 1.0, 1.0, 0, 0],
    "lambda overflows on reject": [1, 1e308, 1024.0, 5.0, 2, 6.0, 1.0, 1, 0],
    "lambda overflows on a failed solve at qmax 9": [1, 1e308, 1024.0, 5.0, 9, 1.0, 1.0, 0, 0],
    "trial chi2 NaN": [1, 3.0, 8.0, 5.0, 2, math.nan, 1.0, 1, 0],
    "trial chi2 +inf": [1, 3.0, 8.0, 5.0, 2, math.inf, 1.0, 1, 0],
    "trial chi2 DBL_MAX, ok": [1, 3.0, 8.0, 5.0, 2, float(DBL_MAX), 1.0, 1, 0],
    "trial chi2 DBL_MAX, ok, current_chi infinite": [1, 3.0, 8.0, math.inf, 2, float(DBL_MAX), 1.0, 1, 0],
    "scale NaN": [1, 3.0, 8.0, 5.0, 2, 1.0, math.nan, 1, 0],
    "scale + 1e-3 is zero, chi2 falls": [1, 3.0, 8.0, 5.0, 2, 1.0, -1e-3, 1, 0],
    "stopped on a rejected trial": [1, 3.0, 8.0, 5.0, 2, 6.0, 1.0, 1, 1],
    "lambda zero, accept": [1, 0.0, 2.0, 10.0, 0, 1.0, 9.999, 1, 0],
    "lambda zero, reject": [1, 0.0, 2.0, 5.0, 0, 6.0, 1.0, 1, 0],
    "begin, it 0": [0, 3.0, 8.0, 5.0, 7, 4.0, 0, 1234.5, 0],
    "begin, it 3": [0, 3.0, 8.0, 5.0, 7, 4.0, 3, 1234.5, 0],
    "begin, it 0, maxdiag 0": [0, 3.0, 8.0, 5.0, 7, 4.0, 0, 0.0, 0],
    "begin, it 0, maxdiag NaN": [0, 3.0, 8.0, 5.0, 7, 4.0, 0, math.nan, 0],
}
# label -> accepted, next, qmax after it, lambda after it / lambda before it (None: not asserted here, the restatement covers it)
EXPECT = {
    "accept, alpha clamped to 2/3 (small gain)": (1, NEXT_ITERATION, 3, 2.0 / 3.0),
    "accept, alpha just above the 2/3 clamp": (1, NEXT_ITERATION, 3, 2.0 / 3.0),
    "accept, alpha just below the 2/3 clamp": (1, NEXT_ITERATION, 3, "between"),
    "accept, alpha just above the 1/3 floor": (1, NEXT_ITERATION, 3, "between"),
    "accept, alpha just below the 1/3 floor": (1, NEXT_ITERATION, 3, 1.0 / 3.0),
    "accept, gain ratio far above 1": (1, NEXT_ITERATION, 3, 1.0 / 3.0),
    "accept with the stop flag set": (1, NEXT_ITERATION, 3, None),
    "rho exactly 0": (0, TERMINATE, 3, 8.0),
    "reject with retry": (0, RETRY, 3, 8.0),
    "reject at qmax 9": (0, TERMINATE, 10, 8.0),
    "failed solve, the step looks good": (0, RETRY, 3, 8.0),
    "failed solve at qmax 9": (0, TERMINATE, 10, 8.0),
    "failed solve, current_chi infinite": (0, RETRY, 3, 8.0),
    "failed solve, current_chi NaN": (0, RETRY, 3, 8.0),
    "lambda overflows on reject": (0, TERMINATE, 2, math.inf),
    "lambda overflows on a failed solve at qmax 9": (0, TERMINATE, 9, math.inf),
    "trial chi2 NaN": (0, NEXT_ITERATION, 3, 8.0),
    "trial chi2 +inf": (0, RETRY, 3, 8.0),
    "trial chi2 DBL_MAX, ok": (0, RETRY, 3, 8.0),
    "trial chi2 DBL_MAX, ok, current_chi infinite": (1, NEXT_ITERATION, 3, 1.0 / 3.0),
    "scale NaN": (0, NEXT_ITERATION, 3, 8.0),
    "scale + 1e-3 is zero, chi2 falls": (1, NEXT_ITERATION, 3, 1.0 / 3.0),
    "stopped on a rejected trial": (0, NEXT_ITERATION, 3, 8.0),
    "lambda zero, accept": (1, NEXT_ITERATION, 1, None),
    "lambda zero, reject": (0, RETRY, 1, None),
}


def _dampings():
    """(lambda, ni) over 30 decades of lambda, ni every power of two a run of rejects reaches, and lambdas that overflow on the way"""
    rng = np.random.default_rng(11)
    lam = 10.0 ** rng.uniform(-15, 15, 60)
    ni = 2.0 ** rng.integers(1, 11, 60)
    return np.concatenate([np.stack([lam, ni], 1), [[1e300, 2.0], [1.7e308, 2.0], [0.0, 2.0], [5e-324, 2.0]]])


def _loops():
    """(iterations, chi0, maxdiag, trials [n][14]): written runs that reach every exit of the loop, then random ones"""
    rng = np.random.default_rng(12)

    def trial(chi, ok=1, big=False):
        x = rng.normal(size=6) * (1e3 if big else 1e-2)
        return [chi, ok] + list(x) + list(rng.normal(size=6))

    down = [trial(100.0 * 0.5 ** k) for k in range(1, 12)]
    loops = [
        (10, 100.0, 50.0, down),                                                             # every trial accepted, the budget ends it
        (10, 100.0, 50.0, [trial(200.0), trial(150.0), trial(40.0), trial(90.0), trial(20.0), trial(10.0)]),   # rejects, then the table ends
        (10, 100.0, 50.0, [trial(50.0)] + [trial(60.0 + k) for k in range(12)]),             # ten rejects in a row: Terminate
        (10, 100.0, 50.0, [trial(50.0), trial(math.nan), trial(25.0), trial(30.0), trial(12.0)]),    # a NaN chi2: next iteration, not accepted
        (10, 100.0, 50.0, [trial(50.0, ok=0), trial(50.0, ok=0), trial(50.0), trial(20.0)]),          # failed solves that look good
        (10, 100.0, 1.7e308, [trial(200.0) for _ in range(9)]),                              # lambda dies on the way
        (10, 100.0, 0.0, down),                                                              # maxdiag 0: lambda stays 0
        (3, 100.0, 50.0, down),                                                              # the budget ends a run of accepts
        (10, 100.0, 50.0, [trial(50.0), trial(50.0), trial(10.0)]),                          # rho exactly 0: Terminate
        (0, 100.0, 50.0, down),
        (10, 100.0, 50.0, []),
    ]
    for _ in range(40):
        chi, rows = 100.0, []
        for _ in range(int(rng.integers(5, 60))):
            u = rng.uniform()
            if u < 0.45:
                chi *= rng.uniform(0.2, 0.999)
                rows.append(trial(chi, big=rng.uniform() < 0.3))
            elif u < 0.85:
                rows.append(trial(chi * rng.uniform(1.001, 3.0)))
            elif u < 0.95:
                rows.append(trial(chi * rng.uniform(0.2, 3.0), ok=0))
            else:
                rows.append(trial(math.nan))
        loops.append((int(rng.integers(1, 21)), 100.0, float(10.0 ** rng.uniform(-3, 8)), rows))
    return loops


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    import subprocess
    tmp = tmp_path_factory.mktemp("lm_ctrl")
    exe = _build_program(tmp, "test_lm_ctrl.cpp")
    cases, damp, loops = list(CASES.values()), _dampings(), _loops()
    parts = [[len(cases)], np.array(cases, np.float64).reshape(-1), [len(damp)], damp.reshape(-1), [len(loops)]]
    for it, chi0, md, rows in loops:
        parts += [[it, chi0, md, len(rows)], np.array(rows, np.float64).reshape(-1)]
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    np.concatenate([np.asarray(p, np.float64) for p in parts]).astype("<f8").tofile(fin)
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr[-3000:]
    out = np.fromfile(fout, "<f8")
    got = {"cases": out[:6 * len(cases)].reshape(-1, 6)}
    at = 6 * len(cases)
    got["damp"] = out[at:at + 30 * len(damp)].reshape(len(damp), 10, 3)
    at += 30 * len(damp)
    got["loops"] = []
    for _ in loops:
        forms = []
        for _ in range(2):
            n = int(out[at])
            forms.append(out[at + 1:at + 1 + 6 * n].reshape(n, 6))
            at += 1 + 6 * n
        got["loops"].append(forms)
    assert at == len(out)
    return got, damp, loops


def _bits(a):
    return np.asarray(a, np.float64).tobytes()


def test_every_decision_equals_the_restatement_bit_for_bit(run):
    got = run[0]["cases"]
    for (label, c), g in zip(CASES.items(), got):
        if c[0] == 0:
            lam, ni, cur, qmax = begin(c[1], c[2], c[3], int(c[4]), c[5], int(c[6]), c[7])
            want = [lam, ni, cur, qmax, -1, -1]
        else:
            want = [float(v) for v in decide(c[1], c[2], c[3], int(c[4]), c[5], c[6], c[7] != 0, c[8] != 0)]
        assert _bits(g) == _bits(want), (label, list(g), want)


def test_every_branch_of_a_decision_was_reached(run):
    """what each written case must come to, stated apart from the restatement: the decision, the trial count, and the factor lambda took"""
    got = dict(zip(CASES, run[0]["cases"]))
    for label, (acc, nxt, qmax, factor) in EXPECT.items():
        lam, ni, cur, q, a, n = got[label]
        c = CASES[label]
        assert (a, n, q) == (acc, nxt, qmax), (label, a, n, q)
        assert ni == (2.0 if acc else 2 * c[2]) and (_bits(cur) == _bits(c[5] if acc else c[3])), label
        if factor == "between":
            assert c[1] / 3 < lam < c[1] * 2 / 3, (label, lam)
        elif factor is not None:
            assert lam == c[1] * factor, (label, lam)
    # a failed solve is rejected whatever its step looked like: the same state as a rejected trial, whatever current_chi is
    for label in ("failed solve, current_chi infinite", "failed solve, current_chi NaN"):
        assert _bits(got[label][[0, 1, 3, 4, 5]]) == _bits(got["failed solve, the step looks good"][[0, 1, 3, 4, 5]])
    # begin: lambda and ni are set at iteration 0 only and kept across iterations; current_chi and qmax always
    assert list(got["begin, it 0"]) == [1e-5 * 1234.5, 2.0, 4.0, 0.0, -1.0, -1.0]
    assert list(got["begin, it 3"]) == [3.0, 8.0, 4.0, 0.0, -1.0, -1.0]
    assert list(got["begin, it 0, maxdiag 0"]) == [0.0, 2.0, 4.0, 0.0, -1.0, -1.0]
    assert math.isnan(got["begin, it 0, maxdiag NaN"][0])
    assert got["lambda zero, accept"][0] == 0.0 and got["lambda zero, reject"][0] == 0.0


def test_trial_damping_table_is_q_rejects(run):
    """lm6_trial_lambda(lambda, ni, q) = the lambda q consecutive rejected lm_decide leave, bit for bit: k_pose_only_reg and k_sim3_optimize
    solve all ten trials of an iteration from the table before any of them is decided"""
    got, damp = run[0]["damp"], run[1]
    assert len(damp) >= 60 and np.log10(damp[:60, 0].max() / damp[:60, 0].min()) > 25
    assert _bits(got[:, :, 0]) == _bits(got[:, :, 1])
    dead = 0
    for (lam0, ni0), g in zip(damp, got):
        lam, ni = f8(lam0), f8(ni0)
        for q in range(10):
            assert _bits(g[q, 0]) == _bits(lam), (lam0, ni0, q)
            with np.errstate(all="ignore"):
                lam, ni = lam * ni, ni * f8(2)
        finite = np.isfinite(g[:, 0])
        # (a lambda that died at reject k stops the count there: qmax = k - 1 behind it)
        assert list(g[:, 2]) == [float(q if finite[q] else np.argmin(finite) - 1) for q in range(10)]
        dead += int(not finite.all())
    assert dead >= 2


def test_both_forms_of_the_loop_take_the_same_decisions(run):
    """the host's do-while and the kernels' state machine over the same replayed trials: the same (it, qmax, lambda, accepted, next) after
    every decision, the state machine's table dampings equal to the lambdas the do-while carried -- and both equal to the restatement"""
    got, loops = run[0]["loops"], run[2]
    seen = set()
    for (it, chi0, md, rows), (host, sm) in zip(loops, got):
        want = optimize(it, chi0, md, rows)
        assert _bits(host) == _bits(sm), (it, md, len(rows))
        assert _bits(host) == _bits(np.array(want, np.float64).reshape(-1, 6)), (it, md, len(rows))
        seen |= {(int(r[3]), int(r[4])) for r in host}
        seen |= {"qmax 10"} if len(host) and host[:, 1].max() == 10 else set()
        seen |= {"dead"} if len(host) and not np.isfinite(host[:, 2]).all() else set()
    assert {(1, NEXT_ITERATION), (0, RETRY), (0, NEXT_ITERATION), (0, TERMINATE), "qmax 10", "dead"} <= seen
    assert sum(len(h) for h, _ in got) > 500
