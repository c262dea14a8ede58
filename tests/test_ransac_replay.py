"""The one replay of Ransac<T>::iterate (csrc/ransac_replay.h) without a GPU: tests/cpp/test_ransac_replay.cpp, a stand-alone program
under the host sanitizers (nothing of it is loaded into python), plays tables of calls and of speculation records through the one
function under both policies.  The tables come from pnp_restatement.Solver and sim3_restatement.Solver: a speculation's records are what
the restatement's own model / check produce for the schedule's samples (its refines logged from a run of the restatement's iterate), so
they are data, the replay does no arithmetic on them, and every field it returns is compared with the restatement's iterate with
tolerance zero.  Which calls a record serves is stated here a second time (Book), and the speculation counts of the written cases are
asserted as plain numbers besides."""
import copy
import subprocess

import numpy as np
import pytest

import pnp_restatement as P
import sim3_restatement as S
from test_essential_graph_host import _build_program

DONE, NO_ROOM = 0, 5  # ransac::Verdict


class Pnp:
    code, min_set, entry_matters, tracks_skipped = 0, 4, True, False

    @staticmethod
    def flat(model):
        return np.zeros(12, np.float32) if model is None else np.concatenate([model[0], model[1]]).astype(np.float32)

    @staticmethod
    def hypotheses(s, samples):
        sm = np.array(samples)
        deg, R, t = P.epnp(s.xyz[sm].astype(np.float64), s.uv[sm].astype(np.float64), s.cam)
        return deg, np.concatenate([R, t], 1), P.check_inliers(s.xyz, s.uv, s.thr, s.cam, R, t)

    @staticmethod
    def room(n_entry, n, size):  # PnPSet.iterate's buffer
        return n_entry + (n + 2) * size + 1


class Sim3:
    code, min_set, entry_matters, tracks_skipped = 1, 3, False, True

    @staticmethod
    def flat(model):
        return np.zeros(12, np.float32) if model is None else np.asarray(model, np.float32)

    @staticmethod
    def hypotheses(s, samples):
        sm = np.array(samples)
        models = S.model_func(s.P3[sm], s.Q3[sm])
        return np.zeros(len(sm), bool), models, S.check_inliers(s.P3, s.Q3, s.P2, s.Q2, s.thrP, s.thrQ, s.cam, models)

    @staticmethod
    def room(n_entry, n, size):  # Sim3Set.iterate's buffer
        return max(n_entry, size) + 1


def budget(kind, s, n, cur):
    return max(0, min(n, s.max_it - cur)) if s.N >= kind.min_set else 0


def clone(s):
    c = copy.copy(s)
    if hasattr(c, "stats"):
        c.stats = dict(c.stats)
    return c


def mask_words(indices, N):
    m = np.zeros(2 * ((N + 63) // 64), np.uint32)
    for i in indices:
        m[i // 32] |= np.uint32(1 << (i % 32))
    return m.view(np.int32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def speculate(kind, sols, cur, called, skipped, engine, p, n, model, entry):
    """What a set uploads and downloads at an unpredicted call (p, n, entry state): that call, the rest of its round, then whole rounds
    over the live problems, ascending, n each, from a copy of the engine.  -> (records, hypotheses).  A hypothesis's refine record is
    what a run of the restatement's iterate over the call's samples did at that hypothesis."""
    cur, called = list(cur), list(called)
    eng = P.Engine(engine)
    recs, hyps = [], []

    def live(q):
        s = sols[q]
        return not skipped[q] and ((cur[q] < s.max_it or not called[q]) if s.N >= kind.min_set else not called[q])

    def add(q, first):
        s, k = sols[q], budget(kind, sols[q], n, cur[q])
        N = s.N
        rec = dict(prob=q, n=n, entry_hyp=-1, engine_start=eng.state, after=[])
        blank = dict(words=(N + 63) // 64, degen=0, count=0, refined=0, ref_count=0, model=np.zeros(12, np.float32),
                     ref_model=np.zeros(12, np.float32), mask=mask_words([], N), ref_mask=mask_words([], N))
        given = model if first and kind.entry_matters else None
        if given is not None and N >= kind.min_set:
            rec["entry_hyp"] = len(hyps)
            inl = s.check(given)
            hyps.append(dict(blank, count=len(inl), model=kind.flat(given), mask=mask_words(inl, N)))
        rec["h0"] = len(hyps)
        probe = P.Engine(eng.state)
        samples = []
        for _ in range(k):
            samples.append(P.random_sample(probe, N, kind.min_set))
            rec["after"].append(probe.state)
        if k:
            deg, models, masks = kind.hypotheses(s, samples)
            for h in range(k):
                hyps.append(dict(blank, degen=int(deg[h])) if deg[h] else
                            dict(blank, count=int(masks[h].sum()), model=models[h], mask=mask_words(np.nonzero(masks[h])[0], N)))
        counts = [h["count"] for h in hyps[len(hyps) - k - (rec["entry_hyp"] >= 0):]]
        if k and max(counts) > s.min_inlier:  # (no count above mnMinInlier: no refine in this call)
            # the refines: a model() call followed by the check() of what it left, at hypothesis cur - cur0
            c = clone(s)
            c.cur, c.best, cur0, pending = cur[q], 0, cur[q], []

            def model_(idx):
                pending.append(c.cur - cur0)
                return type(s).model(c, idx)

            def check_(m):
                inl = type(s).check(c, m)
                if pending:
                    hyps[rec["h0"] + pending.pop()].update(refined=1, ref_count=len(inl), ref_model=kind.flat(m), ref_mask=mask_words(inl, N))
                return inl
            c.model, c.check = model_, check_
            c.iterate(P.Engine(eng.state), n, given, list(entry) if first and kind.entry_matters else [])
        if k:
            eng.state = rec["after"][-1]
        cur[q] += k
        called[q] = True
        recs.append(rec)

    add(p, True)
    for q in range(p + 1, len(sols)):
        if live(q):
            add(q, False)
    any_ = True
    while any_:
        any_ = False
        for q in range(len(sols)):
            if live(q):
                add(q, False)
                any_ = True
    return recs, hyps


class Book:
    """which calls the records serve, restated: the next record serves a call on the same problem with the same n, the engine untouched,
    as many hypotheses as the budget leaves and (PnP) no entry state; a refine success, a refusal and a spent budget drop the records;
    (Sim3) the problems between the expected record and the called one are left out of later schedules until they are called"""

    def __init__(self, kind, sols, engine=1):
        self.kind, self.sols, self.eng = kind, list(sols), P.Engine(engine)
        self.engine0, self.first_sols, self.calls = engine, list(sols), []
        self.recs, self.next = [], 0
        self.called, self.skipped = [False] * len(sols), [False] * len(sols)
        self.specs, self.want = [], []

    def call(self, p, n, model=None, entry=(), cap=None, set_engine=0):
        kind, s, entry = self.kind, self.sols[p], list(entry)
        if set_engine:
            self.eng.state = set_engine
        k = budget(kind, s, n, s.cur)
        pending = 0 < self.next < len(self.recs)
        hit = pending and not (kind.entry_matters and (model is not None or entry))
        if hit:
            r = self.recs[self.next]
            hit = (r["prob"], r["n"], r["engine_start"], len(r["after"])) == (p, n, self.eng.state, k)
        if kind.tracks_skipped:
            if not hit and pending:
                window = [r["prob"] for r in self.recs[self.next:self.next + len(self.sols)]]
                if p in window:
                    for q in window[:window.index(p)]:
                        self.skipped[q] = True
            self.skipped[p] = False
        asked = [0]
        if s.N < kind.min_set or hit or k == 0:
            self.next = self.next + 1 if hit else 0
            self.recs = self.recs if hit else []
        else:
            has = model is not None and kind.entry_matters
            n_entry = len(entry) if kind.entry_matters else 0
            self.recs, hyps = speculate(kind, self.sols, [x.cur for x in self.sols], self.called, self.skipped, self.eng.state, p, n, model, entry)
            self.specs.append((self.recs, hyps))
            self.next = 1
            asked = [1, p, n, int(has), n_entry]
        trial, e2 = clone(s), P.Engine(self.eng.state)
        ret, no_more, out_model, out_list = trial.iterate(e2, n, model, entry)
        cap = kind.room(len(entry), n, s.N) if cap is None else cap
        if len(out_list) > cap:  # refused: nothing committed
            self.recs, self.next = [], 0
            head = [NO_ROOM, 0, 0, int(model is not None)] + list(bits(kind.flat(model))) + [len(out_list)]
        else:
            if s.N >= kind.min_set and trial.cur - s.cur < k:  # a refine success ended the call before its budget
                self.recs, self.next = [], 0
            self.sols[p], self.eng.state, self.called[p] = trial, e2.state, True
            head = [DONE, int(ret), int(no_more), int(out_model is not None)] + list(bits(kind.flat(out_model))) + [len(out_list)] + out_list
        skipped = sum(1 << q for q, f in enumerate(self.skipped) if f)
        self.want.append(head + [self.eng.state, self.sols[p].cur, self.sols[p].best, skipped, len(self.specs)] + asked)
        self.calls.append([p, n, set_engine, int(model is not None)] + list(bits(kind.flat(model))) + [cap, len(entry)] + entry)
        return ret, no_more, out_model, out_list

    def words(self):
        w = [self.kind.code, len(self.sols), len(self.specs), len(self.calls), self.engine0]
        for s in self.first_sols:
            w += [s.N, s.min_inlier, s.max_it]
        for recs, hyps in self.specs:
            w += [len(recs), len(hyps)]
            for r in recs:
                w += [r["prob"], r["n"], r["h0"], len(r["after"]), r["entry_hyp"], r["engine_start"]] + r["after"]
            for h in hyps:
                w += [h["words"], h["degen"], h["count"], h["refined"], h["ref_count"]]
                w += list(bits(h["model"])) + list(bits(h["ref_model"])) + list(h["mask"]) + list(h["ref_mask"])
        for c in self.calls:
            w += c
        return w


def pnp(seed, N, outlier=0.0, degenerate=None, params=(4, 100, 0.4, 0.99)):
    X, uv, oc, _, _ = P.scene(np.random.default_rng(seed), N, outlier=outlier, degenerate=degenerate)
    return P.Solver(X, uv, oc, P.SIGMA2, P.CAM, params)


def sim3(seed, N, outlier=0.0, noise=0.5, **kw):
    return S.Solver(*S.scene(np.random.default_rng(seed), N, outlier=outlier, noise=noise), **kw)


def rounds(b, problems, n, max_calls=400):
    """the reference's loop: round-robin over `problems` until each has said bNoMore"""
    left, log = list(problems), []
    while left and len(log) < max_calls:
        for p in list(left):
            r = b.call(p, n)
            log.append((p, r))
            if r[1]:
                left.remove(p)
    return log


# ---- the written cases: each returns its Book and asserts that the restatement took the path it is about ----------------------------
def case_p1_list_accumulates_and_a_failed_refine_replaces_it():
    """a test_pnp_host test_p1 scene (seed 27 of them, found by search; the path is asserted): in the third call of n = 5 the refine
    receives the list piled up over the call's hypotheses, duplicates included (P1), and fails, so the best model's list is that multiset"""
    X, uv, oc, _, _ = P.scene(np.random.default_rng(27), 60, outlier=0.45)
    b = Book(Pnp, [P.Solver(X, uv, oc, P.SIGMA2, P.CAM, (4, 20, 0.4, 0.99))], 28)
    b.call(0, 5)
    b.call(0, 5)
    ret, no_more, pose, lst = b.call(0, 5)
    assert ret and b.sols[0].cur == 15 and len(lst) != len(set(lst)) and lst == b.sols[0].best_list
    refined = [h for h in b.specs[0][1][10:15] if h["refined"]]
    assert len(refined) == 1 and refined[0]["ref_count"] <= b.sols[0].min_inlier
    b.call(0, 5)
    return b, 1


def _p2_scene():
    X, uv, oc, _, _ = P.scene(np.random.default_rng(2), 5, noise=0.0)
    X[:4] = X[0] + np.linspace(0, 1, 4)[:, None] * (X[1] - X[0])
    st = next(st for st in range(1, 200000) if sorted(P.random_sample(P.Engine(st), 5)) == [0, 1, 2, 3])
    return (X, uv, oc, P.SIGMA2, P.CAM), st


def case_p2_degenerate_sample_with_an_entry_pose():
    args, st = _p2_scene()
    b = Book(Pnp, [P.Solver(*args)], st)
    entry = (np.eye(3, dtype=np.float32).reshape(9), np.array([0, 0, 100], np.float32))
    ret, no_more, pose, lst = b.call(0, 1, entry)
    assert not ret and not no_more and pose is entry and lst == b.sols[0].check(entry) and b.specs[0][1][1]["degen"] == 1
    assert b.specs[0][0][0]["entry_hyp"] == 0
    return b, 1


def case_p2_degenerate_sample_without_an_entry_pose():
    args, st = _p2_scene()
    b = Book(Pnp, [P.Solver(*args)], st)
    assert b.call(0, 1) == (False, False, None, []) and b.specs[0][1][0]["degen"] == 1
    return b, 1


def case_p3_success_leaves_the_budget_and_drops_the_records():
    b = Book(Pnp, [pnp(3, 200, outlier=0.1, params=(4, 15, 0.4, 0.99)), pnp(4, 30, outlier=1.0, params=(4, 10, 0.4, 0.99))])
    ret, no_more, pose, lst = b.call(0, 5)
    assert ret and not no_more and b.sols[0].cur < 5 and len(b.specs[0][0]) > 2
    b.call(1, 5)  # the schedule had this call, but the success dropped it
    b.call(0, 5)
    return b, 2


def case_s3_success_leaves_the_budget_and_drops_the_records():
    b = Book(Sim3, [sim3(1, 100, outlier=0.1), sim3(2, 30, outlier=1.0, params=(3, 10, 0.4, 0.99))])
    ret, no_more, model, lst = b.call(0, 5)
    assert ret and not no_more and b.sols[0].cur < 5 and b.sols[0].stats["refine_success"] == 1 and len(b.specs[0][0]) > 2
    b.call(1, 5)
    b.call(0, 5)
    return b, 2


def case_p4_best_model_returned_by_a_later_empty_call():
    for seed in range(80):
        b = Book(Pnp, [pnp(seed, 30, outlier=0.55, params=(4, 15, 0.4, 0.99))], seed + 7)
        for _ in range(40):
            r = b.call(0, 1)
            if r[1]:
                break
        if b.sols[0].best > 0 and r[1]:
            n_spec = len(b.specs)
            r = b.call(0, 5)  # the budget is spent: the best model again, and nothing for the device
            assert r[0] and r[1] and r[2] is b.sols[0].best_pose and r[3] == b.sols[0].best_list and len(b.specs) == n_spec
            return b, None
    pytest.fail("no persisting best model found")


def case_s4_best_model_returned_by_a_later_empty_call():
    b = Book(Sim3, [sim3(3, 60, outlier=0.5, noise=1.5)])
    log = rounds(b, [0], 1)
    assert log[-1][1][1] and b.sols[0].stats["fallback_best"] >= 2 and b.sols[0].stats["refine_failed"] >= 1
    r = b.call(0, 5, None, [])
    assert r[0] and r[1] and r[2] is b.sols[0].best_model and b.sols[0].stats["zero_budget"] == 1
    return b, 1


def case_p5_small_problems_and_a_spent_budget():
    b = Book(Pnp, [pnp(1, 0), pnp(1, 3), pnp(1, 4), pnp(5, 30, outlier=1.0, params=(4, 5, 0.4, 0.99))])
    entry = (np.arange(9, dtype=np.float32), np.arange(3, dtype=np.float32))
    for p in (0, 1, 2):
        assert b.call(p, 5) == (False, True, None, [])
    r = b.call(1, 5, entry, [2, 0, 0])  # N < 4: the arguments stay
    assert r[1] and r[2] is entry and r[3] == [2, 0, 0]
    assert (b.sols[2].min_inlier, b.sols[2].max_it) == (4, 0)
    assert b.call(3, 5)[:2] == (False, True) and b.call(3, 5)[:2] == (False, True) and b.eng.state != 1
    return b, 1


def case_s5_small_problems_and_a_spent_budget():
    b = Book(Sim3, [sim3(1, 0), sim3(1, 2), sim3(1, 3), sim3(5, 30, outlier=1.0, params=(3, 5, 0.4, 0.99))])
    entry = np.arange(12, dtype=np.float32)
    for p in (0, 1, 2):
        assert b.call(p, 5) == (False, True, None, [])
    r = b.call(1, 5, entry, [1, 1, 0])
    assert r[1] and r[2] is entry and r[3] == [1, 1, 0]
    assert (b.sols[2].min_inlier, b.sols[2].max_it) == (3, 0)
    assert b.call(3, 5)[:2] == (False, True)
    r = b.call(3, 5, entry, [4, 4])  # a spent budget and no best model: the arguments stay
    assert not r[0] and r[1] and r[2] is entry and r[3] == [4, 4]
    return b, 1


def case_s2_the_entry_list_is_ignored():
    b = Book(Sim3, [sim3(1, 100, outlier=0.1), sim3(2, 40, outlier=1.0, params=(3, 10, 0.4, 0.99))])
    ret, no_more, model, lst = b.call(0, 5, None, [7, 7, 7])
    assert ret and lst.count(7) == 1 and lst == sorted(set(lst))
    # and neither the entry model nor the entry list breaks a prediction
    b.call(1, 5)
    b.call(0, 5, np.arange(12, dtype=np.float32), [3, 3])
    assert b.want[-1][-1] == 0
    return b, 2


def _refused(kind, sols):
    b = Book(kind, sols)
    need = len(clone(b.sols[0]).iterate(P.Engine(1), 5)[3])
    assert need > 1
    b.call(0, 5, cap=need - 1)
    assert b.want[-1][0] == NO_ROOM and b.want[-1][16] == need and b.want[-1][17:20] == [1, 0, 0]  # engine, cur, best as they were
    r = b.call(0, 5, cap=need)
    assert r[0] and len(r[3]) == need
    return b, 2


def case_p_one_short_of_room_is_refused_and_nothing_is_committed():
    return _refused(Pnp, [pnp(3, 70, outlier=0.1, params=(4, 10, 0.4, 0.99))])


def case_s_one_short_of_room_is_refused_and_nothing_is_committed():
    return _refused(Sim3, [sim3(1, 70, outlier=0.1)])


def _mispredicted(kind, sols):
    b = Book(kind, sols)
    for p in (0, 1, 2, 0):
        b.call(p, 5)
    assert len(b.specs) == 1
    b.call(2, 5)                       # another problem than the schedule's
    assert len(b.specs) == 2
    b.call(0, 5)
    b.call(1, 1)                       # another n
    assert len(b.specs) == 3
    b.call(2, 1)
    b.call(0, 1, set_engine=4711)      # the engine moved
    assert len(b.specs) == 4
    b.call(1, 1)
    assert not any(w[1] for w in b.want)
    return b, 4


def case_p_a_mispredicted_call_costs_one_more_speculation():
    return _mispredicted(Pnp, [pnp(10 + i, N, outlier=1.0, params=(4, 20, 0.4, 0.99)) for i, N in enumerate((33, 64, 70))])


def case_s_a_mispredicted_call_costs_one_more_speculation():
    return _mispredicted(Sim3, [sim3(10 + i, N, outlier=1.0, params=(3, 20, 0.4, 0.99)) for i, N in enumerate((33, 64, 70))])


def case_s_a_problem_never_called_costs_one_more_speculation_once():
    """test_gpu_sim3's test_a_problem_never_called_costs_one_more_launch: problems 1 and 4 of six stay uncalled through 14 rounds"""
    b = Book(Sim3, [sim3(i, 60, outlier=1.0) for i in range(6)])
    log = rounds(b, [0, 2, 3, 5], 5)
    assert len(log) == 4 * 14 and not any(r[0] for _, r in log) and len(b.specs) == 3 and b.skipped == [False, True, False, False, True, False]
    # called after all, a left-out problem is served like any other: it is back in the schedules, so its second call is predicted
    assert b.call(4, 5)[:2] == (False, False) and len(b.specs) == 4
    assert b.call(4, 5)[:2] == (False, False) and len(b.specs) == 4
    assert b.call(1, 100)[:2] == (False, True) and len(b.specs) == 5
    return b, 5


def case_p_an_entry_state_is_never_served_from_a_record():
    b = Book(Pnp, [pnp(20 + i, N, outlier=1.0, params=(4, 10, 0.4, 0.99)) for i, N in enumerate((40, 65, 50))])
    pose = (np.eye(3, dtype=np.float32).reshape(9), np.array([0, 0, 1], np.float32))
    b.call(0, 5)
    b.call(1, 5)                       # predicted
    assert len(b.specs) == 1
    r = b.call(2, 5, pose)             # the predicted problem and n, with an entry pose
    assert len(b.specs) == 2 and b.specs[1][0][0]["entry_hyp"] == 0
    b.call(0, 5)
    b.call(1, 5, None, [3, 1, 1])      # .. with an entry list
    assert len(b.specs) == 3 and b.want[-1][-1] == 3
    b.call(2, 5, r[2], r[3])           # .. with what the last call on it returned, as Tracking passes it
    assert len(b.specs) == 4
    return b, 4


def case_random_orders(kind, make, seed, n_calls):
    rng = np.random.default_rng(seed)
    b = Book(kind, [make(30 + seed + i, int(rng.integers(3, 71)), float(rng.choice([0.2, 0.6, 1.0]))) for i in range(int(rng.integers(1, 4)))])
    last = {}
    for _ in range(n_calls):
        p, n = int(rng.integers(0, len(b.sols))), int(rng.choice([1, 5]))
        carry = last.get(p) if rng.uniform() < 0.5 else None
        r = b.call(p, n, *(carry or (None, [])), set_engine=int(rng.integers(1, 1 << 30)) if rng.uniform() < 0.1 else 0)
        last[p] = (r[2], r[3])
    return b, None


CASES = {f.__name__[5:]: f for f in list(globals().values()) if callable(f) and getattr(f, "__name__", "").startswith("case_") and f is not case_random_orders}
# (the restatement's EPnP is slow from Python: one short PnP order, three Sim3 ones)
CASES["random_orders_pnp"] = lambda: case_random_orders(Pnp, lambda s, N, o: pnp(s, N, outlier=o, params=(4, 6, 0.4, 0.99)), 1, 20)
for _seed in range(3):
    CASES[f"random_orders_sim3_{_seed}"] = lambda seed=_seed: case_random_orders(Sim3, lambda s, N, o: sim3(s, N, outlier=o, params=(3, 12, 0.4, 0.99)), seed, 30)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ransac_replay")
    exe = _build_program(tmp, "test_ransac_replay.cpp")
    books = {name: f() for name, f in CASES.items()}
    words = [len(books)]
    for b, _ in books.values():
        words += b.words()
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    np.array(words, np.int64).astype("<i4").tofile(fin)
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr[-3000:]
    return books, [int(v) for v in np.fromfile(fout, "<i4")]


def test_every_field_of_every_call_equals_the_restatement(run):
    """ret, no_more, has, the model's bits, the list, the engine, the problem's cur and best, which problems are marked skipped, the
    number of speculations so far and what each speculation was asked for: equal, call by call, under both policies"""
    books, got = run
    at, calls = 0, 0
    for name, (b, _) in books.items():
        for i, want in enumerate(b.want):
            assert got[at:at + len(want)] == want, (name, i, got[at:at + len(want)], want)
            at += len(want)
            calls += 1
    assert at == len(got) and calls > 250


def test_the_speculation_counts_of_the_written_cases(run):
    """stated apart from Book: a success, a refusal, a misprediction and a PnP entry state each cost exactly one more speculation"""
    books, got = run
    for name, (b, n_spec) in books.items():
        if n_spec is not None:
            assert len(b.specs) == n_spec, name
    sizes = {s.N for b, _ in books.values() for s in b.sols}
    assert min(sizes) == 0 and {3, 4} <= sizes and any(64 < N <= 70 for N in sizes) and any(4 < N <= 64 for N in sizes)
    assert {len(b.sols) for b, _ in books.values()} >= {1, 2, 3}
