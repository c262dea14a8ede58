"""The keyframe database without a device: the restatement of KeyFrameDB's rules (tests/kfdb_restatement.py) on hand-built cases with known
answers, orbfe_kfdb_group_filter (host code) against it on random cases, orbfe_kfdb_create's refusal without a device, and the drop-in
KeyFrameDB with the reference's call shapes through the compiler.

Scores in the cases are exact: for positive values DBoW's L1 term |v - w| - |v| - |w| is -2 min(v, w), so a score is the sum of min(v, w)
over the common words, and dyadic values keep every sum exact."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import kfdb_restatement as K
from orb_slam2_ros2_amd._lib import OrbfeError, group_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
COMPAT = os.path.join(HOST, "compat")
STUBS = os.path.join(ROOT, "tests", "cpp", "stubs")


def bow(words, value=0.25):
    return {int(w): float(value) for w in words}


# Each case: keyframes, then (in this order) duplicate adds, erases and bad flags; a query in one mode; the known answer as
# {id: shared-word count} of the survivors and the candidate list.  `conn` is every keyframe's ordered covisible list.
CASES = [
    dict(name="th1_tie_max5", kfs={1: bow(range(5)), 2: bow(range(4)), 3: bow(range(3))}, q=bow(range(8)),
         want={1: 5, 2: 4}, cands=[1, 2]),                      # th1 = 4.0: a count of 4 stays, 3 goes
    dict(name="th1_tie_max10", kfs={10: bow(range(10)), 11: bow(range(8)), 12: bow(range(7)), 13: bow(range(20, 30))}, q=bow(range(12)),
         want={10: 10, 11: 8}, cands=[10, 11]),                 # th1 = 8.0
    dict(name="max_one", kfs={1: bow([3]), 2: bow([4, 50]), 3: bow([60])}, q=bow([3, 4]),
         want={1: 1, 2: 1}, cands=[1, 2]),                      # th1 = 0.8
    dict(name="bad_in_lists_and_covisibility", kfs={1: bow(range(10)), 2: bow(range(5), 0.5), 3: bow(range(4))}, bad=[1],
         conn={2: [1, 3], 3: [1]}, q=bow(range(10), 0.5),
         want={2: 5, 3: 4}, cands=[2]),                         # max 5 among the good ones; 1 is skipped in 2's and 3's groups
    dict(name="ignored_duplicate_erased", kfs={1: bow(range(9)), 2: bow(range(5)), 3: bow(range(6)), 4: bow(range(7))},
         dup=[(2, bow(range(9)))], erase=[4], q=bow(range(9)), mode="loop", all_connected=[1], connected15=[],
         want={2: 5, 3: 6}, cands=[2, 3]),                       # 1 ignored, 2 keeps its first vector, 4 is gone; min_score 0
    dict(name="equal_scores_first_wins", kfs={1: bow([0, 1], 0.125), 2: bow([0, 1]), 3: bow([0, 1])}, conn={1: [3, 2]},
         q=bow([0, 1], 0.5), want={1: 2, 2: 2, 3: 2}, cands=[3]),   # 2 and 3 tie above 1: the first of 1's list (3) wins
    dict(name="equal_scores_own_keyframe_first", kfs={1: bow([0, 1]), 2: bow([0, 1])}, conn={1: [2], 2: [1]},
         q=bow([0, 1], 0.5), want={1: 2, 2: 2}, cands=[1, 2]),
    dict(name="best_shared_by_two_groups", kfs={1: bow([0, 1], 0.125), 2: bow([0, 1], 0.125), 3: bow([0, 1])}, conn={1: [3], 2: [3]},
         q=bow([0, 1], 0.5), want={1: 2, 2: 2, 3: 2}, cands=[3]),
    dict(name="acc_equal_th2", kfs={1: bow([0, 1]), 2: bow([0, 1]), 3: {0: 0.5, 1: 0.25}}, conn={1: [2]},
         q=bow([0, 1], 1.0), want={1: 2, 2: 2, 3: 2}, cands=[1]),   # group 1: 1.0 = best; group 3: 0.75 = th2, not above
    dict(name="empty_database", kfs={}, q=bow(range(5)), want={}, cands=[]),
    dict(name="empty_query", kfs={1: bow(range(5))}, q={}, want={}, cands=[]),
    dict(name="empty_query_loop", kfs={1: bow(range(5))}, q={}, mode="loop", all_connected=[], connected15=[1], want={}, cands=[]),
    dict(name="loop_min_score_from_connected", kfs={1: bow(range(4), 0.5), 2: bow(range(4), 0.125), 3: bow(range(4)), 4: bow(range(4))},
         bad=[4], q=bow(range(4), 0.5), mode="loop", all_connected=[4], connected15=[4, 3],
         want={1: 4, 3: 4}, cands=[1]),                         # floor = score(3) = 1.0 (4 is bad): 2 (0.5) goes
    dict(name="loop_all_connected_bad", kfs={1: bow(range(4), 0.5), 2: bow(range(4))}, bad=[2], q=bow(range(4), 0.5), mode="loop",
         all_connected=[2], connected15=[2], want={1: 4}, cands=[1]),   # floor stays 1: score(1) = 2.0 passes
    dict(name="loop_connected_outside_the_query", kfs={1: bow(range(2), 0.25), 2: bow(range(2), 0.125), 5: bow([7])}, q=bow(range(2), 0.5),
         mode="loop", all_connected=[], connected15=[5], want={1: 2, 2: 2}, cands=[1]),   # score(5) = 0 lowers the floor to 0
]


def build(case):
    R = K.Restatement()
    for k, b in case["kfs"].items():
        R.add(k, b)
    for k, b in case.get("dup", []):
        R.add(k, b)
    for k in case.get("erase", []):
        R.erase(k)
    for k in case.get("bad", []):
        R.set_bad(k)
    return R


def run_case(R, case):
    """(survivors {id: (count, score)}, candidates) of the case's query on the restatement"""
    q, conn = case["q"], case.get("conn", {})
    if case.get("mode", "reloc") == "reloc":
        return R.query(q), R.reloc(q, conn)
    ignore = [k for k in case["all_connected"] if k not in R.bad]
    surv = R.query(q, ignore, R.min_score(q, case["connected15"]))
    return surv, R.loop(q, case["all_connected"], case["connected15"], conn)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_known_answers(case):
    R = build(case)
    surv, cands = run_case(R, case)
    assert {k: c for k, (c, _) in surv.items()} == case["want"]
    assert cands == case["cands"]
    assert list(surv) == sorted(surv)


def test_restatement_thresholds():
    # float th1 = (float)maxWordNum * 0.8: exactly 4.0 and 8.0 at 5 and 10, 0.8 (as a float) at 1
    for mx, th in ((5, 4.0), (10, 8.0), (1, np.float32(0.8))):
        assert np.float32(float(np.float32(mx)) * 0.8) == th
    assert K.min_word_filter({1: 5, 2: 4, 3: 3}) == {1: 5, 2: 4}
    assert K.min_word_filter({}) == {}


def test_restatement_scores_are_dbow_l1():
    q = {1: 0.5, 2: 0.25, 9: 0.25}
    kf = {2: 0.125, 9: 0.5, 11: 0.375}
    assert K.score_l1(q, kf) == 0.125 + 0.25
    R = K.Restatement()
    R.add(7, kf)
    assert R.query(q) == {7: (2, 0.375)}


def _random_groups(rng, n):
    ids = rng.choice(10 * n + 5, n, replace=False).astype(np.uint64)
    scores = rng.choice([0.0, 0.125, 0.25, 0.5, 0.75], n) if rng.random() < 0.5 else rng.random(n)
    pool = np.concatenate([ids, rng.integers(10 * n + 5, 20 * n + 10, 3).astype(np.uint64)])   # some covisible ids are not survivors
    conn = [list(rng.choice(pool, rng.integers(0, min(10, len(pool)) + 1), replace=False)) for _ in range(n)]
    return ids, scores, conn


def test_group_filter_c_abi_equals_the_restatement():
    rng = np.random.default_rng(17)
    for it in range(400):
        n = int(rng.integers(0, 40))
        ids, scores, conn = _random_groups(rng, n)
        want = K.group_filter({int(k): (1, float(s)) for k, s in zip(ids, scores)}, {int(k): [int(c) for c in cs] for k, cs in zip(ids, conn)})
        got = group_filter(ids, scores, conn)
        assert got.tolist() == want, it


def test_group_filter_c_abi_known_cases():
    for case in CASES:
        surv, cands = run_case(build(case), case)
        ids = np.array(list(surv), np.uint64)
        conn = [[c for c in case.get("conn", {}).get(k, []) if c not in case.get("bad", [])] for k in surv]
        assert group_filter(ids, [s for _, s in surv.values()], conn).tolist() == cands, case["name"]


def test_group_filter_rejects_repeated_survivors():
    with pytest.raises(OrbfeError) as ei:
        group_filter([3, 3], [0.5, 0.5], [[], []])
    assert ei.value.status == 1


def test_kfdb_create_fails_loudly_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    from orb_slam2_ros2_amd._lib import KeyFrameDB
    with pytest.raises(OrbfeError) as ei:
        KeyFrameDB(1000)
    assert ei.value.status == 3 and "no CPU fallback" in str(ei.value)


# ---- the drop-in KeyFrameDB and the reference's call shapes through the compiler ---------------------------------------------------
REF = "/root/reference/src/ORB_SLAM2"
_have_ref = os.path.isdir(os.path.join(REF, "include", "ORB_SLAM2")) and shutil.which("g++") is not None

# The reference's call shapes, verbatim in form: Tracking.cc:418, LoopClosing.cc:59 / 224, LocalMapping.cc:731, System.cc:104-109
CALLERS = r"""
#include "ORB_SLAM2/KeyFrameDB.h"
#include "ORB_SLAM2/Frame.h"
#include "ORB_SLAM2/KeyFrame.h"
namespace ORB_SLAM2_ROS2 {
void call_shapes(std::shared_ptr<DBoW3::Vocabulary> pVocab, std::vector<KeyFrame::SharedPtr> allKfs, Frame::SharedPtr mpCurrFrame,
                 KeyFrame::SharedPtr mpCurrKeyFrame) {
  KeyFrameDB::SharedPtr mpKfDB = std::make_shared<KeyFrameDB>(pVocab->size());
  for (auto &pKf : allKfs)
    mpKfDB->addKeyFrame(pKf);
  std::vector<KeyFrame::SharedPtr> vpCandidateKFs;
  mpKfDB->findRelocKfs(mpCurrFrame, vpCandidateKFs);
  mpKfDB->addKeyFrame(mpCurrKeyFrame);
  std::vector<KeyFrame::SharedPtr> vpLoopCandidates;
  mpKfDB->findLoopCloseKfs(mpCurrKeyFrame, vpLoopCandidates);
  std::shared_ptr<KeyFrameDB> pkfDB = mpKfDB;
  pkfDB->addKeyFrame(mpCurrKeyFrame);
  mpKfDB->eraseKeyFrame(mpCurrKeyFrame);
  Group g;
  g.mfAccScore = 0;
  (void)g;
}
}  // namespace ORB_SLAM2_ROS2
"""


def _ref_includes_with_kfdb(tmp):
    d = os.path.join(tmp, "ORB_SLAM2")
    os.makedirs(d)
    src = os.path.join(REF, "include", "ORB_SLAM2")
    for f in os.listdir(src):
        if f not in ("ORBExtractor.h", "KeyFrameDB.h"):
            os.symlink(os.path.join(src, f), os.path.join(d, f))
    with open(os.path.join(d, "ORBExtractor.h"), "w") as fh:
        fh.write("#pragma once\n#include <orbfe_dropin.hpp>\n")
    with open(os.path.join(d, "KeyFrameDB.h"), "w") as fh:   # the header becomes one line
        fh.write("#include <orbfe_kfdb_dropin.hpp>\n")
    return tmp


def _syntax_only(inc, tu):
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + COMPAT, "-I" + inc, "-I" + STUBS, "-I" + os.path.join(STUBS, "refgen"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + HOST, tu], capture_output=True, text=True, timeout=600)


@pytest.mark.skipif(not _have_ref, reason="needs /root/reference (build container only) and g++")
def test_dropin_bodies_and_reference_call_shapes_compile(tmp_path):
    inc = _ref_includes_with_kfdb(str(tmp_path / "inc"))
    bodies = tmp_path / "KeyFrameDB.cc"   # src/KeyFrameDB.cc becomes one line
    bodies.write_text("#include <orbfe_kfdb_dropin_impl.hpp>\n")
    r = _syntax_only(inc, str(bodies))
    assert r.returncode == 0, r.stderr[-4000:]
    callers = tmp_path / "callers.cc"
    callers.write_text(CALLERS)
    r = _syntax_only(inc, str(callers))
    assert r.returncode == 0, r.stderr[-4000:]
