"""searchByBow over stored keyframes (orbfe_search_by_bow_stored) without a device: the scenes of bow_search_scenes.py
really exercise the rules (asserted on the CPU oracle's output, special cases placed by hand), the header without HIP (csrc/bow_angle.h)
runs as a stand-alone program under the host compiler's sanitizers against cases the Python restatement wrote, and the surface: header,
exports, bindings, ctypes mirrors, ABI version, the drop-in against the reference's real declarations."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_search_scenes as bs  # noqa: E402
import triangulation_restatement as tr  # noqa: E402
from orb_slam2_ros2_amd.frontend import ORBMatcher  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src/ORB_SLAM2"
F32 = np.float32


# ---- the rules of verifyAngle, restated piecewise (what bow_angle.h states in C) ----------------------------------------------------------
def angle_bin(aq, at):
    diff = F32(aq) - F32(at)
    diff = diff if diff >= 0 else F32(360) + diff
    b = int(diff / F32(12))
    return 0 if b == 30 else b


def choose_bins(count):
    chosen = []
    for _ in range(3):
        best, best_id = 0, None
        for i, c in enumerate(count):
            if i not in chosen and c > best:
                best, best_id = c, i
        if best_id is not None:
            chosen.append(best_id)
    return sorted(chosen)


def select(matches, aq, at):
    bins = [angle_bin(aq[m[0]], at[m[1]]) for m in matches]
    keep = choose_bins(np.bincount(bins, minlength=30)[:30])
    return [m for b in keep for m, mb in zip(matches, bins) if mb == b]


def test_the_piecewise_restatement_is_verify_angle():
    rng = np.random.default_rng(5)
    for trial in range(40):
        n = int(rng.integers(0, 60))
        aq, at = bs.wrap_angle(rng.uniform(-180, 180, 50)), bs.wrap_angle(rng.uniform(-180, 180, 50))
        if trial % 2:                                   # few distinct differences: ties between bins
            at = bs.wrap_angle(aq.astype(np.float64) - 12.0 * rng.integers(0, 6, 50) - 6)
        m = [(int(rng.integers(0, 50)), int(rng.integers(0, 50)), int(rng.integers(0, 50))) for _ in range(n)]
        assert select(m, aq, at) == ORBMatcher.verifyAngle(m, aq, at)


# ---- 1. the scenes exercise the rules ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return bs.scene(0)


@pytest.mark.parametrize("mode", ["track", "loop"])
def test_the_small_scene_drops_matches_and_folds_long_lists(small, mode):
    query, cands = small
    assert len(cands) == 4 and all(len(c["kps"]) == 300 for c in cands + [query])
    nodes, offs, _ = query["fv"]
    assert np.diff(offs).max() > 128 and nodes[np.argmax(np.diff(offs))] == bs.BIG_NODE     # more than two fold chunks
    free = [p for p in tr.featvec_dict(query["fv"])[bs.BIG_NODE] if not (query["flags"][p] & bs.GOOD)]
    assert len(free) > 64                                                               # ... also after TRACK's filter
    for kf in cands:
        raw, bins = bs.raw_and_bins(query, kf, bs.MODES[mode], 0.75)
        kept = bs.oracle(query, kf, bs.MODES[mode], 0.75, True)
        print(mode, len(raw), len(set(bins)), len(kept))
        assert len(raw) >= 50 and len(set(bins)) >= 4 and 0 < len(kept) < len(raw)
        assert kept == select(raw, query["kps"]["angle"], kf["kps"]["angle"])
    # the modes differ, and ADD's filter acts on both sides
    r = {m: bs.oracle(query, cands[0], bs.MODES[m], 0.75, False) for m in bs.MODES}
    assert len({tuple(v) for v in r.values()}) == 3


def test_the_hand_placed_cases_are_what_they_claim():
    q, c = bs.hand_scene()
    aq = q["kps"]["angle"]
    # bins: a difference a hair below zero lands in bin 30 and is folded into bin 0; 7 and 9 compete for third place, 7 wins
    raw, bins = bs.raw_and_bins(q, c["bins"], bs.TRACK, 0.75)
    pair0 = [b for m, b in zip(raw, bins) if m[0] == 0]
    d = F32(aq[0]) - F32(c["bins"]["kps"]["angle"][[m[1] for m in raw if m[0] == 0][0]])
    assert d < 0 and F32(360) + d == F32(360) and pair0 == [30]
    folded = np.bincount([0 if b == 30 else b for b in bins], minlength=30)
    assert folded[0] == 5 and folded[3] == 4 and folded[7] == 2 and folded[9] == 2 and folded[12] == 1 and folded.sum() == 14
    kept = bs.oracle(q, c["bins"], bs.TRACK, 0.75, True)
    kept_q = [m[0] for m in kept]
    assert len(kept) == 11 and 0 in kept_q and {9, 10} <= set(kept_q) and not {11, 12, 13} & set(kept_q)
    assert kept == select(raw, aq, c["bins"]["kps"]["angle"])
    # fewbins: fewer than three non-empty bins, everything survives
    raw, bins = bs.raw_and_bins(q, c["fewbins"], bs.TRACK, 0.75)
    assert len(set(bins)) == 2 and sorted(bs.oracle(q, c["fewbins"], bs.TRACK, 0.75, True)) == sorted(raw) and len(raw) == 5
    # dup: two matches with one queryIdx
    raw = bs.oracle(q, c["dup"], bs.TRACK, 0.75, True)
    assert sorted(m[0] for m in raw) == [5, 5, 6] and len({m[1] for m in raw}) == 3
    # edge: one candidate (second == INT_MAX), 0 / 0 accepted, ratio 1 rejected
    assert bs.best_second(q, c["edge"], 0) == (3, bs.INT_MAX, 1)
    assert bs.best_second(q, c["edge"], 1) == (0, 0, 2)
    assert bs.best_second(q, c["edge"], 2) == (4, 4, 2)
    assert bs.oracle(q, c["edge"], bs.TRACK, 0.75, True) == [(20, 0, 3), (21, 1, 0)]
    # disjoint: no common node, no match in any mode
    assert not set(c["disjoint"]["fv"][0].tolist()) & set(q["fv"][0].tolist())
    assert all(bs.oracle(q, c["disjoint"], m, 0.75, True) == [] for m in bs.MODES.values())
    # emptied: TRACK's filter removes every query feature of node 70, so the keyframe's feature there is skipped; LOOP matches it
    assert bs.best_second(q, c["emptied"], 0, bs.TRACK)[2] == 0
    assert bs.oracle(q, c["emptied"], bs.TRACK, 0.75, True) == [(1, 1, 0)]
    assert bs.oracle(q, c["emptied"], bs.LOOP, 0.75, True) == [(1, 1, 0), (25, 0, 0)]
    assert bs.oracle(q, c["emptied"], bs.ADD, 0.75, True) == [(1, 1, 0)]


# ---- 2. the header without HIP, stand-alone ------------------------------------------------------------------------------------------------
def _bits(v):
    return "%x" % int(np.asarray(v, F32).view(np.uint32))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_bow_angle_header_stand_alone(tmp_path):
    """tests/cpp/test_bow_angle.cpp: csrc/bow_angle.h has no HIP in it, so the device's bin function and three-bin choice run here, with the
    host compiler's address and undefined-behaviour sanitizers when this g++ has their runtimes (a stand-alone program; nothing of it is
    loaded into python), against the cases and answers of the restatement above"""
    rng = np.random.default_rng(11)
    lines = []
    aq = bs.wrap_angle(rng.uniform(-180, 180, 4000))
    at = bs.wrap_angle(rng.uniform(-180, 180, 4000))
    pairs = list(zip(aq, at))
    for a in (F32(-179.5), F32(0), F32(10), F32(33.25), F32(180)):          # on, just below and just above every bin border
        for k in range(-15, 31):
            t = F32(a - F32(12 * k))
            if -180 < t <= 180:
                pairs += [(a, t), (a, np.nextafter(t, F32(1000))), (a, np.nextafter(t, F32(-1000)))]
    pairs += [(F32(10), np.nextafter(F32(10), F32(20))), (F32(180), F32(-179.99)), (F32(-179.99), F32(180)), (F32(0), F32(0))]
    n30 = 0
    for a, t in pairs:
        d = F32(a) - F32(t)
        d = d if d >= 0 else F32(360) + d
        n30 += int(d / F32(12)) == 30
        lines.append(f"P {_bits(a)} {_bits(t)} {angle_bin(a, t)}")
    assert n30 >= 5                                                          # bin 30 is among the cases
    counts = [np.zeros(30, int), np.ones(30, int), np.arange(30), np.arange(30)[::-1].copy()]
    for _ in range(300):
        c = rng.integers(0, int(rng.integers(1, 6)), 30)                     # small ranges: ties everywhere, many empty bins
        c[rng.random(30) < rng.random()] = 0
        counts.append(c)
    for k in (1, 2):                                                          # fewer than three non-empty bins
        c = np.zeros(30, int)
        c[rng.choice(30, k, replace=False)] = 7
        counts.append(c)
    for c in counts:
        lines.append("C " + " ".join(str(int(v)) for v in c) + " %x" % sum(1 << b for b in choose_bins(list(c))))
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    src = os.path.join(ROOT, "tests", "cpp", "test_bow_angle.cpp")
    exe = str(tmp_path / "t")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "orb_slam2_ros2_amd", "csrc"), "-o", exe, src]
    mode = "address + undefined-behaviour sanitizers"
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        # only a g++ WITHOUT the sanitizers' runtimes (the link step cannot find libasan / libubsan) may run the program plain; anything
        # else the sanitized build says is a failure of this test
        assert re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S* ?: No such file", r.stderr), r.stderr[-3000:]
        mode = "no sanitizer runtime on this machine: plain build"
        subprocess.check_call(base, timeout=300)
    print("test_bow_angle.cpp:", mode)
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["OK", str(len(pairs)), str(len(counts))], (r.stdout + r.stderr)[-2000:]


# ---- 3. surface ----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    from orb_slam2_ros2_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)                       # loading must not need a GPU
    assert re.search(r"\borbfe_status\s+orbfe_search_by_bow_stored\s*\(", hdr)
    assert hasattr(lib, "orbfe_search_by_bow_stored") and "orbfe_search_by_bow_stored" in _lib.EXPORTS
    for typ in ("orbfe_bow_query", "orbfe_bow_match"):
        assert re.search(r"\}\s*" + typ + r"\s*;", hdr), typ
    for name, val in (("ORBFE_BOW_SEARCH_MAX_KF", 64), ("ORBFE_BOW_TRACK", 0), ("ORBFE_BOW_LOOP", 1), ("ORBFE_BOW_ADD", 2)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(val) + r"\b", hdr), name
    assert "#define ORBFE_ABI_VERSION 4" in hdr and lib.orbfe_abi_version() == 4


def test_bindings_exist_and_mirror_the_structures():
    from orb_slam2_ros2_amd import _lib
    assert callable(_lib.Context.search_by_bow_stored) and callable(ORBMatcher.searchByBowStored)
    # the C layout (x86-64 / LP64): int32 (+4) | uint64 | int32 (+4) | 2 pointers | int32 (+4) | 4 pointers; three int32
    assert ctypes.sizeof(_lib.BowQuery) == 8 + 8 + 8 + 16 + 8 + 32 and _lib.BowQuery.id.offset == 8 and _lib.BowQuery.flags.offset == 72
    assert _lib.BOW_MATCH_DTYPE.itemsize == 12 and _lib.BOW_MATCH_DTYPE.names == ("query", "train", "distance")
    assert (_lib.BOW_SEARCH_MAX_KF, _lib.BOW_TRACK, _lib.BOW_LOOP, _lib.BOW_ADD) == (64, 0, 1, 2)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include", "ORB_SLAM2")) or shutil.which("g++") is None,
                    reason="needs the reference tree and g++")
def test_dropin_compiles_against_the_reference_headers(tmp_path):
    """g++ -fsyntax-only of tests/cpp/ref_bowsearch_body.cpp: orbfe_reloc_dropin.hpp with the reference's Tracking.h / LoopClosing.h /
    KeyFrame.h / Frame.h / MapPoint.h (symlinks; Frame.h / KeyFrame.h as temporary copies with INTEGRATION section 3's friend line) and the
    two bodies of INTEGRATION section 13"""
    from test_reference_compile import _include_dir
    inc = _include_dir(str(tmp_path / "inc"), friend_line=True)
    stubs = os.path.join(ROOT, "tests", "cpp", "stubs")
    host = os.path.join(ROOT, "orb_slam2_ros2_amd", "host")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + inc, "-I" + stubs, "-I" + os.path.join(stubs, "refgen"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(ROOT, "tests", "cpp", "ref_bowsearch_body.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
