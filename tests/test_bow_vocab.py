"""The bag-of-words path without a device: the ORB-SLAM2 text vocabulary parser (orbfe_vocab_load_txt / export) against the arrays
orb_slam2_ros2_amd.synth_vocab generated, every rejection rule, DBoW's L1 score of the DBoW3 drop-in header against tests/bow_restatement.py,
and the reference's own Frame.cc / KeyFrameDB.cc through the compiler with the drop-in header ahead of the stand-ins."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from bow_restatement import score_l1
from orb_slam2_ros2_amd import synth_vocab
from orb_slam2_ros2_amd._lib import OrbfeError, Vocabulary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = os.path.join(ROOT, "orb_slam2_ros2_amd", "host", "compat")
STUBS = os.path.join(ROOT, "tests", "cpp", "stubs")


def _same_as_generated(path, voc):
    v = Vocabulary.load_txt(str(path))
    info = v.info()
    assert (info["k"], info["L"], info["n_nodes"], info["n_words"]) == (voc["k"], voc["L"], len(voc["parent"]), int(voc["is_leaf"].sum()))
    got = v.export()
    for key in ("parent", "is_leaf", "desc", "word_id"):
        assert np.array_equal(got[key], voc[key]), key
    assert np.array_equal(got["weight"].view(np.int64), voc["weight"].view(np.int64))
    v.close()


@pytest.mark.parametrize("name", ["trained", "edge", "edge_k2_L10", "edge_k20_L1", "full_k10_L5", "trained_dfs"])
def test_parser_export_equals_the_generator(tmp_path, name):
    voc = {"trained": lambda: synth_vocab.trained(0, L=4), "edge": lambda: synth_vocab.edge(1, 4, 5),
           "edge_k2_L10": lambda: synth_vocab.edge(2, 2, 10), "edge_k20_L1": lambda: synth_vocab.edge(3, 20, 1),
           "full_k10_L5": lambda: synth_vocab.full(4, 10, 5),
           "trained_dfs": lambda: synth_vocab.reorder_dfs(synth_vocab.trained(0, L=4))}[name]()
    if name == "full_k10_L5":
        assert len(voc["parent"]) == 111111
    if name == "trained_dfs":   # parents still before their children, but not breadth-first
        depth = np.zeros(len(voc["parent"]), np.int64)
        for i in range(1, len(depth)):
            assert voc["parent"][i] < i
            depth[i] = depth[voc["parent"][i]] + 1
        assert np.any(np.diff(depth) < 0)
    p = tmp_path / "voc.txt"
    synth_vocab.write_txt(p, voc)
    _same_as_generated(p, voc)


def test_edge_vocabulary_has_every_corner():
    voc = synth_vocab.edge(1, 4, 5)
    ch = synth_vocab.children(voc)
    depth = np.zeros(len(voc["parent"]), np.int64)
    for i in range(1, len(depth)):
        depth[i] = depth[voc["parent"][i]] + 1
    leaves = voc["is_leaf"] == 1
    assert set(depth[leaves].tolist()) == set(range(1, 6))                         # leaves at every level
    assert any(len(c) == 1 for c in ch)                                            # single-child chains
    assert np.any(leaves & (voc["weight"] == 0))                                   # zero-weight leaves
    assert any(len({bytes(voc["desc"][j]) for j in c}) < len(c) for c in ch if c)  # identical siblings


@pytest.mark.parametrize("k,L", [(20, 1), (19, 3)])
def test_edge_vocabulary_has_a_node_beyond_sixteen_children(k, L):
    """the descent's lane j takes children j and j + 16: a node with more than 16 children, exact ties between a child below 16 and one
    from 16 on (in the same lane and in other lanes), and a child from 16 on that only it can win"""
    voc = synth_vocab.edge(3 if k == 20 else 6, k, L)   # the seeds the GPU tests use
    root = synth_vocab.children(voc)[0]
    assert len(root) == k > 16
    d = [bytes(voc["desc"][j]) for j in root]
    ties = [(c, d.index(d[c])) for c in range(16, k) if d.index(d[c]) < 16]
    assert any(c - 16 == e for c, e in ties) and any(c - 16 != e for c, e in ties)
    assert any(d.index(d[c]) == c and voc["weight"][root[c]] > 0 for c in range(16, k))


def test_blank_lines_are_skipped(tmp_path):
    voc = synth_vocab.edge(5, 3, 3)
    p = tmp_path / "v.txt"
    synth_vocab.write_txt(p, voc)
    lines = p.read_text().split("\n")
    p.write_text("\n".join(lines[:3] + ["", "   \t"] + lines[3:]) + "\n\n\r\n")
    _same_as_generated(p, voc)


GOOD = "3 2 0 0\n" + "0 0 " + "1 " * 32 + "0\n" + "0 1 " + "2 " * 32 + "0.5\n" + "1 1 " + "3 " * 32 + "1.5\n"


@pytest.mark.parametrize("text,what", [
    ("3 2 0\n", "malformed header"),
    ("x 2 0 0\n", "malformed header"),
    ("1 2 0 0\n0 1 " + "2 " * 32 + "1\n", "k outside"),
    ("21 2 0 0\n0 1 " + "2 " * 32 + "1\n", "k outside"),
    ("3 0 0 0\n0 1 " + "2 " * 32 + "1\n", "L outside"),
    ("3 11 0 0\n0 1 " + "2 " * 32 + "1\n", "L outside"),
    ("3 2 1 0\n0 1 " + "2 " * 32 + "1\n", "scoring / weighting"),
    ("3 2 0 2\n0 1 " + "2 " * 32 + "1\n", "scoring / weighting"),
    ("3 2 0 0\n1 1 " + "2 " * 32 + "1\n", "parent id"),
    ("3 2 0 0\n0 1 " + "2 " * 32 + "1\n1 1 " + "2 " * 32 + "1\n", "parent is a leaf"),
    ("2 2 0 0\n" + ("0 1 " + "2 " * 32 + "1\n") * 3, "more than k children"),
    ("3 2 0 0\n0 0 " + "2 " * 32 + "0\n", "no children"),
    ("3 2 0 0\n", "no children"),
    ("3 2 0 0\n0 0 " + "2 " * 32 + "0\n1 0 " + "2 " * 32 + "0\n2 1 " + "2 " * 32 + "1\n", "depth > L"),
    ("3 2 0 0\n0 1 " + "2 " * 31 + "256 1\n", "outside 0..255"),
    ("3 2 0 0\n0 1 " + "2 " * 31 + "-1 1\n", "outside 0..255"),
    ("3 2 0 0\n0 1 " + "2 " * 20 + "\n", "truncated"),
    ("3 2 0 0\n0 1 " + "2 " * 32 + "\n", "truncated"),
    ("3 2 0 0\n0 2 " + "2 " * 32 + "1\n", "is_leaf"),
    ("3 2 0 0\n0 1 " + "2 " * 32 + "nan\n", "weight"),
    ("3 2 0 0\n0 1 " + "2 " * 32 + "inf\n", "weight"),
    ("3 2 0 0\n0 1 " + "2 " * 32 + "0x1p3\n", "weight"),
    ("3 2 0 0\n0 1 " + "2 " * 32 + "1,5\n", "weight"),
    ("3 2 0 0\n0 1 " + "2 " * 32 + "1e\n", "weight"),
    ("3 2 0 0\n0 1 " + "2 " * 32 + "+-1\n", "weight"),
])
def test_rejections(tmp_path, text, what):
    p = tmp_path / "bad.txt"
    p.write_text(text)
    with pytest.raises(OrbfeError) as ei:
        Vocabulary.load_txt(str(p))
    assert ei.value.status == 1 and what in str(ei.value), str(ei.value)    # ORBFE_EBADARG with the reason


def test_weights_are_decimal_numbers_read_exactly(tmp_path):
    """[+-]digits[.digits][e[+-]digits], correctly rounded (the same double Python's float() gives)"""
    ws = ["+1.5e-3", "-0.25", "3", "0.1", "2.5E+2", "7.", ".5", "1e-310", "0.30000000000000004"]
    p = tmp_path / "w.txt"
    p.write_text("20 1 0 0\n" + "".join("0 1 " + f"{i} " * 32 + w + "\n" for i, w in enumerate(ws)))
    e = Vocabulary.load_txt(str(p)).export()
    assert e["weight"][1:].tolist() == [float(w) for w in ws]


def test_minimal_good_file_and_missing_file(tmp_path):
    p = tmp_path / "good.txt"
    p.write_text(GOOD)
    v = Vocabulary.load_txt(str(p))
    assert v.info() == dict(k=3, L=2, n_nodes=4, n_words=2)
    e = v.export()
    assert e["parent"].tolist() == [-1, 0, 0, 1] and e["word_id"].tolist() == [-1, -1, 0, 1] and e["weight"].tolist() == [0, 0, 0.5, 1.5]
    with pytest.raises(OrbfeError) as ei:
        Vocabulary.load_txt(str(tmp_path / "missing.txt"))
    assert ei.value.status == 1


def _build_bow(tmp_path):
    exe = str(tmp_path / "test_bow")
    pkg = os.path.join(ROOT, "orb_slam2_ros2_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + COMPAT, "-I" + STUBS, "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_bow.cpp"),
                           "-L" + pkg, "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _random_bow(rng, n_words):
    words = np.unique(rng.integers(0, n_words, rng.integers(0, 60)))
    vals = rng.random(len(words))
    if len(words):
        vals = vals / vals.sum()
    return {int(w): float(v) for w, v in zip(words, vals)}


def test_compat_header_score_equals_the_restatement(tmp_path):
    """DBoW3::Vocabulary(path), size(), empty() and score() of the drop-in header: host only, no device"""
    voc = synth_vocab.edge(7, 4, 4)
    p = tmp_path / "v.txt"
    synth_vocab.write_txt(p, voc)
    rng = np.random.default_rng(11)
    n_words = int(voc["is_leaf"].sum())
    pairs = []
    for i in range(300):
        a = _random_bow(rng, n_words)
        b = _random_bow(rng, n_words) if i % 3 else {**a, **{w: v * 0.5 for w, v in list(a.items())[::2]}}
        pairs.append((a, b))
    with open(tmp_path / "vec.txt", "w") as f:
        f.write(f"{len(pairs)}\n")
        for a, b in pairs:
            for v in (a, b):
                f.write(f"{len(v)} " + " ".join(f"{w} {int(np.float64(x).view(np.uint64)):016x}" for w, x in v.items()) + "\n")
    r = subprocess.run([_build_bow(tmp_path), "score", str(p), str(tmp_path / "vec.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[0].split() == ["SCORE_OK", str(n_words), "0"]
    got = [int(x, 16) for x in lines[1:1 + len(pairs)]]
    want = [int(np.float64(score_l1(a, b)).view(np.uint64)) for a, b in pairs]
    assert got == want
    assert any(0 < np.uint64(g).view(np.float64) < 1 for g in got)


# ---- the reference's own translation units against the drop-in header ------------------------------------------------------------
REF = "/root/reference/src/ORB_SLAM2"
_have_ref = os.path.isdir(os.path.join(REF, "include", "ORB_SLAM2")) and shutil.which("g++") is not None


def _ref_includes(tmp):
    d = os.path.join(tmp, "ORB_SLAM2")
    os.makedirs(d)
    src = os.path.join(REF, "include", "ORB_SLAM2")
    for f in os.listdir(src):
        if f != "ORBExtractor.h":
            os.symlink(os.path.join(src, f), os.path.join(d, f))
    with open(os.path.join(d, "ORBExtractor.h"), "w") as fh:
        fh.write("#pragma once\n#include <orbfe_dropin.hpp>      // ORB_SLAM2_ROS2::ORBExtractor on liborbfe_hip.so\n")
    return tmp


def _syntax_only(inc, tu, compat, extra=()):
    first = ["-I" + COMPAT] if compat else []
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", *extra, *first, "-I" + inc, "-I" + STUBS, "-I" + os.path.join(STUBS, "refgen"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "orb_slam2_ros2_amd", "host"), tu],
                          capture_output=True, text=True, timeout=600)


@pytest.mark.skipif(not _have_ref, reason="needs /root/reference (build container only) and g++")
@pytest.mark.parametrize("tu", ["Frame.cc", "KeyFrameDB.cc"])
def test_reference_sources_compile_against_the_dbow3_drop_in(tmp_path, tu):
    inc = _ref_includes(str(tmp_path / "inc"))
    path = os.path.join(REF, "src", tu)
    r = _syntax_only(inc, path, compat=True)
    assert r.returncode == 0, r.stderr[-4000:]
    # the drop-in is what the compiler took: -H lists every header opened
    r = _syntax_only(inc, path, compat=True, extra=("-H",))
    assert os.path.join(COMPAT, "DBoW3", "DBoW3.h") in r.stderr and os.path.join(STUBS, "DBoW3", "DBoW3.h") not in r.stderr
    # control: without the compat directory the same file resolves to the stand-in
    r = _syntax_only(inc, path, compat=False, extra=("-H",))
    assert r.returncode == 0 and os.path.join(STUBS, "DBoW3", "DBoW3.h") in r.stderr and os.path.join(COMPAT, "DBoW3", "DBoW3.h") not in r.stderr
