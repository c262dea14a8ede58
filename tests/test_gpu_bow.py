"""The bag-of-words transform on the device (orbfe_bow_transform / orbfe_bow_slots, the DBoW3 drop-in header) bit-equal to the plain
restatement of DBoW's rules (tests/bow_restatement.py) over the generator's arrays: words, nodes, offsets and features as equal arrays,
values as equal int64 views."""
import os
import subprocess
import threading

import numpy as np
import pytest

import bow_restatement as R
from orb_slam2_ros2_amd import synth, synth_vocab
from orb_slam2_ros2_amd._lib import Context, OrbfeError, Vocabulary

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vocs(tmp_path_factory):
    d = tmp_path_factory.mktemp("voc")
    gen = {"trained": synth_vocab.trained(0, k=10, L=4), "edge": synth_vocab.edge(1, 4, 5), "edge_k2_L10": synth_vocab.edge(2, 2, 10),
           "edge_k20_L1": synth_vocab.edge(3, 20, 1), "edge_k19_L3": synth_vocab.edge(6, 19, 3), "full_k10_L5": synth_vocab.full(4, 10, 5)}
    out = {}
    for name, voc in gen.items():
        p = d / f"{name}.txt"
        synth_vocab.write_txt(p, voc)
        out[name] = (voc, Vocabulary.load_txt(str(p)), str(p))
    return out


@pytest.fixture(scope="module")
def ctx():
    c = Context(1241, 376, n_features=2000, n_levels=8, device_id=0, max_images=64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def frames(ctx):
    """product descriptors: the left images of 64 synth frames (the four content classes in turn) extracted in one batch into slots 0..63"""
    imgs = [synth.stereo_pair_content(f, synth.CONTENT_CLASSES[f % 4])[0] for f in range(64)]
    return ctx.extract_batch(imgs)


def _check(got, voc, desc, levelsup, what=""):
    R.assert_same(got, R.transform(voc, desc, levelsup), what)


@pytest.mark.parametrize("levelsup", [0, 1, 3, 4, 7])   # L = 4: 0, 1, L - 1, L (= 4), L + 3
def test_trained_vocabulary_on_product_descriptors(ctx, vocs, frames, levelsup):
    voc, v, _ = vocs["trained"]
    for i in range(4):   # one frame of every content class
        d = frames[i][1]
        assert len(d) > 100
        got = ctx.bow_transform(v, d, levelsup)
        _check(got, voc, d, levelsup, f"frame {i} levelsup {levelsup}")
        assert len(got[0]) > 10 and (len(got[2]) > 5 if levelsup < voc["L"] else got[2].tolist() == [0])   # the root from L - levelsup <= 0


@pytest.mark.parametrize("name", ["edge", "edge_k2_L10", "edge_k20_L1", "edge_k19_L3"])
def test_edge_vocabularies_with_exact_ties(ctx, vocs, name):
    voc, v, _ = vocs[name]
    rng = np.random.default_rng(5)
    nodes = rng.integers(1, len(voc["parent"]), 1500)
    d = np.concatenate([rng.integers(0, 256, (1500, 32), dtype=np.uint8), voc["desc"][nodes]])   # copies of node descriptors: ties
    d = d[rng.permutation(len(d))]
    for levelsup in (0, 1, 2, voc["L"] - 1, voc["L"], voc["L"] + 3):
        _check(ctx.bow_transform(v, d, levelsup), voc, d, levelsup, f"{name} levelsup {levelsup}")
    if voc["k"] > 16:   # the descent really reached a child from index 16 on (k = 20, L = 1: the nodes are the root's children)
        root = synth_vocab.children(voc)[0]
        leaf, _ = R.descend(voc, d, 0)
        assert np.isin(leaf, root[16:]).any() and np.isin(leaf, root[:16]).any()


@pytest.mark.parametrize("n", [0, 1, 2, 2000, 20000, 65535])
def test_feature_counts(ctx, vocs, n):
    voc, v, _ = vocs["trained"]
    rng = np.random.default_rng(n)
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if n > 10:
        d[: n // 4] = d[0]   # a word hit many times: the run sum of w + w + ..
    got = ctx.bow_transform(v, d, 2)
    _check(got, voc, d, 2, f"n {n}")
    if n == 0:
        assert all(len(a) == 0 for a in (got[0], got[1], got[2], got[4])) and got[3].tolist() == [0]


def test_above_the_limit_is_refused(ctx, vocs):
    _, v, _ = vocs["trained"]
    with pytest.raises(OrbfeError) as ei:
        ctx.bow_transform(v, np.zeros((65536, 32), np.uint8), 4)
    assert ei.value.status == 4   # ORBFE_ECAPACITY, never a truncated result


def test_k10_L5_vocabulary(ctx, vocs):
    voc, v, _ = vocs["full_k10_L5"]
    d = np.random.default_rng(9).integers(0, 256, (2000, 32), dtype=np.uint8)
    for levelsup in (0, 2, 4):
        _check(ctx.bow_transform(v, d, levelsup), voc, d, levelsup, f"k10 L5 levelsup {levelsup}")


def test_bow_slots_equals_bow_transform_of_the_fetched_descriptors(ctx, vocs, frames):
    voc, v, _ = vocs["trained"]
    res = ctx.bow_slots(v, 0, 64, 4)
    assert len(res) == 64
    for i, (_, d) in enumerate(frames):
        R.assert_same(res[i], ctx.bow_transform(v, d, 4), f"slot {i}")
    for i in (0, 31, 63):
        _check(res[i], voc, frames[i][1], 4, f"slot {i}")
    part = ctx.bow_slots(v, 10, 5, 1)
    for j in range(5):
        _check(part[j], voc, frames[10 + j][1], 1, f"slot {10 + j}")
    left = ctx.bow_slots(v, 0, 32, 4, step=2)   # every other slot: the left images of 32 stereo pairs
    for j in range(32):
        R.assert_same(left[j], res[2 * j], f"step 2, slot {2 * j}")
    odd = ctx.bow_slots(v, 1, 21, 2, step=3)
    for j in (0, 10, 20):
        _check(odd[j], voc, frames[1 + 3 * j][1], 2, f"step 3, slot {1 + 3 * j}")
    for bad in (dict(slot0=0, n=33, step=2), dict(slot0=2, n=32, step=2), dict(slot0=0, n=2, step=0)):
        with pytest.raises(OrbfeError) as ei:
            ctx.bow_slots(v, bad["slot0"], bad["n"], 4, step=bad["step"])
        assert ei.value.status == 1, bad


def test_two_threads_on_two_contexts_share_one_vocabulary(vocs, frames):
    voc, v, _ = vocs["trained"]
    descs = [frames[i][1] for i in range(8)]
    want = [R.transform(voc, d, 4) for d in descs]
    errors = []

    def worker(seed):
        try:
            c = Context(640, 480, n_features=500, n_levels=4, device_id=0, max_images=1)
            for it in range(200):
                k = (it * 3 + seed) % len(descs)
                R.assert_same(c.bow_transform(v, descs[k], 4), want[k], f"thread {seed} call {it}")
            c.close()
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(s,)) for s in (0, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors[0]


@pytest.fixture(scope="module")
def bow_exe(tmp_path_factory):
    from test_bow_vocab import _build_bow
    return _build_bow(tmp_path_factory.mktemp("bowexe"))


def _parse_transform(out):
    lines = out.strip().split("\n")
    head = lines[0].split()
    assert head[0] == "TRANSFORM_OK" and head[1] == "1", lines[0]
    nw, nn = int(head[2]), int(head[3])
    W = [l.split() for l in lines[1:1 + nw]]
    N = [l.split() for l in lines[1 + nw:1 + nw + nn]]
    words = np.array([int(w[1]) for w in W], np.uint32)
    values = np.array([int(w[2], 16) for w in W], np.uint64).view(np.float64)
    nodes = np.array([int(n[1]) for n in N], np.uint32)
    feats = [np.array([int(x) for x in n[2:]], np.uint32) for n in N]
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int32)
    return words, values, nodes, offsets, (np.concatenate(feats) if feats else np.zeros(0, np.uint32)).astype(np.uint32)


def test_compat_header_transform_on_the_device(ctx, vocs, frames, bow_exe, tmp_path):
    voc, v, path = vocs["trained"]
    d = frames[2][1]
    (tmp_path / "d.raw").write_bytes(d.tobytes())
    r = subprocess.run([bow_exe, "transform", path, str(tmp_path / "d.raw"), str(len(d)), "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _parse_transform(r.stdout)
    R.assert_same(got, ctx.bow_transform(v, d, 4), "DBoW3::Vocabulary::transform vs the Python path")
    R.assert_same(got, R.transform(voc, d, 4), "DBoW3::Vocabulary::transform vs the restatement")


def test_search_by_bow_with_device_made_feature_vectors(vocs, frames, bow_exe, tmp_path):
    voc, _, path = vocs["trained"]
    dF = frames[4][1]
    dK = dF[np.random.default_rng(3).permutation(len(dF))]   # the same features in another order: many matches
    for name, d in (("f", dF), ("k", dK)):
        (tmp_path / f"{name}.raw").write_bytes(d.tobytes())
        _, _, nodes, off, feats = R.transform(voc, d, 4)
        with open(tmp_path / f"fv_{name}.txt", "w") as fh:
            fh.write(f"{len(nodes)}\n")
            for i, nd in enumerate(nodes):
                fl = feats[off[i]:off[i + 1]]
                fh.write(f"{nd} {len(fl)} " + " ".join(str(x) for x in fl) + "\n")
    r = subprocess.run([bow_exe, "searchbow", path, str(tmp_path / "f.raw"), str(len(dF)), str(tmp_path / "k.raw"), str(len(dK)),
                        str(tmp_path / "fv_f.txt"), str(tmp_path / "fv_k.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    assert f[0] == "SEARCHBOW_OK" and f[1] == f[2] and f[3:] == ["1", "1"], r.stdout
    assert int(f[1]) > 0
