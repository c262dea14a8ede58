"""orbfe_create_new_map_points on the device against tests/triangulation_restatement.py, bit for bit: records (count, order, neighbour,
query, train, kind, xyz as int32 views) and the tail list."""
import os
import sys
import tempfile
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tri_scenes as ts  # noqa: E402
import triangulation_restatement as tr  # noqa: E402
from orb_slam2_ros2_amd import synth_vocab  # noqa: E402
from orb_slam2_ros2_amd._lib import Context, OrbfeError, Vocabulary  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
    yield c
    c.close()


def run(ctx, cur, nbs, bl=ts.BL, **kw):
    return ctx.create_new_map_points(cur, nbs, ts.CAM, ts.k_inv(), bl, ts.SF, **kw)


def same(ctx, cur, nbs, bl=ts.BL):
    got, gtail, gcons = run(ctx, cur, nbs, bl)
    want, wtail, _, wcons = tr.create_new_map_points(cur, nbs, ts.CAM, ts.k_inv(), bl, ts.SF)
    assert np.array_equal(gcons, wcons)
    assert len(got) == len(want)
    for f in ("nb", "q", "t", "kind"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["xyz"].view(np.int32), want["xyz"].view(np.int32))
    assert np.array_equal(gtail, wtail)
    return got, gtail


@pytest.mark.parametrize("seed", [0, 1])
def test_full_size_bit_exact(ctx, seed):
    cur, nbs, _ = ts.scene(seed, n_nb=10, n=2000)
    got, tail = same(ctx, cur, nbs)
    assert len(got) > 200 and set(np.unique(got["kind"])) == {1, 2, 3} and len(tail) > 0


def test_full_size_device_featurevectors(ctx, tmp_path):
    voc = synth_vocab.full(0, 10, 4)
    p = str(tmp_path / "voc.txt")
    synth_vocab.write_txt(p, voc)
    v = Vocabulary.load_txt(p)
    cur, nbs, _ = ts.scene(7, n_nb=10, n=2000)
    for kf in [cur] + nbs:
        kf["fv"] = ctx.bow_transform(v, kf["desc"], 2)[2:]
    got, _ = same(ctx, cur, nbs)
    assert len(got) > 100


def test_edges(ctx):
    cur, nbs, _ = ts.scene(3, n_nb=3, n=600, n_pts=2000)
    assert len(same(ctx, cur, [])[0]) == 0                                    # no neighbours
    far = dict(nbs[0], fv=(nbs[0]["fv"][0] + np.uint32(100000), nbs[0]["fv"][1], nbs[0]["fv"][2]))
    assert len(same(ctx, cur, [far])[0]) == 0                                  # no common node
    full = dict(cur, flags=np.full(len(cur["kps"]), 3, np.uint8))
    assert len(same(ctx, full, nbs)[0]) == 0                                   # every current feature holds a good in-map point
    got, tail = same(ctx, cur, nbs, bl=np.float32(100.0))                      # every neighbour below the baseline
    assert len(got) == 0 and np.array_equal(tail, np.flatnonzero(cur["unproc"] & ((cur["flags"] & 1) == 0)))


def test_max_neighbours_and_capacity(ctx):
    cur, nbs, _ = ts.scene(4, n_nb=64, n=300, n_pts=900, baselines=list(np.linspace(0.06, 1.0, 64)))
    got, tail = same(ctx, cur, nbs)
    assert len(got) > 10
    with pytest.raises(OrbfeError) as ei:
        run(ctx, cur, nbs, cap=len(got) - 1)
    assert ei.value.status == 4 and ctx.last_counts == (len(got), len(tail))
    with pytest.raises(OrbfeError) as ei:
        run(ctx, cur, nbs + nbs[:1])
    assert ei.value.status == 1


def test_bad_arguments(ctx):
    cur, nbs, _ = ts.scene(5, n_nb=2, n=200, n_pts=600)
    nodes, offs, feats = nbs[0]["fv"]
    for bad in (dict(nbs[0], fv=(nodes[::-1].copy(), offs, feats)), dict(nbs[0], fv=(nodes, offs, feats + np.uint32(10000)))):
        with pytest.raises(OrbfeError) as ei:
            run(ctx, cur, [bad])
        assert ei.value.status == 1
    kps = nbs[1]["kps"].copy()
    kps["octave"][0] = 8
    with pytest.raises(OrbfeError) as ei:
        run(ctx, cur, [dict(nbs[1], kps=kps)])
    assert ei.value.status == 1 and "octave" in str(ei.value)


def test_quirk_constructions_at_scale(ctx):
    from test_triangulation_host import t4_scene, t5_scene
    for cur, nbs in (t4_scene(), t5_scene()):
        same(ctx, cur, nbs)


def test_two_threads_two_contexts():
    cur, nbs, _ = ts.scene(6, n_nb=10, n=1500)
    out = [None, None]

    def work(i):
        c = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
        try:
            out[i] = [run(c, cur, nbs) for _ in range(3)]
        finally:
            c.close()
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    ref = out[0][0]
    for res in out[0] + out[1]:
        assert res[0].tobytes() == ref[0].tobytes() and np.array_equal(res[1], ref[1]) and np.array_equal(res[2], ref[2])


def test_dropin_over_minimal_types(tmp_path):
    """tests/cpp/test_tri_dropin.cpp: the drop-in over minimal KeyFrame / MapPoint / Map types; the map points it creates (positions,
    which slots got them, in mlpAddedMPs order) equal the restatement over the same keyframes in the drop-in's neighbour order"""
    import subprocess
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cur, nbs, _ = ts.scene(8, n_nb=6, n=800, n_pts=2500)
    f = lambda v: repr(float(v))  # noqa: E731
    lines = [" ".join(f(v) for v in ts.CAM), " ".join(f(v) for v in ts.k_inv().reshape(9)), f(ts.BL), f"{len(ts.SF)} " + " ".join(f(v) for v in ts.SF),
             str(1 + len(nbs))]
    for k, kf in enumerate([cur] + nbs):
        lines.append(f"{len(kf['kps'])} " + " ".join(f(v) for v in np.concatenate([kf["Tcw"].reshape(16), kf["Twc"].reshape(16), kf["Ow"]])))
        for i, kp in enumerate(kf["kps"]):
            s = f"{f(kp['x'])} {f(kp['y'])} {int(kp['octave'])} {f(kf['depth'][i])} {f(kf['right_u'][i])} {int(kf['flags'][i])} " + \
                " ".join(str(int(b)) for b in kf["desc"][i])
            if k == 0:
                s += f" {int(kf['unproc'][i])} " + " ".join(f(v) for v in kf["unproc_pos"][i])
            lines.append(s)
        nodes, offs, feats = kf["fv"]
        lines.append(str(len(nodes)))
        for j in range(len(nodes)):
            lines.append(f"{int(nodes[j])} {offs[j + 1] - offs[j]} " + " ".join(str(int(x)) for x in feats[offs[j]:offs[j + 1]]))
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    pkg = os.path.join(ROOT, "orb_slam2_ros2_amd")
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), "-I" + os.path.join(pkg, "host"),
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_tri_dropin.cpp"), "-L" + pkg,
                           "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.strip().splitlines()
    order = [int(x) for x in out[0].split()]
    want, wtail, _, _ = tr.create_new_map_points(cur, [nbs[i] for i in order], ts.CAM, ts.k_inv(), ts.BL, ts.SF)
    got = [ln.split() for ln in out[1:]]
    assert len(got) == len(want) + len(wtail) and len(want) > 20
    for g, w in zip(got, want):
        xyz = " ".join(f"{int(v):08x}" for v in w["xyz"].view(np.uint32))
        assert g == [str(w["q"]), str(order[w["nb"]]), str(w["t"]), "1" if w["kind"] == tr.KIND_OWN else "0", *xyz.split(), "1"]
    tail = got[len(want):]
    assert sorted(int(g[0]) for g in tail) == list(wtail) and all(g[1:4] == ["-1", "-1", "1"] and g[-1] == "1" for g in tail)
