"""orbfe_fuse_into_keyframes on the device against tests/fuse_restatement.py (the CPU oracle's single calls composed), bit for bit:
best_idx, best_dist and visible are integers and flags, so there is no tolerance."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_restatement as fr  # noqa: E402
import fuse_scenes as fs  # noqa: E402
from orb_slam2_ros2_amd._lib import Context, OrbfeError  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
    yield c
    c.close()


def run(ctx, sc, **kw):
    return ctx.fuse_into_keyframes(sc["cur"], sc["pts"], sc["targets"], sc["z"], fs.CAM, fs.BL, fs.SF, **kw)


def same(ctx, orc, sc):
    got = run(ctx, sc)
    want = fr.fuse_into_keyframes(orc, sc["cur"], sc["pts"], sc["targets"], sc["z"], fs.CAM, fs.BL, fs.SF)
    for g, w, what in zip(got, want, ("best_idx", "best_dist", "visible")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), what
    return got


@pytest.mark.parametrize("name", fs.GPU_SCENES)   # K in {3, 4, 6, 61, 64}, cur->n in {1, 63, 64, 65, 300, 400, 2000}, targets of 0 / 1 / 500 features
def test_bit_exact(ctx, orc, name):
    bi, _, _ = same(ctx, orc, fs.gpu_scene(name))
    assert (bi >= 0).any()


def test_one_target_at_a_time(ctx, orc):
    sc = fs.gpu_scene("k3")
    for k in range(3):                               # K = 1, once per octave-window case
        same(ctx, orc, dict(sc, targets=sc["targets"][k:k + 1], z=sc["z"][k:k + 1]))


@pytest.mark.parametrize("count", [63, 64, 65, 200])
def test_dense_cell(ctx, orc, count):
    same(ctx, orc, fs.dense_cell_scene(count))


def test_borders(ctx, orc):
    same(ctx, orc, fs.border_scene())


@pytest.mark.parametrize("name", ["mid", "dense63", "dense64", "dense65", "dense200"])
def test_equals_the_per_keyframe_device_calls(ctx, name):
    """what the parent's entry points need 2 K calls for: project_map_points + search_in_area_features per target.  The two kernels
    share one area loop and differ in their filters: the dense cells put the chunk boundary, the carry and a third chunk under both"""
    sc = fs.gpu_scene("mid") if name == "mid" else fs.dense_cell_scene(int(name[5:]))
    cur, pts = sc["cur"], sc["pts"]
    bi, bd, vis = run(ctx, sc)
    octave = cur["kps"]["octave"].astype(np.int32)
    radius = (F32(3.0) * (fs.SF[octave] * fs.SF[octave])).astype(F32)
    qxy = np.stack([cur["kps"]["x"], cur["kps"]["y"]], 1)
    for k, t in enumerate(sc["targets"]):
        lo, hi = fr.octave_window(octave, sc["z"][k], fs.BL)
        b, d, s, nc = ctx.search_in_area_features(t["kps"], t["desc"], qxy, radius, lo, hi, cur["desc"], bounds=t["bounds"])
        ok = (nc > 0) & (d.astype(F32) / s.astype(F32) < F32(0.6)) & (d < 50)
        assert np.array_equal(bi[k], np.where(ok, b, -1)) and np.array_equal(bd[k], np.where(ok, d, 0))
        p = ctx.project_map_points(pts["pos"], pts["view_dir"], pts["max_dist"], pts["min_dist"], t["Rcw"], t["tcw"], fs.CAM, t["bounds"])
        assert np.array_equal(vis[k], np.where(pts["has_point"] > 0, p["visible"], 0))


def test_empty_inputs_leave_the_outputs_untouched(ctx):
    sc = fs.gpu_scene("k3")
    n = len(sc["cur"]["kps"])
    out = (np.full((0, n), 7, np.int32), np.full((0, n), 7, np.int32), np.full((0, n), 7, np.uint8))
    guard = [np.full((3, n), 7, a.dtype) for a in out]                      # (the call gets these: n_kf == 0 must not write through them)
    run(ctx, dict(sc, targets=[], z=np.zeros(0, F32)), out=tuple(guard))
    assert all((g == 7).all() for g in guard)
    empty = fs.cut(sc, np.arange(0))
    guard = [np.full((3, 4), 7, a.dtype) for a in out]
    run(ctx, empty, out=tuple(guard))
    assert all((g == 7).all() for g in guard)


def test_bad_arguments(ctx):
    sc = fs.gpu_scene("k3")
    with pytest.raises(OrbfeError) as ei:
        run(ctx, dict(sc, targets=[sc["targets"][0]] * 65, z=np.zeros(65, F32)))
    assert ei.value.status == 1
    kps = sc["targets"][1]["kps"].copy()
    kps["octave"][3] = 8
    with pytest.raises(OrbfeError) as ei:
        run(ctx, dict(sc, targets=[sc["targets"][0], dict(sc["targets"][1], kps=kps)], z=sc["z"][:2]))
    assert ei.value.status == 1 and "octave" in str(ei.value)
    with pytest.raises(OrbfeError) as ei:
        run(ctx, dict(sc, pts=dict(sc["pts"], view_dir=None)))
    assert ei.value.status == 1
    with pytest.raises(OrbfeError) as ei:
        run(ctx, dict(sc, z=None))
    assert ei.value.status == 1


def test_two_threads_two_contexts():
    sc = fs.gpu_scene("mid")
    out = [None, None]

    def work(i):
        c = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
        try:
            out[i] = [run(c, sc) for _ in range(3)]
        finally:
            c.close()
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert out[0] is not None and out[1] is not None
    ref = out[0][0]
    for res in out[0] + out[1]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(res, ref))


def test_dropin_over_minimal_types(tmp_path):
    """tests/cpp/test_fuse_dropin.cpp: the same map twice, once through orbfe::dropin::fuseMapPoints and once through the reference-shaped
    chain of the existing fuse bodies in the same target order; equal final maps (slots, observations, bad flags, fuse count), and both
    visibility counters non-zero on a scene where a replace changes a later target's visibility"""
    import subprocess
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sc = fs.scene(21, K=9, n=300, include_cur=True)
    t = sc["target_kfs"]                             # cur, then 8 targets: 4 first-order neighbours, the rest reached through them
    conn = {fs.CUR: t[1:5], t[1]: [fs.CUR, t[5], t[6]], t[2]: [t[6], t[7]], t[3]: [t[8], t[1]], t[4]: []}
    inp = tmp_path / "in.txt"
    fs.write_dropin_input(sc, str(inp), conn)
    pkg = os.path.join(ROOT, "orb_slam2_ros2_amd")
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), "-I" + os.path.join(pkg, "host"),
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_fuse_dropin.cpp"), "-L" + pkg,
                           "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    tag, n_fuse, flags, reeval, n_replaced, n_targets = r.stdout.split()
    assert tag == "OK" and int(n_targets) == 9
    assert int(n_fuse) > 50 and int(n_replaced) > 10 and int(flags) > 0 and int(reeval) > 0
