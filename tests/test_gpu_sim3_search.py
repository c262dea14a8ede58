"""searchBySim3 over stored keyframes (orbfe_search_by_sim3_stored, orbfe_search_by_sim3_points_stored) on the device against
the CPU restatement (sim3_search_restatement.py: matcher_ext's arithmetic, the oracle's findFeaturesInArea + getBestMatch).  Indices and
Hamming distances are integers: every comparison is exact, element for element.  640 x 480, 8 levels throughout."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_search_restatement as rs  # noqa: E402
import sim3_search_scenes as sc  # noqa: E402
from orb_slam2_ros2_amd._lib import Context, KeyframeStore, OrbfeError  # noqa: E402
from orb_slam2_ros2_amd.frontend import ORBMatcher  # noqa: E402

pytestmark = pytest.mark.gpu
C_ID, M_ID = 7, (1 << 40) + 3          # ids are 64 bit


@pytest.fixture(scope="module")
def ctx():
    c = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
    yield c
    c.close()


class Stored:
    """a scene's two keyframes in a store of their own"""

    def __init__(self, scene):
        self.scene, self.st = scene, KeyframeStore(sc.W, sc.H, 8)
        sc.add_to_store(self.st, scene["C"], C_ID), sc.add_to_store(self.st, scene["M"], M_ID)

    def pair(self, ctx, ratio, th=None, matches=None, C=None, M=None, **kw):
        S = self.scene
        return ctx.search_by_sim3_stored(self.st, sc.side(C or S["C"], C_ID), sc.side(M or S["M"], M_ID), S["Scm"][1:], S["Scm"][0],
                                         S["matches"] if matches is None else matches, sc.CAM, sc.SF, th or S["th"], ratio, 50, **kw)

    def points(self, ctx, ratio, th=None, loop=None):
        S = self.scene
        kid = M_ID if S.get("loop_target") == "M" else C_ID
        return ctx.search_by_sim3_points_stored(self.st, kid, loop or S["loop"], S["Scw"][1:], S["Scw"][0], sc.CAM, sc.SF, th or S["th"], ratio, 50)

    def want_pair(self, orc, ratio, th=None, matches=None, C=None, M=None):
        S = self.scene
        return rs.pair(orc, C or S["C"], M or S["M"], S["Scm"], S["matches"] if matches is None else matches, sc.CAM, sc.SF, th or S["th"], ratio)

    def want_points(self, orc, ratio, th=None, loop=None):
        S = self.scene
        return rs.points(orc, S[S.get("loop_target", "C")], loop or S["loop"], S["Scw"], sc.CAM, sc.SF, th or S["th"], ratio)

    def check(self, ctx, orc, ratio, th=None):
        """both calls against the restatement; returns the two restatements"""
        w = self.want_pair(orc, ratio, th)
        assert self.pair(ctx, ratio, th) == w["new"]
        p = self.want_points(orc, ratio, th)
        bi, bd = self.points(ctx, ratio, th)
        assert np.array_equal(bi, p[0]) and np.array_equal(bd, p[1])
        return w, p

    def close(self):
        self.st.close()


@pytest.fixture(scope="module")
def small(ctx):
    s = Stored(sc.seeded(0, 1.0))
    yield s
    s.close()


# ---- 1. seeded scenes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1.0, 0.5, 2.0])
def test_seeded_scene_equals_the_restatement(ctx, orc, s):
    S = Stored(sc.seeded(1, s))
    for ratio in (0.75, 0.9):
        w, p = S.check(ctx, orc, ratio)
        assert (w["a"] >= 0).sum() >= 20 and (w["b"] >= 0).sum() >= 20 and (p[0] >= 0).sum() >= 20
    # the matcher's own entries: what searchBySim3Frames / searchBySim3MapPoints return
    sn = S.scene
    m = ORBMatcher(0.75)
    got = m.searchBySim3Stored(ctx, S.st, sn["matches"], sn["Scm"], (sn["C"]["Rcw"], sn["C"]["tcw"]), (sn["M"]["Rcw"], sn["M"]["tcw"]), C_ID, M_ID,
                               sc.frames_kf(sn["C"]), sc.frames_kf(sn["M"]), 7.5, sc.CAM, sc.SF)
    assert got == list(sn["matches"]) + S.want_pair(orc, 0.75)["new"]
    matched = np.full(len(sn["C"]["kps"]), -1, np.int64)
    matched[[2, 11]] = sn["loop"]["id"][[5, 9]]
    loop = dict(sn["loop"], usable=sn["loop"]["usable"] & ~np.isin(sn["loop"]["id"], matched))
    bi = S.want_points(orc, 0.75, 10.0, loop)[0]
    got, n = m.searchBySim3PointsStored(ctx, S.st, C_ID, sn["loop"], matched, sn["Scw"], 10.0, sc.CAM, sc.SF)
    assert got == [(int(bi[j]), int(j)) for j in np.flatnonzero(bi >= 0)] and n == 2 + len(got) and len(got) > 20
    S.close()


def test_hand_placed_scene_equals_the_restatement(ctx, orc):
    S = Stored(sc.hand())
    w, p = S.check(ctx, orc, 0.75)
    n = S.scene["notes"]
    assert w["reasons_b"][n["B"]["between_bounds"]] == "accepted" and w["reasons_a"][n["A"]["between_bounds"]] == "u_max"
    S.close()


# ---- 2. hand-placed windows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 127, 128, 129])
def test_candidate_counts_at_the_fold_boundaries(ctx, orc, n_cand):
    S = Stored(sc.window(n_cand))
    w, p = S.check(ctx, orc, 1.0)
    assert w["cand_a"][0] == n_cand and p[4][0] > n_cand and w["a"][0] >= 0 and p[0][0] >= 0
    S.close()


@pytest.mark.parametrize("where", [(5, 9), (10, 70), (63, 64), (0, 128)])
def test_first_minimum_tied_inside_a_chunk_and_across_chunks(ctx, orc, where):
    dists = np.full(130, 30)
    dists[list(where)] = 4
    S = Stored(sc.window(130, dists=dists, n_decoys=20))
    w, _ = S.check(ctx, orc, 1.0)
    first = np.flatnonzero((S.scene["M"]["flags"] == 3) & (S.scene["M"]["kps"]["octave"] <= 2))[where[0]]
    assert w["cand_a"][0] == 130 and w["new"] == [(0, int(first))]
    assert S.pair(ctx, 0.99) == []                         # best / second = 1
    S.close()


@pytest.mark.parametrize("at", [(3.0, 200.0), (637.0, 200.0), (300.0, 2.5), (300.0, 477.5), (2.0, 478.0)])
def test_window_clipped_at_an_image_edge(ctx, orc, at):
    S = Stored(sc.window(20, at=at))
    w, p = S.check(ctx, orc, 1.0)
    assert w["cand_a"][0] == 20 and w["a"][0] >= 0
    S.close()


def test_window_over_the_whole_grid(ctx, orc, small):
    w, p = small.check(ctx, orc, 0.9, th=2000.0)
    n_low = int(((small.scene["M"]["flags"] == 3) & (small.scene["M"]["kps"]["octave"] <= 2)).sum())
    assert w["cand_a"].max() == n_low > 128 and p[4].max() == len(small.scene["C"]["kps"])


@pytest.mark.parametrize("bounds", [(sc.WIDE, sc.WIDE), ((-30.0, 700.0, -20.0, 520.0), sc.IMAGE), (sc.IMAGE, (4.0, 630.5, 6.0, 470.25))])
def test_bounds_that_are_not_the_image_and_differ_between_the_keyframes(ctx, orc, bounds):
    scene = sc.seeded(2, 1.0, bounds_c=bounds[0], bounds_m=bounds[1])
    rng = np.random.default_rng(3)
    for kf, b in ((scene["C"], bounds[0]), (scene["M"], bounds[1])):   # features up to the bounds, outside the image where they allow it
        k = rng.permutation(len(kf["kps"]))[:30]
        kf["kps"]["x"][k] = rng.uniform(b[0] + 0.5, b[1] - 0.5, 30).astype(np.float32)
        kf["kps"]["y"][k] = rng.uniform(b[2] + 0.5, b[3] - 0.5, 30).astype(np.float32)
    S = Stored(scene)
    w, p = S.check(ctx, orc, 0.8)
    assert len(w["new"]) > 30
    S.close()


# ---- 3. degenerate inputs ------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs(ctx, orc, small):
    S, st = small.scene, small.st
    C, M = S["C"], S["M"]
    want = small.want_pair(orc, 0.75)
    empty = dict(kps=C["kps"][:0], desc=C["desc"][:0], bounds=None)
    one = dict(kps=M["kps"][:1], desc=M["desc"][:1])
    st.add(900, empty["kps"], empty["desc"])
    st.add(901, one["kps"], one["desc"], bounds=M["bounds"])
    cut = lambda kf, k, i: dict(sc.side(kf, i), flags=kf["flags"][:k], pos=kf["pos"][:k], max_dist=kf["max_dist"][:k], min_dist=kf["min_dist"][:k])  # noqa: E731
    run = lambda a, b, matches=(), **kw: ctx.search_by_sim3_stored(st, a, b, S["Scm"][1:], S["Scm"][0], list(matches), sc.CAM, sc.SF, 7.5, 0.75, 50, **kw)  # noqa: E731
    assert run(cut(C, 0, 900), sc.side(M, M_ID)) == [] and run(sc.side(C, C_ID), cut(M, 0, 900)) == []           # n = 0 on either side
    assert run(cut(C, 0, 900), cut(M, 0, 900)) == []
    # n = 1: M's first feature alone, as target and as source
    M1 = dict(M, kps=M["kps"][:1], desc=M["desc"][:1], flags=np.array([3], np.uint8), pos=M["pos"][:1], max_dist=M["max_dist"][:1], min_dist=M["min_dist"][:1])
    assert run(sc.side(C, C_ID), cut(M1, 1, 901)) == rs.pair(orc, C, M1, S["Scm"], [], sc.CAM, sc.SF, 7.5, 0.75)["new"]
    assert run(cut(M1, 1, 901), sc.side(C, C_ID)) == rs.pair(orc, M1, C, S["Scm"], [], sc.CAM, sc.SF, 7.5, 0.75)["new"]
    # m = 0
    none = {k: v[:0] for k, v in S["loop"].items()}
    bi, bd = ctx.search_by_sim3_points_stored(st, C_ID, none, S["Scw"][1:], S["Scw"][0], sc.CAM, sc.SF, 10.0, 0.75, 50)
    assert len(bi) == 0 and len(bd) == 0
    # all flags 0, flags NULL (on one side: nothing of it is a source and nothing of it is a target)
    zero = lambda kf, i: dict(sc.side(kf, i), flags=np.zeros_like(kf["flags"]))  # noqa: E731
    null = lambda kf, i: dict(id=i, n=len(kf["kps"]), flags=None, Rcw=kf["Rcw"], tcw=kf["tcw"])  # noqa: E731
    assert run(zero(C, C_ID), zero(M, M_ID)) == [] and run(null(C, C_ID), null(M, M_ID)) == []
    assert run(null(C, C_ID), sc.side(M, M_ID), S["matches"]) == [] and run(sc.side(C, C_ID), zero(M, M_ID), S["matches"]) == []
    # every feature named by an input match
    all_named = [(i, i) for i in range(min(len(C["kps"]), len(M["kps"])))]
    assert len(C["kps"]) == len(M["kps"]) and run(sc.side(C, C_ID), sc.side(M, M_ID), all_named) == []
    # cur->id == match->id with the identity similarity and one pose: every good point in range finds its own feature, or a twin
    ident = (np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    me = ctx.search_by_sim3_stored(st, sc.side(C, C_ID), sc.side(C, C_ID), ident, 1.0, [], sc.CAM, sc.SF, 7.5, 0.75, 50)
    w = rs.pair(orc, C, C, (1.0, ident[0], ident[1]), [], sc.CAM, sc.SF, 7.5, 0.75)
    assert me == w["new"] and len(me) > 100 and sum(q == t for q, t in me) > 100
    # cap = 0 with results pending: ECAPACITY, *n_new right, nothing written; exactly enough room succeeds
    with pytest.raises(OrbfeError) as ei:
        small.pair(ctx, 0.75, cap=0)
    assert ei.value.status == 4 and ctx.last_sim3_new == len(want["new"]) > 0 and not ctx.last_sim3_out.view(np.int32).any()
    with pytest.raises(OrbfeError) as ei:
        small.pair(ctx, 0.75, cap=len(want["new"]) - 1)
    assert ei.value.status == 4 and not ctx.last_sim3_out.view(np.int32).any()
    assert small.pair(ctx, 0.75, cap=len(want["new"])) == want["new"]
    st.erase([900, 901])


# ---- 4. map state is an argument -----------------------------------------------------------------------------------------------------------
def test_map_state_is_an_argument_and_the_plain_path_agrees(ctx, orc):
    S = Stored(sc.seeded(4, 1.0, bounds_c=sc.IMAGE, bounds_m=sc.IMAGE))
    sn = S.scene
    rng = np.random.default_rng(8)
    other = {}
    for k in ("C", "M"):
        kf = sn[k]
        p = rng.permutation(len(kf["kps"]))
        other[k] = dict(kf, flags=rng.permutation(kf["flags"]), pos=np.where(rng.random((len(p), 1)) < 0.3, kf["pos"][p], kf["pos"]).astype(np.float32))
    m = ORBMatcher(0.75)
    res = []
    for C, M in ((sn["C"], sn["M"]), (other["C"], other["M"]), (sn["C"], sn["M"])):
        got = S.pair(ctx, 0.75, C=C, M=M)
        assert got == S.want_pair(orc, 0.75, C=C, M=M)["new"]
        # the path it replaces: both keyframes uploaded, two searches (both keyframes have the image as bounds here)
        plain = m.searchBySim3Frames(ctx, sn["matches"], sn["Scm"], (C["Rcw"], C["tcw"]), (M["Rcw"], M["tcw"]), sc.frames_kf(C), sc.frames_kf(M), 7.5,
                                     sc.CAM, sc.IMAGE, sc.SF)
        assert plain == list(sn["matches"]) + got
        res.append(got)
    assert res[0] == res[2] and res[0] != res[1] and len(res[1]) > 10
    S.close()


# ---- 5. one full-size case -----------------------------------------------------------------------------------------------------------------
def test_two_thousand_features_and_four_thousand_loop_points(ctx, orc):
    S = Stored(sc.seeded(6, 1.0, n=2000, n_pts=2600, m_loop=4000))
    assert len(S.scene["C"]["kps"]) == 2000 and len(S.scene["loop"]["usable"]) == 4000
    w, p = S.check(ctx, orc, 0.75)
    assert len(w["new"]) > 300 and (p[0] >= 0).sum() > 500
    S.close()


def test_a_loop_group_too_large_for_the_staging_buffer(ctx, orc, small):
    """past 8 MB of upload the arrays are copied directly instead of through the page-locked buffer: the small scene's loop group 400
    times over (160000 points, 9 MB) must give the small group's answer 400 times over, and that answer is the restatement's"""
    S = small.scene
    bi, bd = small.points(ctx, 0.75, 10.0)
    w = small.want_points(orc, 0.75, 10.0)
    assert np.array_equal(bi, w[0]) and np.array_equal(bd, w[1]) and (bi >= 0).sum() > 100
    big = {k: np.concatenate([v] * 400) for k, v in S["loop"].items()}
    assert len(big["usable"]) * 57 > (8 << 20)
    bi2, bd2 = small.points(ctx, 0.75, 10.0, loop=big)
    assert np.array_equal(bi2, np.tile(bi, 400)) and np.array_equal(bd2, np.tile(bd, 400))
    assert np.array_equal(small.points(ctx, 0.75, 10.0)[0], bi)                 # and the staged path still answers afterwards


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, orc, small):
    S, st = small.scene, small.st
    C, M = sc.side(S["C"], C_ID), sc.side(S["M"], M_ID)
    R, t, s = S["Scm"][1], S["Scm"][2], S["Scm"][0]
    nan_R = R.copy()
    nan_R[1, 2] = np.nan
    short = dict(C, flags=C["flags"][:-1], pos=C["pos"][:-1], max_dist=C["max_dist"][:-1], min_dist=C["min_dist"][:-1])
    n_c, n_m = len(S["C"]["kps"]), len(S["M"]["kps"])
    bad = [
        dict(cur=dict(C, id=12345)), dict(match=dict(M, id=12345)),                                   # an unknown id
        dict(cur=short),                                                                              # n unequal to the stored count
        dict(matches=[(0, 0), (n_c, 0)]), dict(matches=[(0, n_m)]), dict(matches=[(-1, 0)]),          # a match index out of range
        dict(s=np.nan), dict(s=np.inf), dict(s=0.0), dict(s=-1.0),                                    # the scale
        dict(model=(nan_R, t)), dict(model=(R, np.array([0, np.inf, 0], np.float32))),                # a model entry
        dict(sf=sc.SF[:7]),                                                                           # n_levels below the store's
    ]
    for kw in bad:
        with pytest.raises(OrbfeError) as ei:
            ctx.search_by_sim3_stored(st, kw.get("cur", C), kw.get("match", M), kw.get("model", (R, t)), kw.get("s", s), kw.get("matches", S["matches"]),
                                      sc.CAM, kw.get("sf", sc.SF), 7.5, 0.75, 50)
        assert ei.value.status == 1, kw
        assert ctx.last_sim3_new == -1 and not ctx.last_sim3_out.view(np.int32).any()                # nothing written
    loop = S["loop"]
    for kw in (dict(kid=12345), dict(s=np.nan), dict(s=0.0), dict(model=(nan_R, t)), dict(sf=sc.SF[:7])):
        with pytest.raises(OrbfeError) as ei:
            ctx.search_by_sim3_points_stored(st, kw.get("kid", C_ID), loop, kw.get("model", S["Scw"][1:]), kw.get("s", S["Scw"][0]), sc.CAM,
                                             kw.get("sf", sc.SF), 10.0, 0.75, 50)
        assert ei.value.status == 1, kw
    # NULL arrays with a non-zero count, through the C call itself
    from orb_slam2_ros2_amd import _lib
    import ctypes
    keep = []
    c_side, m_side = ctx._sim3_side(C, keep), ctx._sim3_side(M, keep)
    c_side.pos = None
    mdl, sv = ctx._sim3_model((R, t), s)
    cam = _lib.Camera(*[float(v) for v in sc.CAM], 0.0)
    sf = np.ascontiguousarray(sc.SF, np.float32)
    out, n_new = np.zeros(n_c, _lib.BOW_MATCH_DTYPE), ctypes.c_int32(-1)
    call = lambda cs, nm, mt, o: ctx.lib.orbfe_search_by_sim3_stored(ctx.h, st.h, ctypes.byref(cs), ctypes.byref(m_side), _lib.ptr(mdl), sv, nm, mt,  # noqa: E731
                                                                     ctypes.byref(cam), _lib.ptr(sf), 8, 7.5, 0.75, 50, o, n_c, ctypes.byref(n_new))
    assert call(c_side, 0, None, _lib.ptr(out)) == 1
    c_side = ctx._sim3_side(C, keep)
    assert call(c_side, 3, None, _lib.ptr(out)) == 1 and call(c_side, 0, None, None) == 1 and n_new.value == -1 and not out.view(np.int32).any()
    pts = _lib.Sim3Points(len(loop["usable"]), None, None, None, None, None, None)
    bi = np.full(len(loop["usable"]), -7, np.int32)
    assert ctx.lib.orbfe_search_by_sim3_points_stored(ctx.h, st.h, C_ID, ctypes.byref(pts), _lib.ptr(mdl), sv, ctypes.byref(cam), _lib.ptr(sf), 8, 10.0,
                                                      0.75, 50, _lib.ptr(bi), _lib.ptr(bi)) == 1 and (bi == -7).all()
    # a context on another device (where the machine has one)
    import torch
    if torch.cuda.device_count() > 1:
        far = Context(640, 480, n_features=2000, n_levels=8, device_id=1, max_images=1)
        with pytest.raises(OrbfeError) as ei:
            far.search_by_sim3_stored(st, C, M, (R, t), s, S["matches"], sc.CAM, sc.SF, 7.5, 0.75, 50)
        assert ei.value.status == 1
        with pytest.raises(OrbfeError) as ei:
            far.search_by_sim3_points_stored(st, C_ID, loop, S["Scw"][1:], S["Scw"][0], sc.CAM, sc.SF, 10.0, 0.75, 50)
        assert ei.value.status == 1
        far.close()
    # afterwards the same context and store still answer
    small.check(ctx, orc, 0.75)


# ---- 7. drop-in ----------------------------------------------------------------------------------------------------------------------------
def build_dropin(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "orb_slam2_ros2_amd")
    exe = str(tmp_path / "ts")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(root, "tests", "cpp", "stubs"), "-I" + os.path.join(pkg, "host"),
                           "-I" + os.path.join(root, "include"), "-o", exe, os.path.join(root, "tests", "cpp", "test_sim3search_dropin.cpp"), "-L" + pkg,
                           "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    return exe


def write_dropin_input(path, S, th_points, ratio):
    f = lambda v: repr(float(v))  # noqa: E731
    row = lambda a: " ".join(f(v) for v in np.asarray(a).reshape(-1))  # noqa: E731
    lines = [row(S["cam"]), f"{len(sc.SF)} " + row(sc.SF), f"{f(S['th'])} {f(th_points)} {f(ratio)}"]
    for sim in (S["Scm"], S["Scw"]):
        lines.append(f"{f(sim[0])} {row(sim[1])} {row(sim[2])}")
    lines.append(f"{len(S['matches'])} " + " ".join(f"{q} {t}" for q, t in S["matches"]))
    for kf in (S["C"], S["M"]):
        lines.append(f"{row(kf['Rcw'])} {row(kf['tcw'])}")
        lines.append(str(len(kf["kps"])))
        for i, kp in enumerate(kf["kps"]):
            lines.append(f"{f(kp['x'])} {f(kp['y'])} {int(kp['octave'])} {int(kf['flags'][i])} {row(kf['pos'][i])} {f(kf['max_dist'][i])} "
                         f"{f(kf['min_dist'][i])} " + " ".join(str(int(b)) for b in kf["desc"][i]))
    L = S["loop"]
    lines.append(str(len(L["usable"])))
    for j in range(len(L["usable"])):
        lines.append(f"{int(L['usable'][j])} {row(L['pos'][j])} {row(L['view_dir'][j])} {f(L['max_dist'][j])} {f(L['min_dist'][j])} " +
                     " ".join(str(int(b)) for b in L["desc"][j]))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def test_dropin_stored_overloads_equal_the_plain_ones(tmp_path, orc):
    """tests/cpp/test_sim3search_dropin.cpp: one small map on stand-in classes through both searchBySim3 overloads with and without the
    store: equal match vectors, vMatchedMps and return values; the counts are the restatement's"""
    import subprocess
    S = sc.quarter(sc.seeded(5, 1.25, n=150, n_pts=220, m_loop=200))
    inp = tmp_path / "in.txt"
    write_dropin_input(str(inp), S, 10.0, 0.75)
    r = subprocess.run([build_dropin(tmp_path), str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    tag, n_all, n_new, n_matches, filled = r.stdout.split()
    w = rs.pair(orc, S["C"], S["M"], S["Scm"], S["matches"], S["cam"], sc.SF, S["th"], 0.75)
    assert tag == "OK" and int(n_new) == len(w["new"]) > 20 and int(n_all) == len(S["matches"]) + len(w["new"])
    first = np.flatnonzero(S["loop"]["usable"])[:2]
    usable = S["loop"]["usable"].copy()
    usable[first] = False                                              # already in vMatchedMps (slots 3 and 7)
    bi = rs.points(orc, S["C"], dict(S["loop"], usable=usable), S["Scw"], S["cam"], sc.SF, 10.0, 0.75)[0]
    slots = {3: int(first[0]), 7: int(first[1])}
    for j in np.flatnonzero(bi >= 0):
        slots[int(bi[j])] = int(j)
    assert int(n_matches) == 2 + int((bi >= 0).sum()) > 22 and int(filled) == len(slots)
