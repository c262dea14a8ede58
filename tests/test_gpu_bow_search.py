"""searchByBow over stored keyframes (orbfe_search_by_bow_stored) on the device against the CPU oracle
(bow_search_scenes.oracle: frontend.ORBMatcher.searchByBow with the numpy getBestMatch, per candidate).  Matches are integers: every
comparison is exact, element for element and in order."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_search_scenes as bs  # noqa: E402
import tri_scenes as ts  # noqa: E402
import triangulation_restatement as tr  # noqa: E402
from orb_slam2_ros2_amd._lib import Context, KeyframeStore, OrbfeError  # noqa: E402
from orb_slam2_ros2_amd.frontend import ORBMatcher  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_ID = 1 << 40            # ids are 64 bit: the query keyframe's does not fit 32


@pytest.fixture(scope="module")
def ctx():
    c = Context(640, 480, n_features=2000, n_levels=8, device_id=0, max_images=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small():
    """the K = 4, n = 300 scene in a store (the query stored too), and its oracle memo"""
    query, cands = bs.scene(0)
    st = KeyframeStore(ts.W, ts.H, 8)
    ids = bs.fill_store(st, cands)
    bs.fill_store(st, [query], Q_ID)
    memo = {}

    def oracle(mode, ratio, check):
        key = (mode, ratio, check)
        if key not in memo:
            memo[key] = [bs.oracle(query, kf, mode, ratio, check) for kf in cands]
        return memo[key]
    yield dict(query=query, cands=cands, st=st, ids=ids, oracle=oracle)
    st.close()


def run(ctx, st, query, ids, flags, mode, ratio, check, **kw):
    out = ctx.search_by_bow_stored(st, query, ids, flags, mode, ratio, 50, check, **kw)
    return [bs.as_tuples(a) for a in out], ctx.last_bow_offsets.copy()


# ---- 1. bit-exact on the small scene -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("mode", ["track", "loop", "add"])
def test_small_scene_equals_the_oracle(ctx, small, mode, check):
    q, st, ids = small["query"], small["st"], small["ids"]
    flags = [kf["flags"] for kf in small["cands"]]
    for ratio in (0.75, 0.7, 0.6):
        want = small["oracle"](bs.MODES[mode], ratio, check)
        host, off_h = run(ctx, st, bs.host_query(q), ids, flags, bs.MODES[mode], ratio, check)
        stored, off_s = run(ctx, st, dict(id=Q_ID, flags=q["flags"]), ids, flags, bs.MODES[mode], ratio, check)
        assert host == want and stored == want
        off = np.concatenate([[0], np.cumsum([len(w) for w in want])])
        assert np.array_equal(off_h, off) and np.array_equal(off_s, off) and off[-1] > 100
    # the matcher's own entry: ratio, threshold and the orientation switch from the instance
    m = ORBMatcher(0.7, check)
    assert m.searchByBowStored(ctx, st, bs.host_query(q), ids, flags, bAddMPs=mode == "add", bLoop=mode == "loop") == small["oracle"](bs.MODES[mode], 0.7, check)


# ---- 2. the hand-placed cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["track", "loop", "add"])
def test_hand_placed_cases(ctx, mode):
    q, c = bs.hand_scene()
    names = list(c)
    st = KeyframeStore(ts.W, ts.H, 8)
    ids = bs.fill_store(st, [c[k] for k in names], 100)
    flags = [c[k]["flags"] for k in names]
    for check in (True, False):
        want = [bs.oracle(q, c[k], bs.MODES[mode], 0.75, check) for k in names]
        got, _ = run(ctx, st, bs.host_query(q), ids, flags, bs.MODES[mode], 0.75, check)
        for k, g, w in zip(names, got, want):
            assert g == w, k
    st.close()


# ---- 3. one realistic shape ----------------------------------------------------------------------------------------------------------------
def test_twenty_candidates_of_two_thousand_features(ctx):
    query, cands = bs.scene(3, K=20, n=2000, n_pts=3000, skewed=False)
    st = KeyframeStore(ts.W, ts.H, 8)
    ids = bs.fill_store(st, cands)
    want = [bs.oracle(query, kf, bs.TRACK, 0.75, True) for kf in cands]
    got, off = run(ctx, st, bs.host_query(query), ids, [kf["flags"] for kf in cands], bs.TRACK, 0.75, True)
    assert got == want and off[-1] == sum(len(w) for w in want) and min(len(w) for w in want) > 200
    st.close()


# ---- 4. map state is an argument -----------------------------------------------------------------------------------------------------------
def test_map_state_is_an_argument_and_the_plain_path_agrees(ctx, small):
    q, cands, st, ids = small["query"], small["cands"], small["st"], small["ids"]
    rng = np.random.default_rng(9)
    other_q = dict(q, flags=rng.permutation(q["flags"]))
    other_c = [dict(kf, flags=np.where(rng.random(len(kf["flags"])) < 0.5, 3, 0).astype(np.uint8)) for kf in cands]
    m = ORBMatcher(0.75, True)
    res = []
    for qq, cc in ((q, cands), (other_q, other_c), (q, cands)):
        got, _ = run(ctx, st, bs.host_query(qq), ids, [kf["flags"] for kf in cc], bs.TRACK, 0.75, True)
        assert got == [bs.oracle(qq, kf, bs.TRACK, 0.75, True) for kf in cc]
        # the per-candidate path: ORBMatcher.searchByBow through orbfe_match_bruteforce
        plain = []
        for kf in cc:
            fq, fk = qq["flags"], kf["flags"]
            plain.append(m.searchByBow(ctx, desc_f=qq["desc"], desc_kf=kf["desc"], featvec_f=tr.featvec_dict(qq["fv"]), featvec_kf=tr.featvec_dict(kf["fv"]),
                                       good_f=(fq & 1) != 0, inmap_f=(fq & 2) != 0, good_kf=(fk & 1) != 0, inmap_kf=(fk & 2) != 0,
                                       angles_f=qq["kps"]["angle"], angles_kf=kf["kps"]["angle"]))
        assert got == plain
        res.append(got)
    assert res[0] == res[2] and res[0] != res[1]
    # NULL flags are all 0: in TRACK mode no keyframe feature has a good point, nothing matches; in LOOP mode the flags do not matter
    got, off = run(ctx, st, bs.host_query(q, with_flags=False), ids, None, bs.TRACK, 0.75, True)
    assert got == [[]] * 4 and not off.any()
    a, _ = run(ctx, st, bs.host_query(q, with_flags=False), ids, [None, cands[1]["flags"], None, None], bs.LOOP, 0.75, True)
    assert a == small["oracle"](bs.LOOP, 0.75, True)
    zero_q = dict(q, flags=np.zeros_like(q["flags"]))
    b, _ = run(ctx, st, bs.host_query(q, with_flags=False), ids, [kf["flags"] for kf in cands], bs.ADD, 0.75, True)
    assert b == [bs.oracle(zero_q, kf, bs.ADD, 0.75, True) for kf in cands]


# ---- 5. degenerate inputs ------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs(ctx, small):
    q, cands, st, ids = small["query"], small["cands"], small["st"], small["ids"]
    want = small["oracle"](bs.LOOP, 0.75, True)
    fl = [kf["flags"] for kf in cands]
    got, off = run(ctx, st, bs.host_query(q), ids[2:3], fl[2:3], bs.LOOP, 0.75, True)                       # K = 1
    assert got == want[2:3] and off.tolist() == [0, len(want[2])]
    got, _ = run(ctx, st, bs.host_query(q), [ids[1], ids[0], ids[1]], [fl[1], fl[0], fl[1]], bs.LOOP, 0.75, True)   # an id twice
    assert got == [want[1], want[0], want[1]]
    # the query's own id among the candidates (stored query): against itself every feature finds itself at distance 0
    got, _ = run(ctx, st, dict(id=Q_ID, flags=q["flags"]), [ids[0], Q_ID], [fl[0], q["flags"]], bs.LOOP, 0.75, True)
    me = bs.oracle(q, q, bs.LOOP, 0.75, True)
    assert got == [want[0], me] and len(me) > 200 and all(m[2] == 0 for m in me)
    # a keyframe with an empty FeatureVector (set_bow accepts one), and a keyframe without features
    st.add(900, cands[0]["kps"], cands[0]["desc"])
    st.set_bow(900, np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32))
    st.add(901, cands[0]["kps"][:0], cands[0]["desc"][:0])
    st.set_bow(901, np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32))
    got, off = run(ctx, st, bs.host_query(q), [900, ids[3], 901], [None, fl[3], None], bs.LOOP, 0.75, True)
    assert got == [[], want[3], []] and off.tolist() == [0, 0, len(want[3]), len(want[3])]
    got, off = run(ctx, st, bs.host_query(q), [900, 901], None, bs.LOOP, 0.75, True)                        # no slot at all
    assert got == [[], []] and off.tolist() == [0, 0, 0]
    empty_q = dict(desc=np.zeros((0, 32), np.uint8), fv=(np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32)),
                   angle=np.zeros(0, np.float32), flags=None)
    got, _ = run(ctx, st, empty_q, ids[:2], fl[:2], bs.LOOP, 0.75, True)                                   # a query without features
    assert got == [[], []]
    st.erase([900, 901])
    got, off = run(ctx, st, bs.host_query(q), [], [], bs.LOOP, 0.75, True)                                  # n_kf == 0
    assert got == [] and off.tolist() == [0]


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, small):
    q, cands, st, ids = small["query"], small["cands"], small["st"], small["ids"]
    fl = [kf["flags"] for kf in cands]
    hq = bs.host_query(q)
    st.add(950, cands[0]["kps"], cands[0]["desc"])                                                        # no FeatureVector
    nodes, offs, feats = q["fv"]
    unsorted = dict(hq, fv=(nodes[::-1].copy(), offs, feats))
    past = dict(hq, fv=(nodes, offs, np.where(np.arange(len(feats)) == 3, len(q["desc"]), feats).astype(np.uint32)))
    bad = [
        (hq, ids[:2] + [12345], fl[:2] + [None], bs.LOOP),                                                  # an unknown id
        (hq, ids[:2] + [950], fl[:2] + [None], bs.LOOP),                                                    # a keyframe without a FeatureVector
        (dict(id=950), ids, fl, bs.LOOP),                                                                   # ... as the query
        (dict(id=77777), ids, fl, bs.LOOP),                                                                 # an unknown query id
        (dict(id=Q_ID, flags=q["flags"][:-1]), ids, fl, bs.LOOP),                                           # n != the stored count
        (unsorted, ids, fl, bs.LOOP),                                                                       # unsorted query nodes
        (past, ids, fl, bs.LOOP),                                                                           # a feature index past n
        (hq, ids, fl, 3), (hq, ids, fl, -1),                                                                # a bad mode
        (hq, [ids[0]] * 65, [None] * 65, bs.LOOP),                                                          # n_kf = 65
    ]
    for query, kid, flags, mode in bad:
        with pytest.raises(OrbfeError) as ei:
            ctx.search_by_bow_stored(st, query, kid, flags, mode, 0.75, 50, True, cap=100000)
        assert ei.value.status == 1
        assert (ctx.last_bow_offsets == -1).all() and not ctx.last_bow_matches.view(np.int32).any()       # nothing written
    st.erase([950])
    with pytest.raises(OrbfeError) as ei:                                                                   # check_orientation without angles
        ctx.search_by_bow_stored(st, dict(hq, angle=None), ids, fl, bs.LOOP, 0.75, 50, True)
    assert ei.value.status == 1
    # cap one short of the total: ECAPACITY, the offsets set, matches untouched; with exactly enough room the call succeeds
    want = small["oracle"](bs.LOOP, 0.75, True)
    total = sum(len(w) for w in want)
    with pytest.raises(OrbfeError) as ei:
        ctx.search_by_bow_stored(st, hq, ids, fl, bs.LOOP, 0.75, 50, True, cap=total - 1)
    assert ei.value.status == 4
    assert ctx.last_bow_offsets.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert not ctx.last_bow_matches.view(np.int32).any()
    got, _ = run(ctx, st, hq, ids, fl, bs.LOOP, 0.75, True, cap=total)
    assert got == want
    with pytest.raises(OrbfeError) as ei:
        ctx.search_by_bow_stored(st, hq, ids, fl, bs.LOOP, 0.75, 50, True, cap=0)
    assert ei.value.status == 4 and ctx.last_bow_offsets[-1] == total


# ---- 7. drop-in ----------------------------------------------------------------------------------------------------------------------------
def build_dropin(tmp_path):
    pkg = os.path.join(ROOT, "orb_slam2_ros2_amd")
    exe = str(tmp_path / "tb")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "tests", "cpp", "stubs"), "-I" + os.path.join(pkg, "host"),
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_bowsearch_dropin.cpp"), "-L" + pkg,
                           "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    return exe


def write_dropin_input(path, query, cands):
    f = lambda v: repr(float(v))  # noqa: E731
    lines = [str(1 + len(cands))]
    for kf in [query] + cands:
        lines.append(str(len(kf["kps"])))
        for i, kp in enumerate(kf["kps"]):
            lines.append(f"{f(kp['x'])} {f(kp['y'])} {f(kp['angle'])} {int(kf['flags'][i])} " + " ".join(str(int(b)) for b in kf["desc"][i]))
        nodes, offs, feats = kf["fv"]
        lines.append(str(len(nodes)))
        for j, nd in enumerate(nodes):
            ids = feats[offs[j]:offs[j + 1]]
            lines.append(f"{int(nd)} {len(ids)} " + " ".join(str(int(v)) for v in ids))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def test_dropin_batched_search_equals_the_per_candidate_loop(tmp_path):
    """tests/cpp/test_bowsearch_dropin.cpp: the same small map through the per-candidate orbfe::dropin::searchByBow loop and through the
    overload over a store: equal match vectors, addMatchInTrack counts and final map points of the frame"""
    query, cands = bs.scene(5, K=5, n=300)
    inp = tmp_path / "in.txt"
    write_dropin_input(str(inp), query, cands)
    r = subprocess.run([build_dropin(tmp_path), str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    tag, n_track, n_loop, n_add, bumps = r.stdout.split()
    zero_q = dict(query, flags=np.zeros_like(query["flags"]))          # setMapPointsNull() before every candidate
    want = [sum(len(bs.oracle(q, kf, m, 0.75, True)) for kf in cands) for q, m in ((zero_q, bs.TRACK), (query, bs.LOOP), (query, bs.ADD))]
    assert tag == "OK" and [int(n_track), int(n_loop), int(n_add)] == want and min(want) > 100
    assert int(bumps) == want[0]          # every tracking match is on a good keyframe point: one addMatchInTrack each
