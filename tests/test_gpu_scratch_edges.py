"""The scratch layouts of the host entry points (csrc/scratch_layout.h) at the sizes where a layout can go wrong: array sizes one below,
on and one above a 256-byte boundary for byte, 4-byte and 8-byte fields, empty arrays, and the two unstaged branches.  Every call is
checked against the oracle or restatement its neighbouring test uses, with that test's tolerance; the calls run back to back on ONE
context, so an array that overran its place in the shared scratch would corrupt the next call's inputs or results."""
import numpy as np
import pytest

import bow_restatement as R
from orb_slam2_ros2_amd import ba_synth, synth_vocab
from orb_slam2_ros2_amd._lib import KP_DTYPE, Context, Vocabulary
from test_guided_wrappers import _vision_case
from test_local_ba import _pose_dist
from test_pose_only import _args as _pose_args

pytestmark = pytest.mark.gpu
W, H = 640, 480
SIZES = (1, 7, 8, 9, 63, 64, 65, 255, 256, 257)
INT_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(W, H, n_features=500, max_images=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def voc(tmp_path_factory):
    v = synth_vocab.edge(1, 4, 5)
    p = tmp_path_factory.mktemp("voc") / "edge.txt"
    synth_vocab.write_txt(p, v)
    return v, Vocabulary.load_txt(str(p))


# ---- one case per entry point and size: run(ctx) -> result, check(result) against the oracle ----------------------------------------
def _bruteforce(orc, nq, nt, lists):
    """lists: None (every target), "random" (a list per query, some empty), "empty" (offsets all zero, no entries)"""
    r = np.random.default_rng(1000 * nq + nt)
    t = r.integers(0, 256, (nt, 32), dtype=np.uint8)
    q = t[r.integers(0, nt, nq)] ^ (r.integers(0, 256, (nq, 32), dtype=np.uint8) & r.integers(0, 2, (nq, 32), dtype=np.uint8) * 3)
    if lists is None:
        offs = cand = None
    else:
        lens = r.integers(0, nt + 1, nq) if lists == "random" else np.zeros(nq, np.int64)
        if lists == "random":
            lens[0] = 0
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        cand = np.concatenate([r.permutation(nt)[:n] for n in lens] + [np.zeros(0, np.int64)]).astype(np.uint32)

    def check(got):
        bi, bd, sd = got
        if lists is None:
            assert all(np.array_equal(a, b) for a, b in zip(got, orc.match_bruteforce(q, t)))
            return
        for i in range(nq):
            c = cand[offs[i]:offs[i + 1]].astype(np.int64)
            want = (-1, INT_MAX, INT_MAX) if len(c) == 0 else orc.best_match(q[i], t, c)[:3]
            assert (bi[i], bd[i], sd[i]) == want, (nq, nt, lists, i)

    return (lambda c: c.match_bruteforce(q, t, offs, cand)), check


def _search(orc, nq, nt, hits):
    r = np.random.default_rng(77 * nq + nt)
    kps = np.zeros(nt, KP_DTYPE)
    kps["x"], kps["y"], kps["octave"] = r.uniform(0, W, nt), r.uniform(0, H, nt), r.integers(0, 8, nt)
    desc = r.integers(0, 256, (nt, 32), dtype=np.uint8)
    pick = r.integers(0, nt, nq)
    qxy = (np.stack([kps["x"][pick], kps["y"][pick]], 1) + r.normal(0, 3, (nq, 2))).astype(np.float32)
    rad = r.uniform(2, 80, nq).astype(np.float32)
    lo, hi = r.integers(-1, 4, nq).astype(np.int8), r.integers(3, 9, nq).astype(np.int8)
    qd = desc[pick] ^ (r.integers(0, 256, (nq, 32), dtype=np.uint8) & r.integers(0, 2, (nq, 32), dtype=np.uint8))
    ex = (r.random(nt) < 0.3).astype(np.uint8) if hits else None

    def check(got):
        want = orc.search_in_area_ex(kps, desc, (0.0, float(W), 0.0, float(H)), qxy, rad, lo, hi, qd, ex) if hits else \
            orc.search_in_area(kps, desc, W, H, qxy, rad, lo, hi, qd, None)
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), (nq, nt, hits)

    return (lambda c: c.search_in_area_features(kps, desc, qxy, rad, lo, hi, qd, ex, want_hits=hits)), check


def _pose_only(orc, n):
    p = ba_synth.make_pose_problem(seed=3 + n, n=max(n, 1))
    a = _pose_args(p)
    if n == 0:
        for k in ("Xw", "meas", "info", "sigma2"):
            a[k] = a[k][:0]

    def check(g):
        o = orc.pose_only_optimize(**a)
        assert np.abs(g[1] - o[1]).max() < 1e-6 and abs(g[0] - o[0]) <= 1 and (g[2] != o[2]).sum() <= 1

    return (lambda c: c.pose_only_optimize(**a)), check


def _project(orc, n):
    args = _vision_case(n, 40 + n)

    def check(got):
        want = orc.project_map_points(*args)
        assert (got["visible"] == want["visible"]).all()
        k = want["visible"].astype(bool)
        for key in ("uv", "distance", "cos_theta", "level"):
            assert (got[key][k] == want[key][k]).all(), key

    return (lambda c: c.project_map_points(*args)), check


def _small_ba(n_kf, n_pt, n_e):
    """a problem of exactly n_kf poses, n_pt points and n_e edges out of ba_synth.make_problem's: the first n_kf poses, the n_pt points
    they see most often (renumbered), n_e of the edges between them"""
    p = ba_synth.make_problem(seed=5, n_kf=3, n_pt=32)
    per_edge = ("edge_pose", "edge_point", "meas", "is_stereo", "info", "huber_delta")
    seen = np.bincount(p["edge_point"][p["edge_pose"] < n_kf], minlength=32)
    pts = np.sort(np.argsort(-seen, kind="stable")[:n_pt])
    ok = np.flatnonzero((p["edge_pose"] < n_kf) & np.isin(p["edge_point"], pts))
    assert len(ok) >= n_e, (n_kf, n_pt, n_e, len(ok))
    e = ok[np.linspace(0, len(ok) - 1, n_e).astype(int)]
    out = {k: (v[e] if k in per_edge else v) for k, v in p.items()}
    out["edge_point"] = np.searchsorted(pts, out["edge_point"]).astype(np.int32)
    out["poses"], out["points"] = p["poses"][:n_kf], p["points"][pts]
    return out


def _eval_edges(orc, p, jac):
    def check(out):
        ref = orc.ba_eval_edges(**p)
        for k in ("error", "chi2", "rho") + (("j_point", "j_pose") if jac else ()):
            assert out[k].shape == ref[k].shape and np.allclose(out[k], ref[k], rtol=1e-9, atol=1e-12), k
        assert np.array_equal(out["depth_positive"], ref["depth_positive"]) and ("j_pose" in out) == jac

    return (lambda c: c.ba_eval_edges(**p, jacobians=jac)), check


def _build_system(orc, p, hpl):
    fixed = np.zeros(len(p["poses"]), np.uint8)
    fixed[0] = len(fixed) > 1

    def check(out):
        ref = orc.ba_build_system(**p, pose_fixed=fixed)
        for k in ("Hpp", "bp", "Hll", "bl") + (("Hpl",) if hpl else ()):
            assert np.allclose(out[k], ref[k], rtol=1e-9, atol=1e-12 * np.abs(ref[k]).max()), k
        assert ("Hpl" in out) == hpl

    return (lambda c: c.ba_build_system(**p, pose_fixed=fixed, want_hpl=hpl)), check


def _local_ba(orc):
    """2 poses (1 fixed), 4 points, 8 edges"""
    pr, fixed = _small_ba(2, 4, 8), np.array([1, 0], np.uint8)

    def check(g):
        o = orc.ba_local_optimize(pr, fixed)
        assert tuple(g["iters"]) == tuple(o["iters"])
        assert _pose_dist(g["poses"], o["poses"]) < 1e-7 and np.abs(g["points"] - o["points"]).max() < 1e-7
        assert np.array_equal(g["poses"][:1], pr["poses"][:1])
        assert (g["level"] != o["level"]).sum() <= 1 and (g["bad"] != o["bad"]).sum() <= 1

    return (lambda c: c.ba_local_optimize(pr, fixed)), check


def _bow(voc, n):
    v, dev = voc
    d = np.random.default_rng(n).integers(0, 256, (n, 32), dtype=np.uint8)
    return (lambda c: c.bow_transform(dev, d, 2)), (lambda got: R.assert_same(got, R.transform(v, d, 2), f"n {n}"))


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def _run_back_to_back(ctx, cases):
    """every case on the one context, each checked; then the first again: bit-identical to its first run"""
    first = None
    for run, check in cases:
        got = run(ctx)
        check(got)
        first = got if first is None else first
    assert _same(cases[0][0](ctx), first)


def test_alignment_and_empty_array_sizes_back_to_back(orc, ctx, voc):
    cases = []
    for i, nq in enumerate(SIZES):   # every nq and every nt, the two boundary triples crossed in full
        for nt in {SIZES[(i + 3) % len(SIZES)], nq} | ({7, 8, 9, 255, 256, 257} if nq in (63, 64, 65, 255, 256, 257) else set()):
            cases.append(_bruteforce(orc, nq, nt, None))
        cases.append(_bruteforce(orc, nq, SIZES[(i + 5) % len(SIZES)], "random"))
    cases.append(_bruteforce(orc, 9, 65, "empty"))
    for nq in SIZES:
        for nt in (1, 256, 257):
            cases.append(_search(orc, nq, nt, False))
            cases.append(_pose_only(orc, (0, 1, 255, 256, 257)[(nq + nt) % 5]))   # a neighbour whose scratch is laid out differently
    cases.append(_search(orc, 65, 257, True))
    for n in (1, 64, 65):
        cases.append(_project(orc, n))
    for shape in ((1, 1, 1), (2, 3, 5), (3, 32, 33)):
        p = _small_ba(*shape)
        for flag in (True, False):
            cases.append(_eval_edges(orc, p, flag))
            cases.append(_build_system(orc, p, flag))
    cases.append(_local_ba(orc))   # (the context's default: the device-side Levenberg-Marquardt path)
    for n in (0, 1, 8, 9):
        cases.append(_bow(voc, n))
        cases.append(_bruteforce(orc, 8, 9, "random"))
    _run_back_to_back(ctx, cases)


def test_local_ba_host_driven_path_back_to_back(orc, monkeypatch):
    """the same small problem down the host-driven optimiser (the switch is read at orbfe_create), between two other calls"""
    monkeypatch.setenv("ORBFE_LBA_HOST_LM", "1")
    c = Context(W, H, n_features=500, max_images=1)
    try:
        _run_back_to_back(c, [_bruteforce(orc, 65, 257, "random"), _local_ba(orc), _pose_only(orc, 257), _local_ba(orc),
                              _build_system(orc, _small_ba(2, 3, 5), True)])
    finally:
        c.close()


def test_bruteforce_unstaged_branch_equals_staged_pieces(ctx):
    """more than 8 MB of scratch (70 000 x 32 + 200 000 x 32 bytes of descriptors): the inputs and results are copied directly, not through
    the staging buffer.  One candidate per query keeps the kernel's work trivial.  Against the same queries in two staged halves."""
    r = np.random.default_rng(8)
    nq, nt = 70_000, 200_000
    t = r.integers(0, 256, (nt, 32), dtype=np.uint8)
    cand = r.integers(0, nt, nq).astype(np.uint32)
    q = t[cand] ^ (r.integers(0, 256, (nq, 32), dtype=np.uint8) & np.uint8(1))
    offs = np.arange(nq + 1, dtype=np.uint32)
    whole = ctx.match_bruteforce(q, t, offs, cand)
    h = nq // 2
    assert h * 32 + nt * 32 + (h + 1) * 4 + h * 4 * 4 + 8 * 256 <= 8 << 20 < nq * 32 + nt * 32   # the halves are staged, the whole is not
    parts = [ctx.match_bruteforce(q[a:b], t, np.arange(b - a + 1, dtype=np.uint32), cand[a:b]) for a, b in ((0, h), (h, nq))]
    for k in range(3):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts]))
    assert np.array_equal(whole[0], cand.astype(np.int32)) and whole[1].max() <= 32 and (whole[2] == INT_MAX).all()


def test_eval_edges_unstaged_branch_equals_staged_pieces(ctx):
    """61 200 edges with both Jacobian outputs: 19 MB of inputs and results, past the 16 MB the staging buffer takes.  Against the same
    edges evaluated in four staged pieces (an edge's results depend on that edge alone)."""
    p = ba_synth.make_problem(seed=2, n_kf=12, n_pt=120)
    e = len(p["edge_pose"])
    rep = -(-61_200 // e)
    big = {k: (np.concatenate([v] * rep)[:61_200] if k in ("edge_pose", "edge_point", "meas", "is_stereo", "info", "huber_delta") else v)
           for k, v in p.items()}
    E = len(big["edge_pose"])
    assert E == 61_200 and E * (49 + 265) > 16 << 20 > E // 4 * (49 + 265) + (1 << 16)
    whole = ctx.ba_eval_edges(**big)
    cut = [0, E // 4, E // 2, 3 * E // 4, E]
    parts = [ctx.ba_eval_edges(**{k: (v[a:b] if k in ("edge_pose", "edge_point", "meas", "is_stereo", "info", "huber_delta") else v)
                                  for k, v in big.items()}) for a, b in zip(cut, cut[1:])]
    for k in whole:
        assert np.array_equal(whole[k], np.concatenate([q[k] for q in parts])), k
    assert whole["chi2"].any() and whole["j_pose"].any()
