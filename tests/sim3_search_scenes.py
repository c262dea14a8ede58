"""Scenes for the searchBySim3 tests: two keyframes (tri_scenes.make_kf) that see the same points while their world frames differ by a
known similarity, loop-group points for the map-point overload, one scene placed by hand whose every feature is there for a reason, and
single-window scenes with a chosen number of candidates.  A keyframe is the dict of sim3_search_restatement.py."""
from __future__ import annotations

import numpy as np

import tri_scenes as ts
from orb_slam2_ros2_amd._lib import KP_DTYPE

F32 = np.float32
CAM, SF, W, H = ts.CAM, ts.SF, ts.W, ts.H
IMAGE = (0.0, float(W), 0.0, float(H))
WIDE = (-12.5, 655.0, -9.25, 492.5)            # a distorted camera's undistorted bounds
GOOD, INMAP = 1, 2


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def add_to_store(st, kf, kf_id):
    st.add(kf_id, kf["kps"], kf["desc"], bounds=kf["bounds"])
    return kf_id


def side(kf, kf_id):
    """the map state of a keyframe as Context.search_by_sim3_stored takes it"""
    return dict(id=kf_id, flags=kf["flags"], pos=kf["pos"], max_dist=kf["max_dist"], min_dist=kf["min_dist"], Rcw=kf["Rcw"], tcw=kf["tcw"])


def frames_kf(kf):
    """... as MatcherExt.searchBySim3Frames takes it"""
    return dict(kps=kf["kps"], desc=kf["desc"], pos=kf["pos"], good=(kf["flags"] & GOOD) != 0, inmap=(kf["flags"] & INMAP) != 0,
                max_dist=kf["max_dist"], min_dist=kf["min_dist"])


# ---- seeded ------------------------------------------------------------------------------------------------------------------------------
def seeded(seed=0, s=1.0, n=300, n_pts=420, bounds_c=IMAGE, bounds_m=WIDE, m_loop=400, n_matches=30):
    """C and M look at one cloud from two places.  C's map is metric; M's map is the same world shrunk by s (positions and camera
    translation divided by s), so that p_c = s R_cm p_m + t_cm.  The distance range of a point is centred on the octave of its feature.
    Loop-group points (the points M sees, given in M's world) go into C with Scw = the similarity from M's world into C's camera."""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-5, 5, n_pts), rng.uniform(-3.5, 3.5, n_pts), rng.uniform(5, 12, n_pts)], 1)
    base = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)
    out = {}
    for name, centre, R, bounds in (("C", (0.0, 0.0, 0.0), rot(0.01, -0.02, 0.015), bounds_c), ("M", (0.35, -0.1, 0.2), rot(-0.02, 0.04, -0.01), bounds_m)):
        kf = ts.make_kf(rng, pts, base, centre, R, n=n, good_frac=0.7, flip_bits=8)
        scale = 1.0 if name == "C" else 1.0 / s
        Tcw = kf["Tcw"].astype(np.float64)
        pc = (Tcw[:3, :3] @ pts[kf["pid"]].T).T + Tcw[:3, 3]
        dist = np.linalg.norm(pc, axis=1) * scale
        k = len(kf["kps"])
        noise = rng.normal(0, 0.01, (k, 3))
        out[name] = dict(kps=kf["kps"], desc=kf["desc"], bounds=bounds, flags=kf["flags"], pid=kf["pid"],
                         pos=((pts[kf["pid"]] + noise) * scale).astype(F32),
                         max_dist=(dist * 1.2 ** kf["kps"]["octave"] * rng.uniform(0.97, 1.03, k)).astype(F32),
                         min_dist=(dist * rng.uniform(0.2, 0.5, k)).astype(F32),
                         Rcw=Tcw[:3, :3].astype(F32), tcw=(Tcw[:3, 3] * scale).astype(F32), Tcw=Tcw)
    Tc, Tm = out["C"]["Tcw"], out["M"]["Tcw"]
    Rcm = Tc[:3, :3] @ Tm[:3, :3].T
    tcm = Tc[:3, 3] - Rcm @ Tm[:3, 3]
    C, M = out["C"], out["M"]
    # the matches the solver came with: pairs of features of one point, both good and in the map
    of_m = {int(p): j for j, p in enumerate(M["pid"])}
    both = [(i, of_m[int(p)]) for i, p in enumerate(C["pid"]) if int(p) in of_m and C["flags"][i] == 3 and M["flags"][of_m[int(p)]] == 3]
    matches = both[::4][:n_matches]
    # the loop group: M's points in M's world; Scw takes M's world into C's camera: p_c = s R_cm (R_mw p + t_mw) + t_cm
    Rcw_l = Rcm @ Tm[:3, :3]
    tcw_l = s * (Rcm @ (Tm[:3, 3] / s)) + tcm
    sel = rng.permutation(n_pts)[:m_loop] if m_loop <= n_pts else rng.integers(0, n_pts, m_loop)     # (a large group: points repeat)
    Xm = pts[sel] / s
    pc = s * (Rcw_l @ Xm.T).T + tcw_l
    d = np.linalg.norm(pc, axis=1) / s
    octave = (sel * 31) % 3
    centre_m = -(Tm[:3, :3].T @ Tm[:3, 3]) / s
    vd = Xm - centre_m
    vd /= np.linalg.norm(vd, axis=1)[:, None]
    flip = rng.random(m_loop) < 0.1
    vd[flip] *= -1                                                   # seen from behind: the viewing-angle test
    desc = base[sel].copy()
    for i in range(m_loop):
        for b in rng.integers(0, 256, rng.integers(0, 7)):
            desc[i, b >> 3] ^= np.uint8(1 << (b & 7))
    loop = dict(usable=rng.random(m_loop) < 0.85, pos=Xm.astype(F32), view_dir=vd.astype(F32), desc=desc,
                max_dist=(d * 1.2 ** octave * rng.uniform(0.97, 1.03, m_loop)).astype(F32), min_dist=(d * rng.uniform(0.2, 0.5, m_loop)).astype(F32),
                id=np.arange(5000, 5000 + m_loop))
    return dict(C=C, M=M, Scm=(F32(s), Rcm.astype(F32), tcm.astype(F32)), matches=matches, loop=loop,
                Scw=(F32(s), Rcw_l.astype(F32), tcw_l.astype(F32)), th=7.5)


# ---- by hand -----------------------------------------------------------------------------------------------------------------------------
def flipped(desc, bits):
    d = np.array(desc, np.uint8)
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


class Builder:
    """features one by one"""

    def __init__(self, bounds, R, centre):
        self.rows, self.bounds = [], bounds
        Tcw = ts.pose(centre, R)[0].astype(np.float64)
        self.R, self.t = Tcw[:3, :3], Tcw[:3, 3]

    def add(self, x, y, octave, desc, flags=0, pos=(0, 0, 1), mx=1.0, mn=0.0):
        self.rows.append((x, y, octave, np.array(desc, np.uint8), flags, pos, mx, mn))
        return len(self.rows) - 1

    def world(self, p_cam):
        return self.R.T @ (np.asarray(p_cam, np.float64) - self.t)

    def kf(self):
        n = len(self.rows)
        kps = np.zeros(n, KP_DTYPE)
        kps["x"], kps["y"], kps["octave"] = [r[0] for r in self.rows], [r[1] for r in self.rows], [r[2] for r in self.rows]
        kps["size"], kps["class_id"] = 7.0, -1
        return dict(kps=kps, desc=np.stack([r[3] for r in self.rows]), bounds=self.bounds, flags=np.array([r[4] for r in self.rows], np.uint8),
                    pos=np.array([r[5] for r in self.rows], F32), max_dist=np.array([r[6] for r in self.rows], F32),
                    min_dist=np.array([r[7] for r in self.rows], F32), Rcw=self.R.astype(F32), tcw=self.t.astype(F32))


def ray(u, v, depth):
    fx, fy, cx, cy = (float(c) for c in CAM)
    return np.array([(u - cx) / fx * depth, (v - cy) / fy * depth, depth])


def hand():
    """Every rejection reason in both directions and for the points, the merge's three collisions, octaves 0 and 7, the source-bounds rule.
    C has the image as bounds, M the wide bounds.  findFeaturesInArea returns whole grid cells, so every case has a cell of its own (a spot
    is a cell's centre; an octave-1 window stays inside the cell), and the features that are only sources sit in the far corner cell."""
    rng = np.random.default_rng(77)
    s, Rcm, tcm = 1.25, rot(0.02, -0.03, 0.01), np.array([0.1, -0.05, 0.08])
    B = dict(C=Builder(IMAGE, rot(0.03, 0.01, -0.02), (0.2, 0.1, -0.1)), M=Builder(WIDE, rot(-0.01, 0.02, 0.03), (-0.3, 0.05, 0.1)))
    rnd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)  # noqa: E731
    spots = iter([(64.0 * i + 32, 48.0 * j + 24) for j in range(8) for i in range(9)])
    notes = {}

    def source(d, target_cam, octave, desc, flags=3, mx_f=None, mn_f=0.5, xy=(608.0, 456.0)):
        """a feature of the direction's source keyframe whose map point lands at target_cam in the target camera"""
        Y = np.asarray(target_cam, np.float64)
        if d == "A":                                   # C -> M through Scm.inv(): pm = Y means pc = s R Y + t; d = |pm| / s' = |Y| s
            p_src, dist, b = s * (Rcm @ Y) + tcm, np.linalg.norm(Y) * s, B["C"]
        else:                                          # M -> C through Scm: pc = Y means pm = R^T (Y - t) / s; d = |pc| / s
            p_src, dist, b = Rcm.T @ (Y - tcm) / s, np.linalg.norm(Y) / s, B["M"]
        mx = dist * (1.2 ** octave if mx_f is None else mx_f)
        return b.add(xy[0], xy[1], octave, desc, flags, b.world(p_src), mx, dist * mn_f)

    for d in ("A", "B"):
        T = B["M" if d == "A" else "C"]
        src_bounds = IMAGE if d == "A" else WIDE
        n = {}
        # geometry
        n["z"] = source(d, (0.1, 0.1, -4.0), 1, rnd())
        n["u_max"] = source(d, ray(src_bounds[1] + 6, 200, 6), 1, rnd())
        n["u_min"] = source(d, ray(src_bounds[0] - 6, 200, 6), 1, rnd())
        n["v_max"] = source(d, ray(300, src_bounds[3] + 6, 6), 1, rnd())
        n["v_min"] = source(d, ray(300, src_bounds[2] - 6, 6), 1, rnd())
        u, v = next(spots)
        n["d_max"] = source(d, ray(u, v, 6), 1, rnd(), mx_f=0.9)
        n["d_min"] = source(d, ray(u, v, 6), 1, rnd(), mx_f=2.0, mn_f=1.1)
        # the candidate list
        u, v = next(spots)
        n["no_candidate"] = source(d, ray(u, v, 6), 1, rnd())
        u, v = next(spots)
        q = rnd()
        T.add(u + 2, v, 5, q, 3)                                          # right place, wrong octave
        n["no_candidate_octave"] = source(d, ray(u, v, 6), 1, q)
        u, v = next(spots)
        q = rnd()
        T.add(u + 1, v + 1, 1, q, GOOD), T.add(u - 1, v, 1, q, 0), T.add(u, v - 2, 2, q, INMAP)
        n["flags"] = source(d, ray(u, v, 6), 1, q)
        u, v = next(spots)
        T.add(u + 1, v, 1, rnd(), 3)
        n["threshold"] = source(d, ray(u, v, 6), 1, rnd())
        u, v = next(spots)
        q = rnd()
        T.add(u + 1, v, 1, flipped(q, range(0, 50)), 3)                   # exactly the threshold: accepted (<=)
        n["threshold_equal"] = source(d, ray(u, v, 6), 1, q)
        u, v = next(spots)
        q = rnd()
        T.add(u + 1, v, 1, flipped(q, range(0, 51)), 3)
        n["threshold_plus_one"] = source(d, ray(u, v, 6), 1, q)
        u, v = next(spots)
        q = rnd()
        T.add(u + 1, v, 1, flipped(q, range(0, 8)), 3), T.add(u - 1, v, 1, flipped(q, range(10, 20)), 3)   # 8 / 10 = 0.8 > 0.75
        n["ratio"] = source(d, ray(u, v, 6), 1, q)
        u, v = next(spots)
        q = rnd()
        T.add(u + 1, v, 1, flipped(q, range(0, 6)), 3), T.add(u - 1, v, 1, flipped(q, range(10, 18)), 3)    # 6 / 8 = 0.75: accepted (<=)
        n["ratio_equal"] = source(d, ray(u, v, 6), 1, q)
        u, v = next(spots)
        q = rnd()
        T.add(u + 1, v, 1, flipped(q, range(10, 20)), 3), T.add(u - 1, v, 1, flipped(q, range(0, 8)), 3)   # the better one second: no second best
        n["record_order"] = source(d, ray(u, v, 6), 1, q)
        u, v = next(spots)
        q = rnd()
        T.add(u + 1, v, 1, q, 3), T.add(u - 1, v, 1, q, 3)                                                 # 0 / 0
        n["nan"] = source(d, ray(u, v, 6), 1, q)
        u, v = next(spots)
        q = rnd()
        n["single_target"] = T.add(u + 1, v, 1, flipped(q, [3, 77]), 3)                                    # one candidate: second = INT_MAX
        n["single"] = source(d, ray(u, v, 6), 1, q)
        # octaves 0 and 7: windows -1 .. 1 and 6 .. 8
        u, v = next(spots)
        q = rnd()
        T.add(u, v + 1, 2, q, 3), T.add(u + 1, v, 0, flipped(q, [1, 2, 3]), 3)
        n["octave0"] = source(d, ray(u, v, 6), 0, q, mx_f=1.05)
        u, v = next(spots)
        q = rnd()
        T.add(u, v + 1, 5, q, 3), T.add(u + 1, v, 7, flipped(q, [1, 2, 3]), 3)
        n["octave7"] = source(d, ray(u, v, 6), 7, q, mx_f=1.2 ** 9)                                        # predicted 9, clamped to 7
        notes[d] = n
    C, M = B["C"], B["M"]
    # the source-bounds rule: a point that lands between the image and the wide bounds, with a matching feature within reach
    q = rnd()
    C.add(634.0, 200.0, 1, flipped(q, [5]), 3)
    notes["B"]["between_bounds"] = source("B", ray(646, 200, 6), 1, q)          # source M: inside M's bounds -> accepted
    q = rnd()
    M.add(644.0, 300.0, 1, flipped(q, [5]), 3)
    notes["A"]["between_bounds"] = source("A", ray(646, 300, 6), 1, q)          # source C: outside C's bounds -> u_max
    # features outside the image (the wide bounds allow them): border cells of M's grid
    q = rnd()
    notes["A"]["outside_target"] = M.add(-8.0, -5.0, 1, flipped(q, [9]), 3)
    notes["A"]["outside"] = source("A", ray(3.0, 4.0, 6), 1, q)
    # the merge.  (1) A and B agree on a pair: B's key is already there
    u, v = next(spots)
    u2, v2 = next(spots)
    q = rnd()
    ic = source("A", ray(u, v, 6), 1, q, xy=(u2, v2))
    im = source("B", ray(u2, v2, 6), 1, flipped(q, [4]), xy=(u, v))
    notes["mutual"] = (ic, im)
    # (2) two sources of B with one key; C's feature is no source itself
    u, v = next(spots)
    q = rnd()
    k = C.add(u, v, 1, q, 3, pos=C.world((0, 0, -3.0)))
    notes["shared_key"] = (k, source("B", ray(u, v, 6), 1, flipped(q, [1])), source("B", ray(u + 1, v, 6), 1, flipped(q, [2])))
    # (3) a new key that is the queryIdx of an input match
    u, v = next(spots)
    q = rnd()
    q0 = C.add(u, v, 1, q, 3, pos=C.world((0, 0, 5.0)), mx=50.0)
    t0 = M.add(600.0, 450.0, 3, rnd(), 3, pos=M.world((0, 0, 5.0)), mx=50.0)
    notes["repeat_query"] = (q0, t0, source("B", ray(u, v, 6), 1, flipped(q, [7])))
    C, M = C.kf(), M.kf()
    # loop points against M (its wide bounds), Scw arbitrary: p_c = s R p_w + t
    sw, Rw, tw = 0.8, rot(-0.02, 0.05, 0.02), np.array([0.3, -0.2, 0.4])
    rows, pn = [], {}

    def point(name, cam, octave, desc, usable=1, mx_f=None, mn_f=0.5, view=1.0):
        Y = np.asarray(cam, np.float64)
        Xw = Rw.T @ (Y - tw) / sw
        dist = np.linalg.norm(Y) / sw
        vd = Rw.T @ (Y / np.linalg.norm(Y)) * view
        rows.append((usable, Xw, vd, dist * (1.2 ** octave if mx_f is None else mx_f), dist * mn_f, desc))
        pn[name] = len(rows) - 1

    feat = {name: int(notes["A"][name + "_target"]) for name in ("single", "outside")}
    point("unusable", ray(100, 100, 6), 1, rnd(), usable=0)
    point("z", (0, 0, -2.0), 1, rnd())
    point("u_max", ray(WIDE[1] + 4, 200, 6), 1, rnd())
    point("u_min", ray(WIDE[0] - 4, 200, 6), 1, rnd())
    point("v_max", ray(200, WIDE[3] + 4, 6), 1, rnd())
    point("v_min", ray(200, WIDE[2] - 4, 6), 1, rnd())
    kx, ky = float(M["kps"]["x"][feat["single"]]), float(M["kps"]["y"][feat["single"]])
    qd = M["desc"][feat["single"]]
    point("d_max", ray(kx, ky, 6), 1, qd, mx_f=0.9)
    point("d_min", ray(kx, ky, 6), 1, qd, mx_f=2.0, mn_f=1.1)
    point("view", ray(kx, ky, 6), 1, qd, view=-1.0)
    point("accepted", ray(kx, ky, 6), 1, flipped(qd, [100, 101]))
    point("accepted_again", ray(kx + 1, ky, 6), 1, flipped(qd, [102]))          # a later point overwrites an earlier one
    point("no_candidate", ray(kx, ky, 6), 3, qd)
    point("threshold", ray(kx, ky, 6), 1, rnd())
    for name in ("ratio", "nan", "octave0", "octave7", "flags"):                  # the spots direction A built in M (no flag filter here)
        i = notes["A"][name]
        p = sim_target_of_a(C, i, s, Rcm, tcm)
        octave = {"octave0": 0, "octave7": 7}.get(name, 1)
        point(name, ray(p[0], p[1], 6), octave, C["desc"][i], mx_f={"octave7": 1.2 ** 9, "octave0": 1.05}.get(name))
    point("outside", ray(3.0, 4.0, 6), 1, M["desc"][feat["outside"]])
    loop = dict(usable=np.array([r[0] for r in rows], np.uint8), pos=np.array([r[1] for r in rows], F32), view_dir=np.array([r[2] for r in rows], F32),
                max_dist=np.array([r[3] for r in rows], F32), min_dist=np.array([r[4] for r in rows], F32), desc=np.stack([r[5] for r in rows]),
                id=np.arange(len(rows)))
    return dict(C=C, M=M, Scm=(F32(s), Rcm.astype(F32), tcm.astype(F32)), matches=[(notes["repeat_query"][0], notes["repeat_query"][1])],
                loop=loop, loop_target="M", Scw=(F32(sw), Rw.astype(F32), tw.astype(F32)), th=7.5, ratio=0.75, notes=notes, point_notes=pn)


def sim_target_of_a(C, i, s, Rcm, tcm):
    """pixel in M where direction A sends feature i of C (float64; for placing things)"""
    pc = C["Rcw"].astype(np.float64) @ C["pos"][i].astype(np.float64) + C["tcw"].astype(np.float64)
    pm = Rcm.T @ (pc - tcm) / s
    fx, fy, cx, cy = (float(c) for c in CAM)
    return fx * pm[0] / pm[2] + cx, fy * pm[1] / pm[2] + cy


# ---- one window with a chosen candidate list ---------------------------------------------------------------------------------------------
def window(n_pass, dists=None, at=(352.0, 264.0), bounds=IMAGE, seed=5, n_decoys=40):
    """A target keyframe whose n_pass good features of octave 1 lie inside the window of one projected point, all in one grid cell when `at`
    is a cell's centre (list order = index order), between decoys that the octave window or the flags remove; dists[k]: Hamming distance of
    candidate k to the point's descriptor (default: 20 + k % 30).  Identity poses and similarity; the same point as a pair source (C has
    one feature) and as a loop point.  Returns a scene and the expected list length."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, 32, dtype=np.uint8)
    I = np.eye(3)
    M, C = Builder(bounds, I, (0, 0, 0)), Builder(IMAGE, I, (0, 0, 0))
    order = rng.permutation(n_pass + n_decoys)
    k = 0
    for slot in order:                                   # decoys interleaved with the candidates, candidates in index order
        ang, r = rng.uniform(0, 2 * np.pi), rng.uniform(0, 6.0)
        x, y = at[0] + r * np.cos(ang), at[1] + r * np.sin(ang)
        if slot < n_pass:
            d = (20 + k % 30) if dists is None else dists[k]
            M.add(x, y, int(rng.integers(0, 3)), flipped(q, rng.permutation(256)[:d]), 3)
            k += 1
        elif slot % 2:
            M.add(x, y, int(rng.integers(3, 8)), flipped(q, [1]), 3)       # outside the octave window
        else:
            M.add(x, y, 1, flipped(q, [1]), int(rng.integers(0, 3)))        # removed by vGoodIndices (the points overload keeps these)
    p = ray(at[0], at[1], 6.0)
    dist = float(np.linalg.norm(p))
    C.add(100.0, 100.0, 1, q, 3, p, dist * 1.2, dist * 0.5)
    loop = dict(usable=np.ones(1, np.uint8), pos=np.array([p], F32), view_dir=np.array([p / dist], F32), max_dist=np.array([dist * 1.2], F32),
                min_dist=np.array([dist * 0.5], F32), desc=q[None], id=np.arange(1))
    ident = (F32(1), np.eye(3, dtype=F32), np.zeros(3, F32))
    return dict(C=C.kf(), M=M.kf(), Scm=ident, matches=[], loop=loop, loop_target="M", Scw=ident, th=7.5)


def quarter(scene):
    """the scene through a camera of a quarter of the resolution (160 x 120): pixel coordinates and intrinsics divided by four, both
    keyframes with the image as bounds"""
    out = dict(scene)
    for k in ("C", "M"):
        kps = scene[k]["kps"].copy()
        kps["x"], kps["y"] = kps["x"] / F32(4), kps["y"] / F32(4)
        out[k] = dict(scene[k], kps=kps, bounds=(0.0, 160.0, 0.0, 120.0))
    out["cam"] = tuple(F32(c) / F32(4) for c in CAM)
    return out
