"""Scenes for orbfe_track_reference_stored, built on the CPU as reloc_refine_scenes.py builds its own: the frame is the
oracle's extraction of one KITTI-shaped synthetic pair (1241 x 376, 2000 features), the vocabulary synth_vocab.trained(0, k=10, L=4), the
reference keyframe a jittered, bit-flipped subset of a few hundred of the frame's own features with map points at the stereo depth under a
true pose a few centimetres from the pose the frame comes with.  The keyframe's FeatureVector is the restatement's transform of its own
descriptors.  levelsup is 2 unless a scene says otherwise: with four levels that is the hundred nodes of level 2, what the reference's
levelsup = 4 gives on its six-level vocabulary; levelsup = 4 puts every feature under the root and is a shape scene of its own.

A keyframe is made of groups, every one derived from distinct features of the frame, shuffled into no particular order:
  match   good points at the true position (with a little noise): matched, optimised, inliers
  bad     good points metres off: matched, thrown out by the optimisation
  dup     second keyframe features on the frame features of some `match` ones, in the same node: both match, the last one keeps the feature
  fill    features without a point (never search), and good points with random descriptors that match nothing
The frame may arrive holding points (own): those features are edges, not candidates, and come back as OWN or -1."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_restatement as br  # noqa: E402
import bow_search_scenes as bs  # noqa: E402
import reloc_refine_scenes as rs  # noqa: E402
import track_reference_restatement as tr  # noqa: E402
from reloc_refine_scenes import BOUNDS, CAM, CX, CY, FX, FY, H, INV_SIGMA2, NF, SIGMA2, W, frame, quat_to_R  # noqa: E402,F401

LEVELSUP = 2
_voc = {}


def vocabulary():
    """(the generated arrays, their child table) of synth_vocab.trained(0, k=10, L=4), made once"""
    if not _voc:
        from orb_slam2_ros2_amd import synth_vocab
        voc = synth_vocab.trained(0, k=10, L=4)
        _voc["v"] = (voc, br._table(voc))
    return _voc["v"]


# verifyAngle's scene: the differences angle_frame - angle_keyframe of the matched features, as (bin centre, share): bins 0, 3 and 8 are
# chosen, the quarter spread over five other bins is dropped
ANGLE_MIX = ((6.0, 0.35), (42.0, 0.22), (102.0, 0.18), (150.0, 0.05), (198.0, 0.05), (246.0, 0.05), (294.0, 0.05), (330.0, 0.05))


def build(orc, image_seed=3, n_match=60, n_bad=0, n_dup=0, n_fill=150, n_own=0, own_bad=0, own_on_matched=0, mono=False, angles=False,
          levelsup=LEVELSUP, noise=0.01, rng_seed=None):
    voc, tab = vocabulary()
    fr = frame(orc, image_seed)
    rng = np.random.default_rng(7000 * image_seed + n_match if rng_seed is None else rng_seed)
    kps, desc = fr["lk"], fr["ld"]
    n = len(kps)
    ru = np.full(NF, -1.0)
    ru[:n] = fr["right_u"][:n]
    dp = fr["depth"][:n]
    q = np.array([0.01, -0.02, 0.005, 1.0]); q /= np.linalg.norm(q)
    Rt, tt = quat_to_R(q), np.array([0.05, -0.02, 0.1])
    depth = np.where(dp > 0, dp, rng.uniform(4, 30, n))
    pc = np.stack([(kps["x"] - CX) / FX * depth, (kps["y"] - CY) / FY * depth, depth], 1)
    Xw = (pc - tt) @ Rt
    rest = rng.permutation(n)
    take = lambda k: (rest[:k], rest[k:])
    match, rest = take(n_match)
    bad, rest = take(n_bad)
    fill, rest = take(n_fill)
    own, rest = take(n_own)
    dup = match[:n_dup]

    groups = []   # (frame feature, x, y, descriptor, position, good, angle difference)

    def add(fs, s, bits, pos, good, d=None):
        d = rs._flip(rng, desc[fs], bits) if d is None else d
        x, y = kps["x"][fs] + rng.normal(0, s, len(fs)), kps["y"][fs] + rng.normal(0, s, len(fs))
        for k, f in enumerate(fs):
            groups.append((int(f), float(x[k]), float(y[k]), d[k], pos[k], good))

    off = lambda fs: Xw[fs] + rng.uniform(2.0, 5.0, (len(fs), 3)) * rng.choice([-1.0, 1.0], (len(fs), 3))
    add(match, 1.5, 6, Xw[match] + rng.normal(0, noise, (len(match), 3)), 1)
    add(bad, 1.5, 6, off(bad), 1)
    add(dup, 1.0, 9, Xw[dup] + rng.normal(0, noise, (len(dup), 3)), 1)
    half = len(fill) // 2
    add(fill[:half], 2.0, 0, Xw[fill[:half]], 0)
    add(fill[half:], 2.0, 0, Xw[fill[half:]], 1, d=rng.integers(0, 256, (len(fill) - half, 32)).astype(np.uint8))

    perm = rng.permutation(len(groups))
    groups = [groups[k] for k in perm]
    m = len(groups)
    kf_kps = np.zeros(m, kps.dtype)
    kf_desc = np.zeros((m, 32), np.uint8)
    pos = np.zeros((m, 3), np.float32)
    good = np.zeros(m, np.uint8)
    src = np.zeros(m, np.int64)
    for i, (f, x, y, d, p, g) in enumerate(groups):
        kf_kps[i] = kps[f]
        kf_kps[i]["x"], kf_kps[i]["y"] = np.float32(x), np.float32(y)
        kf_desc[i], pos[i], good[i], src[i] = d, p.astype(np.float32), g, f
    if angles:
        diffs = np.concatenate([np.full(int(round(share * m)) + 1, c) for c, share in ANGLE_MIX])[:m]
        diffs = diffs[rng.permutation(m)] + rng.uniform(-4.0, 4.0, m)
        kf_kps["angle"] = bs.wrap_angle(kps["angle"][src].astype(np.float64) - diffs)      # (the extractor's range)
    frame_good = frame_pos = None
    if n_own or own_on_matched:
        own = np.concatenate([own, match[n_dup:n_dup + own_on_matched]])       # some of them on features the keyframe would have matched
        frame_good = np.zeros(NF, np.uint8)
        frame_pos = np.zeros((NF, 3), np.float32)
        frame_good[own] = 1
        frame_pos[own] = (Xw[own] + rng.normal(0, noise, (len(own), 3))).astype(np.float32)
        frame_pos[own[:own_bad]] = off(own[:own_bad]).astype(np.float32)
    q0 = q + np.array([0.002, -0.001, 0.0015, 0.0]); q0 /= np.linalg.norm(q0)
    t0 = tt + np.array([0.03, -0.02, 0.04])
    kf_fv = br.transform(voc, kf_desc, levelsup, tab)[2:]
    return dict(image_seed=image_seed, nf=NF, kps=kps, desc=desc, n_kp=n, right_u=None if mono else ru, kf_kps=kf_kps, kf_desc=kf_desc, kf_fv=kf_fv,
                good=good, pos=pos, src=src, frame_good=frame_good, frame_pos=frame_pos, Rcw=quat_to_R(q0).astype(np.float32).reshape(9),
                tcw=t0.astype(np.float32), cam=CAM, bounds=BOUNDS, sigma2=SIGMA2, inv_sigma2=INV_SIGMA2, levelsup=levelsup)


def restate(orc, s, **kw):
    return tr.track(orc, s, voc=vocabulary()[0], levelsup=s["levelsup"], **kw)


# the free-running scenes, one per verdict
VERDICT_SCENES = {
    "REJECT_MATCHES": dict(image_seed=3, n_match=40, n_fill=100, want_matches=9),
    "REJECT_INLIERS": dict(image_seed=8, n_match=40, n_bad=30, n_fill=100, want_inliers=9),
    "ACCEPT": dict(image_seed=11, n_match=250, n_bad=20, n_dup=10, n_fill=150),
}
# 9 / 10 matches and 9 / 10 inliers: a larger scene whose surplus is cleared until the restated count is the one wanted
BOUNDARY_SCENES = {
    "matches_9": (dict(image_seed=3, n_match=30, n_fill=60, want_matches=9, rng_seed=4242), "REJECT_MATCHES"),
    "matches_10": (dict(image_seed=3, n_match=30, n_fill=60, want_matches=10, rng_seed=4242), "ACCEPT"),
    "inliers_9": (dict(image_seed=3, n_match=30, n_bad=6, n_fill=60, want_inliers=9, rng_seed=4243), "REJECT_INLIERS"),
    "inliers_10": (dict(image_seed=3, n_match=30, n_bad=6, n_fill=60, want_inliers=10, rng_seed=4243), "ACCEPT"),
}


def margins(orc, s, o):
    """the smallest relative distance of an edge's chi2 from its threshold at the restated estimate (inf without an optimisation)"""
    if o["n_edges"] == 0:
        return np.inf
    _, c2, th = tr.chi2(s, o["assigned"], o["pose_se3"])
    return float(np.abs(c2 / th - 1.0).min())


def trimmed(orc, want_matches=None, want_inliers=None, **kw):
    """build(**kw), then `good` cleared on surplus matched keyframe features -- the last match's, or the last inlier match's -- until the
    restatement counts exactly want_matches matches or want_inliers inliers.  Asserts the count and that no edge lies within 1 % of its
    chi-square threshold, so that an implementation cannot differ there by rounding.  -> (scene, the restatement's result)"""
    s = build(orc, **kw)
    s["good"] = s["good"].copy()
    for _ in range(len(s["good"])):
        o = restate(orc, s)
        if want_matches is not None:
            if o["n_matches"] <= want_matches:
                break
            s["good"][o["matches"][-1][1]] = 0
        else:
            if o["n_inliers"] <= want_inliers:
                break
            inl = [t for (qf, t, _) in o["matches"] if o["inlier"][qf] and o["assigned"][qf] == t]
            s["good"][inl[-1]] = 0
    assert (o["n_matches"] if want_matches is not None else o["n_inliers"]) == (want_matches if want_matches is not None else want_inliers)
    assert margins(orc, s, o) > 0.01, "an edge within 1 % of its chi-square threshold"
    return s, o


_restated = {}


def restated(orc, name):
    """(scene, the restatement's result) of a named scene of VERDICT_SCENES or BOUNDARY_SCENES, computed once, shared by the tests and left
    unchanged"""
    if name not in _restated:
        kw = dict(VERDICT_SCENES[name] if name in VERDICT_SCENES else BOUNDARY_SCENES[name][0])
        if "want_matches" in kw or "want_inliers" in kw:
            _restated[name] = trimmed(orc, **kw)
        else:
            s = build(orc, **kw)
            _restated[name] = (s, restate(orc, s))
    return _restated[name]


# ---- the shape scenes ------------------------------------------------------------------------------------------------------------------
def shape(orc, name):
    """-> (scene, restatement, parameters of the call)"""
    kw = {}
    if name == "dup":          # two keyframe features of one node pick the same frame feature
        s = build(orc, image_seed=3, n_match=60, n_dup=12, rng_seed=501)
    elif name == "angles":     # verifyAngle drops at least a fifth, bin 0 is one of the three
        s = build(orc, image_seed=8, n_match=300, n_fill=60, angles=True, rng_seed=502)
    elif name == "own":        # the frame arrives holding points, some of them bad, some on features the keyframe would have matched
        s = build(orc, image_seed=11, n_match=120, n_own=90, own_bad=12, own_on_matched=10, rng_seed=503)
    elif name == "mono":
        s = build(orc, image_seed=3, n_match=120, n_bad=10, mono=True, rng_seed=504)
    elif name == "no_good":    # a keyframe with no good point: 0 matches
        s = build(orc, image_seed=3, n_match=60, rng_seed=505)
        s["good"] = np.zeros_like(s["good"])
    elif name == "root":       # levelsup = 4 on four levels: every feature under the root, one node
        s = build(orc, image_seed=8, n_match=80, n_dup=5, levelsup=4, rng_seed=506)
    elif name == "one":        # a stored keyframe of one feature, no minimum of matches
        b = build(orc, image_seed=3, n_match=60, n_fill=0, rng_seed=507)
        o = restate(orc, b)
        i = o["matches"][0][1]
        s = dict(b, kf_kps=b["kf_kps"][i:i + 1], kf_desc=b["kf_desc"][i:i + 1], good=np.ones(1, np.uint8), pos=b["pos"][i:i + 1], src=b["src"][i:i + 1])
        s["kf_fv"] = br.transform(vocabulary()[0], s["kf_desc"], s["levelsup"], vocabulary()[1])[2:]
        kw = dict(min_matches=0)
    else:
        raise KeyError(name)
    return s, restate(orc, s, **kw), kw


SHAPES = ("dup", "angles", "own", "mono", "no_good", "root", "one")
