"""Scenes for orbfe_reloc_refine_stored, built on the CPU: the frame is the oracle's extraction of one KITTI-shaped synthetic
pair (1241 x 376, 2000 features: the project's smallest frame with a realistic grid), the candidate keyframe a jittered, bit-flipped subset
of the frame's own features with map points at the stereo depth under a true pose -- what a keyframe that saw the same place looks like.

A keyframe is made of groups, every one derived from distinct features of the frame, shuffled into no particular order:
  seeds   the PnP inliers: held[f] names them; their points are exact (no noise unless asked for), so every seed edge is an inlier
  near    queries a few pixels from their feature, found by both searches; good points (with noise) or `bad` ones, metres off, that the
          second optimisation throws out again
  far     queries placed 6 sigma2(octave) pixels left of the grid column of their feature: the box of th = 10 reaches that column, the
          box of th = 3 does not (findFeaturesInArea goes by grid cell), so only the first search finds them; bad points
  dup     second queries on the features of some near queries: both are accepted, the last one keeps the feature
  border  queries on and beyond the image border
  fill    features without a point, and good points with random descriptors that match nothing
plus three seeds whose keyframe point is bad (setCurrFrameAttrib skips them)."""
from __future__ import annotations

import numpy as np

from orb_slam2_ros2_amd import synth

W, H, NF = 1241, 376, 2000
FX, FY, CX, CY = 718.856, 718.856, 607.1928, 185.2157
BASELINE = 0.537166
BF = 718.856 * BASELINE
CAM = (FX, FY, CX, CY, BF)
BOUNDS = (0.0, float(W), 0.0, float(H))
SF = np.array([np.float32(1.2) ** l for l in range(8)], np.float32)
SIGMA2 = (SF * SF).astype(np.float32)
INV_SIGMA2 = (np.float32(1.0) / SIGMA2).astype(np.float32)
KF_ID = 77

_frames = {}


def frame(orc, image_seed):
    """the oracle's stereo frame of the synthetic pair -> dict(lk, ld, right_u, depth, ...), computed once per seed and left unchanged"""
    if image_seed not in _frames:
        L, R = synth.stereo_pair(image_seed)
        _frames[image_seed] = orc.stereo_frame(L, R, n_features=NF, fx=FX, bf=BF)
    return _frames[image_seed]


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _flip(rng, d, bits):
    d = d.copy()
    fl = rng.integers(0, 256, (len(d), bits))
    for k in range(bits):
        d[np.arange(len(d)), fl[:, k] // 8] ^= (1 << (fl[:, k] % 8)).astype(np.uint8)
    return d


def build(orc, image_seed=3, n_seed=30, n_near=0, near_bad=False, n_far=0, n_dup=0, n_border=0, n_fill=150, mode="same", mono=False,
          seed_noise=0.0, near_noise=0.01, rng_seed=None):
    fr = frame(orc, image_seed)
    rng = np.random.default_rng(1000 * image_seed + n_seed if rng_seed is None else rng_seed)
    kps, desc = fr["lk"], fr["ld"]
    n = len(kps)
    ru = np.full(NF, -1.0)
    ru[:n] = fr["right_u"][:n]
    dp = fr["depth"][:n]
    q = np.array([0.01, -0.02, 0.005, 1.0]); q /= np.linalg.norm(q)
    Rt, tt = quat_to_R(q), np.array([0.05, -0.02, 0.1])
    depth = np.where(dp > 0, dp, rng.uniform(4, 30, n))
    pc = np.stack([(kps["x"] - CX) / FX * depth, (kps["y"] - CY) / FY * depth, depth], 1)
    Xw = (pc - tt) @ Rt                                                   # Rt^T (pc - t)
    order = rng.permutation(n)
    far_ok = order[(kps["x"][order] >= 64 + 6 * SIGMA2[kps["octave"][order]] + 1)]     # the query stays inside the image
    far = far_ok[:n_far]
    rest = order[~np.isin(order, far)]
    take = lambda k: (rest[:k], rest[k:])
    seeds, rest = take(n_seed)
    bad_seeds, rest = take(3)
    near, rest = take(n_near)
    fill, rest = take(n_fill)
    dup = near[:n_dup]

    groups = []   # (frame feature, x, y, descriptor, position, good)

    def add(fs, x, y, d, pos, good):
        for k, f in enumerate(fs):
            groups.append((int(f), float(x[k]), float(y[k]), d[k], pos[k], good))

    jit = lambda fs, s: (kps["x"][fs] + rng.normal(0, s, len(fs)), kps["y"][fs] + rng.normal(0, s, len(fs)))
    off = lambda fs: Xw[fs] + rng.uniform(2.0, 5.0, (len(fs), 3)) * rng.choice([-1.0, 1.0], (len(fs), 3))
    add(seeds, *jit(seeds, 1.5), _flip(rng, desc[seeds], 6), Xw[seeds] + rng.normal(0, seed_noise, (len(seeds), 3)), 1)
    add(bad_seeds, *jit(bad_seeds, 1.5), _flip(rng, desc[bad_seeds], 6), Xw[bad_seeds], 0)
    add(near, *jit(near, 1.5), _flip(rng, desc[near], 6), off(near) if near_bad else Xw[near] + rng.normal(0, near_noise, (len(near), 3)), 1)
    add(dup, *jit(dup, 1.0), _flip(rng, desc[dup], 9), off(dup) if near_bad else Xw[dup] + rng.normal(0, near_noise, (len(dup), 3)), 1)
    col = np.floor(kps["x"][far] / 64.0) * 64.0
    add(far, col - 6.0 * SIGMA2[kps["octave"][far]], kps["y"][far], _flip(rng, desc[far], 6), off(far), 1)
    if n_border:
        ends = np.array([np.argmin(kps["x"]), np.argmax(kps["x"]), np.argmin(kps["y"]), np.argmax(kps["y"])])[np.arange(n_border) % 4]
        bx = np.where(np.arange(n_border) % 4 == 0, -5.0, np.where(np.arange(n_border) % 4 == 1, W + 3.0, kps["x"][ends]))
        by = np.where(np.arange(n_border) % 4 == 2, -4.0, np.where(np.arange(n_border) % 4 == 3, H + 2.0, kps["y"][ends]))
        add(ends, bx, by, _flip(rng, desc[ends], 4), Xw[ends] + rng.normal(0, near_noise, (len(ends), 3)), 1)
    half = len(fill) // 2
    add(fill[:half], *jit(fill[:half], 2.0), desc[fill[:half]], Xw[fill[:half]], 0)
    add(fill[half:], *jit(fill[half:], 2.0), rng.integers(0, 256, (len(fill) - half, 32)).astype(np.uint8), Xw[fill[half:]], 1)

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
    held = np.full(NF, -1, np.int32)
    inv = np.empty(m, np.int64); inv[perm] = np.arange(m)
    for k in range(n_seed + 3):                                           # the seeds and the bad seeds are the first groups
        held[groups[inv[k]][0]] = inv[k]
    # the keyframe looks along the frame's axis from in front of it, behind it, or from beside it: tlc.z ~ +1, -1, 0.1 against a baseline of 0.54
    dz = {"up": 1.0, "down": -1.0, "same": 0.1}[mode]
    q0 = q + np.array([0.002, -0.001, 0.0015, 0.0]); q0 /= np.linalg.norm(q0)
    t0 = tt + np.array([0.03, -0.02, 0.04])
    return dict(image_seed=image_seed, kps=kps, desc=desc, n_kp=n, right_u=None if mono else ru, kf_kps=kf_kps, kf_desc=kf_desc, good=good, pos=pos,
                src=src, kf_Rcw=Rt.astype(np.float32).reshape(9), kf_tcw=(tt + np.array([0.0, 0.0, dz])).astype(np.float32), held=held,
                Rcw=quat_to_R(q0).astype(np.float32).reshape(9), tcw=t0.astype(np.float32), cam=CAM, bounds=BOUNDS, baseline=BASELINE,
                sigma2=SIGMA2, inv_sigma2=INV_SIGMA2, mode=mode)


# the free-running scenes, one per verdict (tests/test_reloc_refine_host.py asserts that the restatement reaches it with every count at least
# 3 away from 10 and 50), and the boundary scenes: noise-free seeds and nothing else to find
VERDICT_SCENES = {
    "REJECT_1": dict(image_seed=3, n_seed=5, n_near=40),
    "ACCEPT_1": dict(image_seed=3, n_seed=100, n_near=40, seed_noise=0.01),
    "REJECT_2": dict(image_seed=8, n_seed=30, n_near=10, mode="up"),
    "ACCEPT_2": dict(image_seed=8, n_seed=30, n_near=400, n_dup=25, n_border=8, mode="up"),
    "REJECT_3": dict(image_seed=11, n_seed=34, n_far=20, mode="same"),
    "ACCEPT_3": dict(image_seed=11, n_seed=40, n_near=14, near_bad=True, mode="down"),
}
# (10 seeds go on to a search that finds next to nothing; 49 seeds go on to one whose few finds -- the seeds' own features at a neighbouring
# octave -- carry them over 50)
BOUNDARY_SCENES = {9: "REJECT_1", 10: "REJECT_2", 49: "ACCEPT_2", 50: "ACCEPT_1"}


def boundary(orc, n_seed):
    return build(orc, image_seed=3, n_seed=n_seed, n_fill=60, rng_seed=4242)


_restated = {}


def restated(orc, name):
    """(scene, the restatement's result) of a named scene -- a key of VERDICT_SCENES or a seed count of BOUNDARY_SCENES -- computed once,
    shared by the tests and left unchanged"""
    import reloc_refine_restatement as rr
    if name not in _restated:
        s = boundary(orc, name) if isinstance(name, int) else build(orc, **VERDICT_SCENES[name])
        _restated[name] = (s, rr.refine(orc, s))
    return _restated[name]
