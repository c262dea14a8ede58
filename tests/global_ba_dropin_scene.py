"""The scene tests/cpp/test_global_ba_dropin.cpp reads, the graph Optimizer::globalOptimization must build from it (:946-1028), and the
reader of the program's output.  Eight keyframes and 48 map points of a trajectory problem, with what the function has to skip: a bad
keyframe (5), a keyframe that is not in vpKfs (6), a null in each vector, a bad map point (3), an observer that no longer exists; and
what it has to keep: a map point with no observation at all (10) and one whose only observer is the bad keyframe (11)."""
import os

import numpy as np

from orb_slam2_ros2_amd import ba_synth

N_KF, PER_KF, BAD_KF, ABSENT_KF, BAD_MP, BARE_MP, ORPHAN_MP, GHOST_MP = 8, 6, 5, 6, 3, 10, 11, 12
CAMERA = tuple(float(np.float32(v)) for v in (520.908620, 521.007327, 325.141442, 249.701764, 40.0))
INV_SIGMA2 = ((np.float32(1.0) / np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2).astype(np.float32)
DELTA_MONO, DELTA_STEREO = float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815)))


def f32(v):
    return "%.9g" % float(np.float32(v))


def scene(use_rk, iterations=10, stop=0):
    """-> (text, expected): expected = dict(kf_ids, fixed, poses, lm_index, points, edges per landmark as sorted tuples)"""
    pr = ba_synth.make_trajectory_problem(9, N_KF, PER_KF, loop=2)
    n_mp = pr["points"].shape[0]
    ek, ep = pr["edge_pose"].copy(), pr["edge_point"].copy()
    ek[ep == ORPHAN_MP] = BAD_KF                                               # seen by the bad keyframe only
    keep = ep != BARE_MP                                                       # no observation at all
    if not ((ek == BAD_KF) & keep).any() or not ((ek == ABSENT_KF) & keep).any():
        raise AssertionError("the scene lost a pattern")
    feats = [[] for _ in range(N_KF)]
    obs = [[] for _ in range(n_mp)]
    seen = set()
    for e in np.flatnonzero(keep):
        k, p = int(ek[e]), int(ep[e])
        if (k, p) in seen:                                                    # (a map point holds a keyframe once: Observations is a map)
            continue
        seen.add((k, p))
        octave = int(np.flatnonzero(INV_SIGMA2.astype(np.float64) == pr["info"][e])[0])
        ru = float(np.float32(pr["meas"][e, 2])) if pr["is_stereo"][e] else -1.0
        feats[k].append((float(np.float32(pr["meas"][e, 0])), float(np.float32(pr["meas"][e, 1])), octave, ru))
        obs[p].append((k, len(feats[k]) - 1))
    obs[GHOST_MP].append((-1, 0))
    lines = [f"{len(INV_SIGMA2)} " + " ".join(f32(v) for v in INV_SIGMA2), str(N_KF)]
    t = pr["poses"][:, 4:].astype(np.float32)
    for k in range(N_KF):
        lines.append(f"{k} {int(k == BAD_KF)} 1 0 0 0 1 0 0 0 1 " + " ".join(f32(v) for v in t[k]) + f" {len(feats[k])} " +
                     " ".join(f"{f32(x)} {f32(y)} {o} {r:.17g}" for x, y, o, r in feats[k]))       # (rightU is a double in the reference)
    pos = pr["points"].astype(np.float32)
    lines.append(str(n_mp))
    for p in range(n_mp):
        lines.append(f"{int(p == BAD_MP)} " + " ".join(f32(v) for v in pos[p]) + f" {len(obs[p])} " + " ".join(f"{k} {i}" for k, i in obs[p]))
    vp_kfs = [0, 1, 2, 3, -1, 4, 5, 7]
    vp_mps = [(p + 5) % n_mp for p in range(n_mp)]
    vp_mps.insert(7, -1)
    lines.append(f"{len(vp_kfs)} " + " ".join(map(str, vp_kfs)))
    lines.append(f"{len(vp_mps)} " + " ".join(map(str, vp_mps)))
    lines.append(f"{int(use_rk)} {iterations} {stop}")
    kf_ids = [k for k in vp_kfs if k >= 0 and k != BAD_KF]
    lm_index = [p for p in vp_mps if p >= 0 and p != BAD_MP]
    edges = {}
    for p in lm_index:
        rows = []
        for k, i in obs[p]:
            if k < 0 or k not in kf_ids:
                continue
            x, y, o, r = feats[k][i]
            st = r > 0
            rows.append((k, int(st), x, y, r if st else 0.0, float(INV_SIGMA2[o]), (DELTA_STEREO if st else DELTA_MONO) if use_rk else -1.0))
        edges[p] = sorted(rows)
    poses = np.zeros((len(kf_ids), 7))
    poses[:, 3] = 1.0
    poses[:, 4:] = t[kf_ids].astype(np.float64)
    return "\n".join(lines) + "\n", dict(kf_ids=kf_ids, fixed=[int(k == 0) for k in kf_ids], poses=poses, lm_index=lm_index,
                                         points=pos[lm_index].astype(np.float64), edges=edges, n_kf=N_KF, n_mp=n_mp)


def build_command(root, exe):
    pkg = os.path.join(root, "orb_slam2_ros2_amd")
    return ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(root, "tests", "cpp", "stubs"), "-I" + os.path.join(pkg, "host"),
            "-I" + os.path.join(root, "include"), "-o", exe, os.path.join(root, "tests", "cpp", "test_global_ba_dropin.cpp"), "-L" + pkg,
            "-lorbfe_hip", "-pthread", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"]


def _d(h):
    return float(np.array([int(h, 16)], np.uint64).view(np.float64)[0])


def _f(h):
    return float(np.array([int(h, 16)], np.uint32).view(np.float32)[0])


def parse(stdout):
    """-> dict(camera, kf_ids, fixed, poses, lm_index, points, problem arrays, gba = {kf id: 4x4 or None}, pgba = {mp index: 3 or None})"""
    cam, kf_ids, fixed, poses, lm_index, points, edges, gba, pgba = None, [], [], [], [], [], [], {}, {}
    for ln in stdout.splitlines():
        w = ln.split()
        if w[0] == "c":
            cam = tuple(_d(h) for h in w[1:])
        elif w[0] == "p":
            kf_ids.append(int(w[1])), fixed.append(int(w[2])), poses.append([_d(h) for h in w[3:]])
        elif w[0] == "l":
            lm_index.append(int(w[1])), points.append([_d(h) for h in w[2:]])
        elif w[0] == "e":
            edges.append((int(w[1]), int(w[2]), int(w[3])) + tuple(_d(h) for h in w[4:]))
        elif w[0] == "kf":
            gba[int(w[1])] = None if w[2] == "none" else np.array([_f(h) for h in w[2:]], np.float32).reshape(4, 4)
        elif w[0] == "mp":
            pgba[int(w[1])] = None if w[2] == "none" else np.array([_f(h) for h in w[2:]], np.float32)
    e = np.array(edges, np.float64).reshape(-1, 8)
    prob = dict(poses=np.array(poses).reshape(-1, 7), points=np.array(points).reshape(-1, 3), edge_pose=e[:, 0].astype(np.int32),
                edge_point=e[:, 1].astype(np.int32), is_stereo=e[:, 2].astype(np.uint8), meas=e[:, 3:6].copy(), info=e[:, 6].copy(),
                huber_delta=e[:, 7].copy(), fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3], bf=cam[4])
    return dict(camera=cam, kf_ids=kf_ids, fixed=fixed, lm_index=lm_index, problem=prob, gba=gba, pgba=pgba)
