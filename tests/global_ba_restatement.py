"""numpy restatement of orbfe_ba_global_optimize's block-sparse path: the second yardstick besides the oracle.

  bsr_symbolic   the block-CSR structure of the reduced camera system (the rules of csrc/bsr_symbolic.h)
  reduced_bsr    the Schur complement S = Hpp + lambda I - Hpl (Hll + lambda I)^-1 Hpl^T and its right-hand side from the oracle's blocks
  pcg            block-Jacobi preconditioned conjugate gradient: x0 = 0, stop at r.M^-1 r <= tol^2 b.M^-1 b
  optimize       one SparseOptimizer::optimize(n) with OptimizationAlgorithmLevenberg (oracle/lba_oracle.cpp's loop) on that solver

Edge evaluation, the normal-equation blocks and the SE3 update are the oracle's."""
import numpy as np


def slots(n_poses, pose_fixed):
    fixed = np.zeros(n_poses, np.uint8) if pose_fixed is None else np.asarray(pose_fixed, np.uint8)
    slot = np.full(n_poses, -1, np.int64)
    free = np.flatnonzero(fixed == 0)
    slot[free] = np.arange(free.size)
    return slot, free


def bsr_symbolic(nf, n_points, edge_pose, edge_point, slot):
    """-> dict(row_off, col, twin, low, low_row, pair_off, pairs): both triangles, a row's columns ascending, the diagonal always there;
    the blocks with row >= col carry the pairs (e1, e2) -- pose(e1) = row, pose(e2) = col, same point -- points ascending, then e1, then
    e2, each in ascending edge order."""
    edge_pose, edge_point = np.asarray(edge_pose), np.asarray(edge_point)
    by_point = [[] for _ in range(n_points)]
    for e in range(edge_pose.size):
        by_point[edge_point[e]].append(e)
    lists = {(i, i): [] for i in range(nf)}
    for es in by_point:
        for e1 in es:
            i = slot[edge_pose[e1]]
            if i < 0:
                continue
            for e2 in es:
                j = slot[edge_pose[e2]]
                if j >= 0 and i >= j:
                    lists.setdefault((int(i), int(j)), []).append((e1, e2))
    lower = sorted(lists)
    full = sorted(set(lower) | {(j, i) for i, j in lower})
    index = {b: q for q, b in enumerate(full)}
    row_off = np.zeros(nf + 1, np.int32)
    for i, _ in full:
        row_off[i + 1] += 1
    row_off = np.cumsum(row_off).astype(np.int32)
    col = np.array([j for _, j in full], np.int32).reshape(-1)
    twin = np.array([index[(j, i)] for i, j in full], np.int32).reshape(-1)
    low = np.array([index[b] for b in lower], np.int32).reshape(-1)
    low_row = np.array([i for i, _ in lower], np.int32).reshape(-1)
    pair_off = np.cumsum([0] + [len(lists[b]) for b in lower]).astype(np.int32)
    pairs = np.array([pr for b in lower for pr in lists[b]], np.int32).reshape(-1, 2)
    return dict(row_off=row_off, col=col, twin=twin, low=low, low_row=low_row, pair_off=pair_off, pairs=pairs)


def _dinv(Hll, lam):
    return np.linalg.inv(Hll + lam * np.eye(3)[None]) if Hll.shape[0] else Hll.copy()


def reduced_bsr(sym, system, lam, edge_pose, edge_point, slot, free):
    """blocks (nnzb, 6, 6) and rhs (6 nf,) of the structure `sym` from the oracle's blocks `system` (ba_build_system)"""
    edge_pose, edge_point = np.asarray(edge_pose), np.asarray(edge_point)
    Hpp, bp, Hll, bl, Hpl = system["Hpp"], system["bp"], system["Hll"], system["bl"], system["Hpl"]
    nf = free.size
    Dinv = _dinv(Hll, lam)
    W = np.einsum("eak,ekc->eac", Hpl, Dinv[edge_point])                      # Hpl(e) Dinv(point(e)), 6x3
    blocks = np.zeros((sym["col"].size, 6, 6))
    for l, q in enumerate(sym["low"]):
        i, j = sym["low_row"][l], sym["col"][q]
        pr = sym["pairs"][sym["pair_off"][l]:sym["pair_off"][l + 1]]
        B = -np.einsum("pak,pck->ac", W[pr[:, 0]], Hpl[pr[:, 1]]) if len(pr) else np.zeros((6, 6))
        if i == j:
            B = B + Hpp[free[i]] + lam * np.eye(6)
            B = np.tril(B) + np.tril(B, -1).T
        blocks[q] = B
        blocks[sym["twin"][q]] = B.T
    rhs = bp[free].copy()
    on_free = slot[edge_pose] >= 0
    np.subtract.at(rhs, slot[edge_pose[on_free]], np.einsum("eak,ek->ea", W[on_free], bl[edge_point[on_free]]))
    return blocks, rhs.reshape(6 * nf)


def bsr_rows(row_off):
    return np.repeat(np.arange(row_off.size - 1), np.diff(row_off))


def bsr_matvec(row_off, col, blocks, x, dtype=np.float64):
    nb = row_off.size - 1
    prod = np.einsum("kab,kb->ka", blocks.astype(dtype), x.reshape(nb, 6).astype(dtype)[col])
    y = np.zeros((nb, 6), dtype)
    np.add.at(y, bsr_rows(row_off), prod)
    return y.reshape(-1)


def bsr_to_dense(row_off, col, blocks):
    nb = row_off.size - 1
    S = np.zeros((6 * nb, 6 * nb))
    for q, (i, j) in enumerate(zip(bsr_rows(row_off), col)):
        S[6 * i:6 * i + 6, 6 * j:6 * j + 6] = blocks[q]
    return S


def pcg(row_off, col, blocks, b, tol=1e-10, max_iter=0):
    """-> (x, iterations, ok).  ok = 0: a diagonal block that is not positive definite (x = 0), p.Sp not positive and finite, or no
    convergence within max_iter (default 4 * 6 * nb)."""
    nb = row_off.size - 1
    max_iter = max_iter if max_iter > 0 else 24 * nb
    blocks = np.asarray(blocks, np.float64).reshape(-1, 6, 6)
    rows = bsr_rows(row_off)
    diag = np.flatnonzero(rows == col)
    x = np.zeros(6 * nb)
    if diag.size != nb:
        return x, 0, 0
    D = blocks[diag]
    try:
        np.linalg.cholesky(D)
    except np.linalg.LinAlgError:
        return x, 0, 0
    if not np.isfinite(D).all():
        return x, 0, 0
    Minv = np.linalg.inv(D)
    prec = lambda r: np.einsum("kab,kb->ka", Minv, r.reshape(nb, 6)).reshape(-1)
    r = np.asarray(b, np.float64).copy()
    z = prec(r)
    p = z.copy()
    rz = rz0 = float(r @ z)
    if rz0 == 0:
        return x, 0, 1
    if not np.isfinite(rz0) or rz0 < 0:
        return x, 0, 0
    for it in range(max_iter):
        q = bsr_matvec(row_off, col, blocks, p)
        pq = float(p @ q)
        if not (pq > 0) or not np.isfinite(pq):
            return x, it, 0
        alpha = rz / pq
        x = x + alpha * p
        r = r - alpha * q
        z = prec(r)
        rz_new = float(r @ z)
        if not np.isfinite(rz_new):
            return x, it + 1, 0
        if rz_new <= tol * tol * rz0:
            return x, it + 1, 1
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, max_iter, 0


def true_residual(row_off, col, blocks, b, x):
    """||b - S x||_2 / ||b||_2 in np.longdouble"""
    L = np.longdouble
    r = np.asarray(b, L) - bsr_matvec(row_off, col, np.asarray(blocks).reshape(-1, 6, 6), np.asarray(x), L)
    return float(np.sqrt((r * r).sum()) / np.sqrt((np.asarray(b, L) ** 2).sum()))


def _robust_chi2(orc, pr, poses, points):
    e = orc.ba_eval_edges(poses, points, pr["edge_pose"], pr["edge_point"], pr["meas"], pr["is_stereo"], pr["info"], pr["huber_delta"],
                          pr["fx"], pr["fy"], pr["cx"], pr["cy"], pr["bf"])
    return float(e["rho"][:, 0].sum()), e["chi2"]


def optimize(orc, pr, pose_fixed, iterations, tol=1e-10, max_iter=0, exact=False):
    """-> dict(poses, points, chi2, iters, cg_stats = (trials, CG iterations, rejected by the solver)).  exact: a dense solve of the
    same system instead of the conjugate gradient."""
    ek, ep = np.asarray(pr["edge_pose"]), np.asarray(pr["edge_point"])
    poses, points = np.array(pr["poses"], np.float64), np.array(pr["points"], np.float64)
    nk, npt = poses.shape[0], points.shape[0]
    slot, free = slots(nk, pose_fixed)
    fixed = (slot < 0).astype(np.uint8)
    nf = free.size
    sym = bsr_symbolic(nf, npt, ek, ep, slot)
    on_free = slot[ek] >= 0
    lam, ni, done = 0.0, 2.0, 0
    trials = cg_total = rejected = 0
    for it in range(iterations if ek.size else 0):
        done += 1
        current_chi, _ = _robust_chi2(orc, pr, poses, points)
        sysm = orc.ba_build_system(poses, points, ek, ep, pr["meas"], pr["is_stereo"], pr["info"], pr["huber_delta"], pr["fx"], pr["fy"],
                                   pr["cx"], pr["cy"], pr["bf"], fixed)
        if it == 0:
            d = [np.abs(np.einsum("kaa->ka", sysm["Hpp"])).max(initial=0.0), np.abs(np.einsum("kaa->ka", sysm["Hll"])).max(initial=0.0)]
            lam, ni = 1e-5 * max(d), 2.0
        rho, qmax = 0.0, 0
        while True:
            backup = poses.copy(), points.copy()
            ok = True
            x = np.zeros(6 * nf)
            try:
                Dinv = _dinv(sysm["Hll"], lam)
            except np.linalg.LinAlgError:
                ok = False
            if ok and nf:
                blocks, rhs = reduced_bsr(sym, sysm, lam, ek, ep, slot, free)
                if exact:
                    try:
                        S = bsr_to_dense(sym["row_off"], sym["col"], blocks)
                        np.linalg.cholesky(S)
                        x = np.linalg.solve(S, rhs)
                    except np.linalg.LinAlgError:
                        ok = False
                else:
                    x, n_cg, good = pcg(sym["row_off"], sym["col"], blocks, rhs, tol, max_iter)
                    cg_total += n_cg
                    ok = bool(good)
            trials += 1
            dxp, dxl = np.zeros((nk, 6)), np.zeros((npt, 3))
            if ok:
                dxp[free] = x.reshape(nf, 6)
                r = sysm["bl"].copy()
                np.subtract.at(r, ep[on_free], np.einsum("eak,ea->ek", sysm["Hpl"][on_free], dxp[ek[on_free]]))
                dxl = np.einsum("pab,pb->pa", Dinv, r)
                for k in free:
                    out = orc.se3_oplus(poses[k], dxp[k])
                    poses[k] = -out if out[3] < 0 else out
                points = points + dxl
            else:
                rejected += 1
            temp_chi, _ = _robust_chi2(orc, pr, poses, points)
            if not ok:
                temp_chi = np.finfo(np.float64).max
            scale = float((dxp[free] * (lam * dxp[free] + sysm["bp"][free])).sum() + (dxl * (lam * dxl + sysm["bl"])).sum()) + 1e-3
            rho = (current_chi - temp_chi) / scale
            if rho > 0 and np.isfinite(temp_chi):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                current_chi = temp_chi
            else:
                lam *= ni
                ni *= 2
                poses, points = backup
                if not np.isfinite(lam):
                    break
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0 or not np.isfinite(lam):
            break
    _, chi2 = _robust_chi2(orc, pr, poses, points) if ek.size else (0.0, np.zeros(0))
    return dict(poses=poses, points=points, chi2=chi2, iters=done, cg_stats=(trials, cg_total, rejected))
