"""Reduced camera systems for the four Cholesky solvers of the local BA (orbfe_debug_reduced_solve), and the yardstick they are held to.

Two families of symmetric positive-definite matrices of nb 6x6 block rows:
  "eig"  a random orthogonal basis with eigenvalues log-spaced over `cond` (the largest is 1), times `scale`, symmetrised;
  "jtj"  J^T J + lambda I of a random sparse block Jacobian (3 x 6 blocks, two keyframes per row block, translation columns thirty times
         the rotation columns, fewer rows than unknowns): the shape of the real thing, 6x6 blocks with structure; lambda = |J^T J|_2 / cond.
`scale` is a power of two and multiplies exactly, so the systems of one (family, nb, cond) differ by their exponents only.

The case table: cond in {1e2, 1e8, 1e13} x scale in {1, 2^-60, 2^60} (a map in millimetres or kilometres), both families.

The measure is the normwise backward error  eta = |b - S x|_inf / (|S|_inf |x|_inf + |b|_inf), residual in np.longdouble.
The reference is LAPACK: scipy.linalg.cho_solve(np.linalg.cholesky(S)).  A backward-stable fp64 Cholesky solve has eta of the order of
u = 2^-53 whatever n, cond and scale are, and a legitimate second one (other elimination order, fused multiply-adds, a pivot 1 / sqrt(d)
good to an ulp) stays within a small factor of it.  The bound on a device solver is therefore

    eta_device <= 8 * max(eta_reference over the table)

with the maximum taken over the whole table (both families) at n = 6, 258 and 606 -- the sizes at which test_reduced_solve_host.py holds
the reference itself under 2 u -- and never per case: one case's reference eta can be accidentally tiny (at n = 6 it is a handful of
operations).  An indexing slip costs >= 2^40 of that, a missing correction term after the hardware reciprocal square root >= 2^20.
"""
import functools

import numpy as np

U = 2.0 ** -53
CONDS = (1e2, 1e8, 1e13)
SCALES = (1.0, 2.0 ** -60, 2.0 ** 60)
FAMILIES = ("eig", "jtj")
TABLE = tuple((c, s) for c in CONDS for s in SCALES)
BOUND_SIZES = (1, 43, 101)     # block rows: n = 6, 258, 606
BOUND_FACTOR = 8.0


def spd(rng, nb, cond, scale):
    """random orthogonal basis, eigenvalues log-spaced over cond (largest 1), times scale, symmetrised"""
    n = 6 * nb
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    q = q * np.sign(np.diag(r))                                   # (Haar: the sign convention of QR taken out)
    ev = np.logspace(0.0, -np.log10(cond), n)
    s = (q * ev) @ q.T
    return (s + s.T) * (0.5 * scale)


def spd_jtj(rng, nb, cond, scale):
    """J^T J + lambda I, J a sparse block Jacobian: 3 nb rows, row block k sees keyframes k % nb and a random other one"""
    n = 6 * nb
    col = np.array([1.0, 1.0, 1.0, 30.0, 30.0, 30.0])
    j = np.zeros((3 * nb, n))
    for k in range(nb):
        for kf in {k, int(rng.integers(0, nb))}:
            j[3 * k:3 * k + 3, 6 * kf:6 * kf + 6] = rng.standard_normal((3, 6)) * col
    h = j.T @ j
    lam = np.linalg.norm(h, 2) / cond
    s = h + lam * np.eye(n)
    return (s + s.T) * (0.5 * scale)


@functools.lru_cache(maxsize=None)
def _base(family, nb, cond):
    """(S at scale 1, x0): one per (family, nb, cond), never modified (the arrays are read-only)"""
    rng = np.random.default_rng([FAMILIES.index(family), nb, int(round(np.log10(cond)))])
    s = (spd if family == "eig" else spd_jtj)(rng, nb, cond, 1.0)
    x0 = rng.standard_normal(6 * nb)
    s.setflags(write=False), x0.setflags(write=False)
    return s, x0


def system(family, nb, cond, scale):
    """(S, b) with b = S x0, x0 standard normal: fresh arrays"""
    s1, x0 = _base(family, nb, cond)
    s = s1 * scale
    return s, s @ x0


def eta(S, b, x):
    """normwise backward error of x as a solution of S x = b; NaN if x is not finite"""
    Sl, bl, xl = (np.asarray(a, np.longdouble) for a in (S, b, x))
    r = bl - Sl @ xl
    den = np.abs(Sl).sum(1).max() * np.abs(xl).max() + np.abs(bl).max()
    return float(np.abs(r).max() / den)


def reference_solve(S, b):
    from scipy.linalg import cho_solve
    return cho_solve((np.linalg.cholesky(S), True), b)


def reference_eta(family, nb, cond, scale):
    S, b = system(family, nb, cond, scale)
    return eta(S, b, reference_solve(S, b))


@functools.lru_cache(maxsize=None)
def reference_eta_max():
    """the largest backward error of the reference over the table, both families, at BOUND_SIZES"""
    return max(reference_eta(f, nb, c, s) for f in FAMILIES for nb in BOUND_SIZES for c, s in TABLE)


def eta_bound():
    return BOUND_FACTOR * reference_eta_max()


# ---- the layouts orbfe_debug_reduced_solve packs the system into (Python mirrors of its packers), and what a solver may read of them ----
def poison_upper(S):
    """S with its strict upper triangle NaN: a solver that reads only i >= j returns the same bits"""
    P = np.array(S, np.float64)
    P[np.triu_indices(P.shape[0], 1)] = np.nan
    return P


def with_pivot(S, p, value):
    P = np.array(S, np.float64)
    P[p, p] = value
    return P


def big_ld(nb):
    return (6 * nb + 47) // 48 * 48


def pack_blocks(S):
    """solver 0: the 6x6 blocks (I, J), I >= J, whole and row-major, block (I, J) at I (I + 1) / 2 + J"""
    nb = S.shape[0] // 6
    out = np.empty((nb * (nb + 1) // 2, 6, 6))
    for i in range(nb):
        for j in range(i + 1):
            out[i * (i + 1) // 2 + j] = S[6 * i:6 * i + 6, 6 * j:6 * j + 6]
    return out


def unpack_blocks(blk):
    """the symmetric matrix from the entries i >= j of pack_blocks' layout"""
    nb = int(round((np.sqrt(8 * len(blk) + 1) - 1) / 2))
    S = np.zeros((6 * nb, 6 * nb))
    for i in range(nb):
        for j in range(i + 1):
            S[6 * i:6 * i + 6, 6 * j:6 * j + 6] = blk[i * (i + 1) // 2 + j]
    return _mirror_lower(S)


def pack_padded(S, rhs):
    """solver 1: (ld + 48) x ld row-major, ld = 6 nb rounded up to 48; the blocks (I, J), I >= J, whole; unit diagonal in the padding rows;
    the right-hand side in row ld; zero elsewhere"""
    n = S.shape[0]
    nb, ld = n // 6, big_ld(n // 6)
    M = np.zeros((ld + 48, ld))
    for i in range(nb):
        M[6 * i:6 * i + 6, :6 * i + 6] = S[6 * i:6 * i + 6, :6 * i + 6]
    M[np.arange(n, ld), np.arange(n, ld)] = 1.0
    M[ld, :n] = rhs
    return M


def unpack_padded(M, nb):
    n, ld = 6 * nb, M.shape[1]
    return _mirror_lower(M[:n, :n]), M[ld, :n].copy()


def pack_colmajor(S):
    """solvers 2 and 3: all of S, column-major (flat index r + c n)"""
    return np.asarray(S, np.float64).flatten(order="F")


def unpack_colmajor(flat):
    n = int(round(np.sqrt(flat.size)))
    return _mirror_lower(flat.reshape((n, n), order="F"))


def _mirror_lower(A):
    L = np.tril(np.where(np.tri(*A.shape, dtype=bool), A, 0.0))
    return L + np.tril(L, -1).T
