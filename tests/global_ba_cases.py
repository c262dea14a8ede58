"""Block-CSR systems for the conjugate-gradient solver of the global BA (orbfe_debug_bsr_pcg), and the yardstick they are held to.

The matrices are J^T J + lambda I of a sparse block Jacobian in the style of reduced_system_cases.spd_jtj (translation columns thirty
times the rotation columns, fewer rows than unknowns, lambda = |J^T J|_2 / cond), with the block pattern chosen, not random:

  "one"     nb = 1
  "two"     nb = 2, no off-diagonal block
  "star"    nb = 70, block row 0 coupled to every other row (71 > 10 blocks: a row longer than any one pass of the SpMV wave) and a chain
  "band"    nb = 1100, a band of half-width 3 plus 5 far blocks: more block rows than a workgroup has threads, every partial-sum stage
            takes a second trip

cond in {1e2, 1e6} x scale in {1, 2^-60, 2^60}.  `scale` is a power of two and multiplies exactly; a PCG with a relative stopping rule is
scale-invariant to the bit, one with an absolute epsilon anywhere is not.

The measure is the true relative residual |b - S x|_2 / |b|_2 in np.longdouble at tol = 1e-10.  The reference is the restatement's PCG
(tests/global_ba_restatement.py).  The bound on the device is

    residual_device <= 8 * max(residual_restatement over the table)      and      iterations_device <= 1.25 * iterations_restatement

-- the factor and the "maximum over the whole table, never per case" rule of reduced_system_cases.py: the recursively updated residual
of one case can land accidentally far below tol.  Summation order perturbs at 1e-16; going from tol = 1e-10 to 1e-12 costs 13-30 %
iterations; a broken preconditioner costs multiples."""
import functools

import numpy as np

import global_ba_restatement as R

CONDS = (1e2, 1e6)
SCALES = (1.0, 2.0 ** -60, 2.0 ** 60)
SHAPES = ("one", "two", "star", "band")
TABLE = tuple((sh, c, s) for sh in SHAPES for c in CONDS for s in SCALES)
TOL = 1e-10
BOUND_FACTOR = 8.0
ITER_FACTOR = 1.25


def pattern(shape):
    """(nb, [(a, b, rows)]): row blocks of J seeing keyframes a and b (a == b: one keyframe) with `rows` rows"""
    if shape == "one":
        return 1, [(0, 0, 3)]
    if shape == "two":
        return 2, [(0, 0, 3), (1, 1, 3)]
    if shape == "star":
        return 70, [(k, k + 1, 3) for k in range(69)] + [(0, k, 1) for k in range(2, 70)]
    if shape == "band":
        nb = 1100
        pairs = [(k, k + 1, 3) for k in range(nb - 1)] + [(k, k + d, 1) for d in (2, 3) for k in range(nb - d)]
        return nb, pairs + [(7, 611, 1), (100, 1099, 1), (0, 550, 1), (333, 900, 1), (512, 1024, 1)]
    raise KeyError(shape)


@functools.lru_cache(maxsize=None)
def _base(shape, cond):
    """(row_off, col, blocks at scale 1, b at scale 1): one per (shape, cond), read-only"""
    nb, pairs = pattern(shape)
    rng = np.random.default_rng([SHAPES.index(shape), int(round(np.log10(cond)))])
    colw = np.array([1.0, 1.0, 1.0, 30.0, 30.0, 30.0])
    acc = {(i, i): np.zeros((6, 6)) for i in range(nb)}
    for a, b, rows in pairs:
        ja = rng.standard_normal((rows, 6)) * colw
        jb = rng.standard_normal((rows, 6)) * colw
        if a == b:
            acc[(a, a)] += ja.T @ ja
            continue
        acc[(a, a)] += ja.T @ ja
        acc[(b, b)] += jb.T @ jb
        acc.setdefault((a, b), np.zeros((6, 6)))
        acc.setdefault((b, a), np.zeros((6, 6)))
        acc[(a, b)] += ja.T @ jb
        acc[(b, a)] += jb.T @ ja
    keys = sorted(acc)
    row_off = np.zeros(nb + 1, np.int32)
    for i, _ in keys:
        row_off[i + 1] += 1
    row_off = np.cumsum(row_off).astype(np.int32)
    col = np.array([j for _, j in keys], np.int32)
    blocks = np.array([acc[k] for k in keys])
    # |J^T J|_2 by power iteration from a fixed start (the value only places lambda; 60 steps settle it to a per cent)
    v = np.ones(6 * nb) / np.sqrt(6 * nb)
    norm = 1.0
    for _ in range(60):
        w = R.bsr_matvec(row_off, col, blocks, v)
        norm = float(np.linalg.norm(w))
        v = w / norm
    lam = norm / cond
    rows_of = R.bsr_rows(row_off)
    blocks[rows_of == col] += lam * np.eye(6)
    tw = {k: q for q, k in enumerate(keys)}
    for q, (i, j) in enumerate(keys):                        # symmetric to the bit, as the Schur kernel leaves it
        if i > j:
            blocks[tw[(j, i)]] = blocks[q].T
        elif i == j:
            blocks[q] = np.tril(blocks[q]) + np.tril(blocks[q], -1).T
    x0 = rng.standard_normal(6 * nb)
    b = R.bsr_matvec(row_off, col, blocks, x0)
    for a in (row_off, col, blocks, b):
        a.setflags(write=False)
    return row_off, col, blocks, b


def system(shape, cond, scale):
    """(row_off, col, blocks, b): fresh value arrays"""
    row_off, col, blocks, b = _base(shape, cond)
    return row_off, col, blocks * scale, b * scale


@functools.lru_cache(maxsize=None)
def reference(shape, cond, scale):
    """(true residual, iterations, ok) of the restatement's PCG at TOL and the default cap"""
    row_off, col, blocks, b = system(shape, cond, scale)
    x, it, ok = R.pcg(row_off, col, blocks, b, TOL, 0)
    return R.true_residual(row_off, col, blocks, b, x), it, ok


@functools.lru_cache(maxsize=None)
def reference_residual_max():
    return max(reference(*c)[0] for c in TABLE)


def residual_bound():
    return BOUND_FACTOR * reference_residual_max()
