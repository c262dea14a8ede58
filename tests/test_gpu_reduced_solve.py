"""The four reduced-system solvers of the local BA, each alone (orbfe_debug_reduced_solve: the production kernels through the production
launch code), against the backward error of LAPACK on the same systems (tests/reduced_system_cases.py):

    solver 0  k_lm_chol                              registers, one workgroup         1..42 block rows
    solver 1  k_lmb_step / k_lmb_back_mw             48x48 tiles, fp64 matrix cores   43..1000
    solver 2  k_lba_chol_solve                       LDS, one workgroup               1..100
    solver 3  k_lba_chol_panel / _trail / _back      panel in global memory           >= 101

eta_device <= 8 * max(eta_reference over the table) at every size where a solver changes its path; only the lower triangle is read;
two runs give the same bits; a bad pivot gives ok = 0 and x = 0 and the next solve on the same context is good again; refusals."""
import numpy as np
import pytest

import reduced_system_cases as rc

pytestmark = pytest.mark.gpu

NAMES = ("registers", "blocked", "LDS", "panel")
ONE_SIZE = (42, 50, 100, 101)          # the size each solver is run at where one size is enough


@pytest.fixture(scope="module")
def ctx():
    from orb_slam2_ros2_amd._lib import Context
    c = Context(640, 480, n_features=500, max_images=1)
    yield c
    c.close()


def _solve_and_measure(ctx, solver, nb, cases):
    """every case through the solver: ok == 1, 6 nb entries, eta under the bound; returns (worst device eta, worst reference eta)"""
    worst_dev = worst_ref = 0.0
    for family, cond, scale in cases:
        S, b = rc.system(family, nb, cond, scale)
        x, ok = ctx.debug_reduced_solve(solver, S, b)
        assert ok == 1 and x.shape == (6 * nb,), (NAMES[solver], nb, family, cond, scale, ok)
        e = rc.eta(S, b, x)
        worst_dev, worst_ref = max(worst_dev, e), max(worst_ref, rc.reference_eta(family, nb, cond, scale))
        assert e <= rc.eta_bound(), (NAMES[solver], nb, family, cond, scale, e / rc.U, rc.eta_bound() / rc.U)
    return worst_dev, worst_ref


def _report(solver, what, dev, ref):
    print(f"solver {solver} ({NAMES[solver]}) {what}: eta device {dev / rc.U:.3f} u, reference {ref / rc.U:.3f} u, "
          f"bound {rc.eta_bound() / rc.U:.3f} u")


FULL = [(f, c, s) for f in rc.FAMILIES for c, s in rc.TABLE]
MID = [(f, 1e8, 1.0) for f in rc.FAMILIES]


@pytest.mark.parametrize("solver,sizes,full_at", [
    (0, range(1, 43), (1, 2, 30, 31, 42)),                 # 30 -> 31: threads start owning a second block (31 * 30 / 2 = 465 > 448)
    (1, (*range(43, 51), 56, 101, 150), (47, 48, 49)),     # 43..50: every residue of 6 nb mod 48, 48 -> 49 a seventh tile column; 56: 7 tiles exactly
    (2, (1, 2, 17, 43, 99, 100), (100,)),                  # 100: the limit, 62.4 KB of LDS
    (3, (101, 107, 171), (101,)),                          # 171: n = 1026, the 1024-thread row loops take a second trip
], ids=NAMES)
def test_backward_error_against_the_reference(ctx, solver, sizes, full_at):
    dev = ref = 0.0
    for nb in sizes:
        d, r = _solve_and_measure(ctx, solver, nb, MID)
        dev, ref = max(dev, d), max(ref, r)
    _report(solver, f"cond 1e8 at {len(list(sizes))} sizes", dev, ref)
    dev = ref = 0.0
    for nb in full_at:
        d, r = _solve_and_measure(ctx, solver, nb, FULL)
        dev, ref = max(dev, d), max(ref, r)
    _report(solver, f"full table at {tuple(full_at)}", dev, ref)


@pytest.mark.parametrize("solver", [1, 3], ids=["blocked", "panel"])
def test_a_system_past_the_staging_limit(ctx, solver):
    """242 block rows: the dense system is 16.9 MB, past the 16 MB the entry point stages in page-locked memory -- it goes up by direct
    copies instead (and, for the blocked solver, 31 tile columns with 36 padding rows)."""
    nb = 242
    assert (6 * nb) ** 2 * 8 > 16 << 20
    dev, ref = _solve_and_measure(ctx, solver, nb, [("jtj", 1e8, 1.0)])
    _report(solver, f"past the staging limit, {nb} block rows", dev, ref)


@pytest.mark.parametrize("solver", range(4), ids=NAMES)
def test_only_the_lower_triangle_is_read_and_two_runs_give_the_same_bits(ctx, solver):
    nb = ONE_SIZE[solver]
    for family in rc.FAMILIES:
        S, b = rc.system(family, nb, 1e8, 1.0)
        x, ok = ctx.debug_reduced_solve(solver, S, b)
        x2, ok2 = ctx.debug_reduced_solve(solver, S, b)
        xp, okp = ctx.debug_reduced_solve(solver, rc.poison_upper(S), b)
        assert ok == ok2 == okp == 1
        assert np.array_equal(x, x2), (NAMES[solver], family, np.abs(x - x2).max())          # fixed summation orders
        assert np.array_equal(x, xp), (NAMES[solver], family, np.isnan(xp).sum())            # NaN above the diagonal never arrives


@pytest.mark.parametrize("value", [-1.0, 0.0, np.nan, np.inf], ids=["minus_one", "zero", "nan", "inf"])
@pytest.mark.parametrize("solver", range(4), ids=NAMES)
def test_bad_pivot_is_reported_and_the_next_solve_is_good(ctx, solver, value):
    """The documented return path of a failed factorisation: status OK, ok = 0, x = 0 (the optimiser rejects the trial).  The blocked
    solver keeps its bad-pivot flag across launches and clears it in the first launch of the NEXT factorisation, so the good solve that
    follows on the same context is part of what is pinned."""
    nb = ONE_SIZE[solver]
    n = 6 * nb
    S, b = rc.system("jtj", nb, 1e2, 1.0)
    for p in (0, 5, 6, 6 * (nb // 2) + 3, n - 1):            # (n - 1, solver 1: the last tile, next to the padding rows)
        x, ok = ctx.debug_reduced_solve(solver, rc.with_pivot(S, p, value), b)
        assert ok == 0 and x.shape == (n,) and not x.any(), (NAMES[solver], p, value, ok, np.abs(x).max())
        x, ok = ctx.debug_reduced_solve(solver, S, b)
        assert ok == 1 and rc.eta(S, b, x) <= rc.eta_bound(), (NAMES[solver], p, value, ok, rc.eta(S, b, x) / rc.U)


@pytest.mark.parametrize("value", [-1.0, 0.0, np.nan, np.inf], ids=["minus_one", "zero", "nan", "inf"])
@pytest.mark.parametrize("nb", [48, 56])
def test_blocked_solver_bad_last_pivot_with_no_padding_row_behind_it(ctx, nb, value):
    """6 nb a multiple of 48: the last pivot of the system is the last pivot of the last tile, no padding row comes after it -- a pivot
    the factorisation lets through cannot be caught by a later one."""
    n = 6 * nb
    S, b = rc.system("jtj", nb, 1e2, 1.0)
    x, ok = ctx.debug_reduced_solve(1, rc.with_pivot(S, n - 1, value), b)
    assert ok == 0 and not x.any(), (nb, value, ok, np.isnan(x).sum())
    x, ok = ctx.debug_reduced_solve(1, S, b)
    assert ok == 1 and rc.eta(S, b, x) <= rc.eta_bound()


def test_refusals(ctx):
    from orb_slam2_ros2_amd._lib import OrbfeError, ptr
    S, b = rc.system("eig", 2, 1e2, 1.0)
    x, ok = np.zeros(12), np.zeros(1, np.int32)
    call = ctx.lib.orbfe_debug_reduced_solve
    EBADARG = 1
    # nb outside what production gives the solver (refused before anything is read: the arrays may be small)
    for solver, nb in [(-1, 2), (4, 2), (0, 0), (0, 43), (1, 42), (1, 1001), (2, 0), (2, 101), (3, 100), (3, 2), (0, -1), (3, -5)]:
        assert call(ctx.h, solver, nb, ptr(S), ptr(b), ptr(x), ptr(ok)) == EBADARG, (solver, nb)
    assert b"block rows" in ctx.lib.orbfe_last_error(ctx.h)
    with pytest.raises(OrbfeError):
        ctx.debug_reduced_solve(1, S, b)
    with pytest.raises(ValueError):
        ctx.debug_reduced_solve(0, S[:7, :7], b[:7])
    for args in [(None, ptr(b), ptr(x), ptr(ok)), (ptr(S), None, ptr(x), ptr(ok)), (ptr(S), ptr(b), None, ptr(ok)), (ptr(S), ptr(b), ptr(x), None)]:
        assert call(ctx.h, 0, 2, *args) == EBADARG
    assert call(None, 0, 2, ptr(S), ptr(b), ptr(x), ptr(ok)) == EBADARG
    # and the context is as good as before
    x, ok = ctx.debug_reduced_solve(0, S, b)
    assert ok == 1 and rc.eta(S, b, x) <= rc.eta_bound()
