"""The yardstick of test_gpu_reduced_solve.py, checked without a device (tests/reduced_system_cases.py): the reference's own backward
error on the case table, that the bound notices a solution wrong in its tenth digit, and the layout mirrors of the entry point's packers."""
import numpy as np
import pytest

import reduced_system_cases as rc


@pytest.mark.parametrize("nb", rc.BOUND_SIZES)
def test_reference_backward_error_stays_under_2u_on_the_table(nb):
    worst = 0.0
    for family in rc.FAMILIES:
        for cond, scale in rc.TABLE:
            S, b = rc.system(family, nb, cond, scale)
            assert np.array_equal(S, S.T) and np.isfinite(S).all()
            e = rc.reference_eta(family, nb, cond, scale)
            worst = max(worst, e)
            assert e < 2 * rc.U, (family, nb, cond, scale, e / rc.U)
    print(f"reference eta, n = {6 * nb}: worst {worst / rc.U:.3f} u")
    assert worst <= rc.reference_eta_max() and 0 < rc.eta_bound() < 16 * rc.U


def test_the_families_have_the_condition_and_scale_they_are_asked_for():
    for family in rc.FAMILIES:
        for cond in rc.CONDS:
            S, _ = rc.system(family, 7, cond, 1.0)
            ev = np.linalg.eigvalsh(S)
            assert ev[0] > 0 and 0.5 * cond < ev[-1] / ev[0] < 2 * cond, (family, cond, ev[-1] / ev[0])
            for scale in rc.SCALES:
                assert np.array_equal(rc.system(family, 7, cond, scale)[0], S * scale)
    # the second family has structure inside its 6x6 blocks (translation columns thirty times the rotation columns) and is sparse in blocks
    S, _ = rc.system("jtj", 20, 1e8, 1.0)
    d = np.diag(S).reshape(20, 6)
    assert np.median(d[:, 3:]) > 100 * np.median(d[:, :3])
    blocks = np.abs(S.reshape(20, 6, 20, 6)).max((1, 3))
    assert (blocks == 0).sum() > 200


@pytest.mark.parametrize("nb", rc.BOUND_SIZES)
def test_a_solution_wrong_in_its_tenth_digit_exceeds_the_bound(nb):
    for family in rc.FAMILIES:
        for cond, scale in rc.TABLE:
            S, b = rc.system(family, nb, cond, scale)
            x = rc.reference_solve(S, b)
            assert rc.eta(S, b, x) <= rc.eta_bound()
            k = int(np.abs(x).argmax())
            x[k] *= 1 + 1e-10
            assert rc.eta(S, b, x) > rc.eta_bound(), (family, nb, cond, scale, rc.eta(S, b, x) / rc.U)
    x[0] = np.nan
    assert not rc.eta(S, b, x) <= rc.eta_bound()          # a NaN in the solution fails the comparison, it does not pass it


@pytest.mark.parametrize("nb", [1, 2, 8, 9, 17])
def test_layout_mirrors_round_trip_from_the_lower_triangle_alone(nb):
    S, b = rc.system("eig", nb, 1e2, 1.0)
    P = rc.poison_upper(S)
    n = 6 * nb
    assert np.isnan(P).sum() == n * (n - 1) // 2 and np.array_equal(np.tril(P), np.tril(S))
    blk = rc.pack_blocks(P)
    assert blk.shape == (nb * (nb + 1) // 2, 6, 6) and np.array_equal(rc.unpack_blocks(blk), S)
    assert np.array_equal(blk[nb * (nb + 1) // 2 - 1], P[n - 6:, n - 6:], equal_nan=True)
    M = rc.pack_padded(P, b)
    ld = rc.big_ld(nb)
    assert ld % 48 == 0 and 0 <= ld - n < 48 and M.shape == (ld + 48, ld)
    S1, b1 = rc.unpack_padded(M, nb)
    assert np.array_equal(S1, S) and np.array_equal(b1, b)
    assert np.array_equal(np.diag(M[n:ld, n:ld]), np.ones(ld - n)) and np.isclose(np.abs(M[n:]).sum(), (ld - n) + np.abs(b).sum(), rtol=1e-12)
    flat = rc.pack_colmajor(P)
    assert flat[3 + 1 * n] == S[3, 1] and np.array_equal(rc.unpack_colmajor(flat), S)
    Q = rc.with_pivot(S, n - 1, -1.0)
    assert Q[n - 1, n - 1] == -1.0 and (Q != S).sum() == 1
