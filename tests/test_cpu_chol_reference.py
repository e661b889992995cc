"""The yardstick of the direct Cholesky tests, checked without a GPU: the exact solve of chol_util against mpmath's own LU at
60 digits, and the two error measures against LAPACK -- numpy.linalg.solve has to pass every matrix the GPU test measures with 64
times the GPU test's margin, which is the check that the inputs are passable at all."""
import numpy as np
import pytest

import chol_util as cu

LAPACK_MARGIN = 64.0


@pytest.mark.parametrize("n", [1, 17, 65])
def test_exact_solve_matches_mpmath_lu(n):
    """x* of the refinement (long-double Cholesky, mpmath residual) against mpmath.lu_solve at 60 digits over the whole ladder:
    1e-22 relative in the 2-norm.  (A float64 solve is right to 1e-16 kappa at best, long-double refinement to 1e-19 kappa.)"""
    import mpmath
    for name, kappa, scaled in cu.LADDER:
        A, b = cu.make_spd(n, kappa, 0, scaled)
        x = cu.exact_solve(A, b)
        with mpmath.workdps(60):
            ref = mpmath.lu_solve(mpmath.matrix(A.tolist()), mpmath.matrix(b.tolist()))
            err = mpmath.sqrt(mpmath.fsum((x[i] - ref[i]) ** 2 for i in range(n))) / mpmath.sqrt(mpmath.fsum(ref[i] ** 2 for i in range(n)))
        assert err <= mpmath.mpf("1e-22"), (name, n, mpmath.nstr(err, 3))


def test_exact_solve_reads_the_lower_triangle_only():
    A, b = cu.make_spd(17, 1e4, 0)
    An = A.copy()
    An[np.triu_indices(17, 1)] = np.nan
    assert [float(v) for v in cu.exact_solve(An, b)] == [float(v) for v in cu.exact_solve(A, b)]


def test_measures_of_an_exact_and_of_a_perturbed_solution():
    """eta_s and fwd are what their formulas say: ~ 0 for the rounded exact solution of a well-conditioned system, and a relative
    perturbation e of x in the scaled norm comes back as fwd = e."""
    c = cu.case(33, 1.0, False, 0)
    x = c["x_star"].astype(np.float64)
    eta, fwd, kappa = cu.measures(c["A"], c["b"], x, c["x_star"], c["jac"])
    assert eta < 2e-16 and fwd < 2e-16 and abs(kappa - 1.0) < 1e-12, (eta, fwd, kappa)
    eta, fwd, _ = cu.measures(c["A"], c["b"], x * (1 + 1e-6), c["x_star"], c["jac"])
    assert abs(fwd / 1e-6 - 1) < 1e-6 and abs(eta / 0.5e-6 - 1) < 1e-3, (eta, fwd)  # A = Q Q^T: ||r|| = e ||b||, denominator 2 ||b||


def test_lapack_passes_every_measured_case_with_64_times_the_margin():
    worst = {}
    for n, kappa, scaled in cu.measured_cases():
        for seed in (0, 1):
            c = cu.case(n, kappa, scaled, seed)
            x = np.linalg.solve(np.tril(c["A"]) + np.tril(c["A"], -1).T, c["b"])
            eta, fwd, ks = cu.measures(c["A"], c["b"], x, c["x_star"], c["jac"])
            key = "k%g%s" % (kappa, "_scaled" if scaled else "")
            w = worst.setdefault(key, [0.0, 0.0, 0.0])
            w[0], w[1], w[2] = max(w[0], eta), max(w[1], fwd / ks), max(w[2], ks)
            assert eta <= LAPACK_MARGIN * cu.ETA_BOUND, (n, kappa, scaled, seed, eta)
            assert fwd <= LAPACK_MARGIN * cu.FWD_BOUND * ks, (n, kappa, scaled, seed, fwd, ks)
    for key, w in worst.items():
        print("LAPACK %-12s max eta_s %.2e  max fwd/kappa_s %.2e  max kappa_s %.2e" % (key, *w))


def test_failure_inputs_fail_where_they_say():
    """The indefinite and the singular inputs of the GPU test: in long double pivot p is the first that is not positive, and the
    integer matrix's pivot p is exactly zero."""
    for p in cu.FAIL_PIVOTS:
        A, _ = cu.make_indefinite(cu.FAIL_ORDER, p)
        piv = cu.ld_pivots(A)
        assert len(piv) == p + 1 and piv[-1] < 0 and (piv[:-1] > 0).all(), (p, piv[-1])
        Z, _ = cu.make_zero_pivot(cu.FAIL_ORDER, p)
        assert np.array_equal(Z, np.round(Z)) and np.abs(Z).max() < 2 ** 20
        piv = cu.ld_pivots(Z)
        assert len(piv) == p + 1 and piv[-1] == 0 and (piv[:-1] > 0).all(), (p, piv[-1])
