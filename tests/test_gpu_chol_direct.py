"""The batch Cholesky's four factorisation families, each launched directly (api.chol_solve_debug / ptz_debug_chol_solve) on dense
systems at the edges of its 16-row blocks and 64-row tiles, against the exact solve of chol_util.

Paths: 1 chol_chain_kernel (one launch), 2 chol_col_step_kernel (one launch per step), 3 right-looking panel + syrk,
4 left-looking chol_update_col_h_kernel + panel (the loop of chol_factor_solve_profiled).  Paths 1 and 2 make the diagonal
tiles' inverses inside the sweep, 3 and 4 by chol_tile_inverse_kernel afterwards.  Every call is poisoned (Ldiag, Dinv, Linv and x
start as 0xFF bytes) unless the test is about the difference.

Bounds (chol_util): eta_s <= 1e-13 and fwd <= 1e-13 kappa_s on the Jacobi-scaled system -- test_chol_solve_vs_numpy's own
1e-13 / 1e-9 at kappa 1e4, made to scale.  They are not fitted to what the device returns.

Measured on one MI355X (largest value per family; LAPACK = numpy.linalg.solve on the same matrices; the families' figures differ
only where paths 3 and 4 also ran a batch of 9 -- a system's bits are the same on all four):

    spectrum            eta_s chain / per-step   right- / left-looking   LAPACK     fwd / kappa_s, all four   LAPACK
    kappa 1             1.9e-16                  1.9e-16                 2.2e-16    3.8e-16                   4.3e-16
    kappa 1e4           1.6e-16                  2.0e-16                 9.5e-17    4.1e-17                   2.3e-17
    kappa 1e8           1.6e-16                  1.7e-16                 5.6e-17    6.4e-18                   1.3e-17
    kappa 1e12          1.0e-16                  1.9e-16                 6.2e-17    3.2e-18                   9.2e-18
    kappa 1e4 scaled    9.0e-17                  1.2e-16                 4.6e-16    1.1e-17                   4.6e-17
    kappa 1e8 scaled    1.2e-16                  1.5e-16                 2.6e-16    4.6e-18                   1.4e-17
    reduced camera system (kappa_s 1.3e4 .. 1.7e8 at r = 1e4 .. 1e8; not positive definite at r = 1e12: fail = 1 on every path)
                        1.9e-16                  1.9e-16                 2.7e-13    3.0e-17                   5.9e-15

eta_s does not grow with kappa_s (the explicit tile inverses of the back-substitution cost nothing measurable), so eta_s <= 1e-13
is asserted on every rung of the ladder; the realistic systems lie inside it.  No family departed from the others in any bit.

Not covered here: tile masks, step schedules, xperm, the two-workgroup back-substitution and compacted launches (they need the
planner of ptz_ba_batch_create; the bundle-adjustment bit-equality tests hold them), and the LIST = false back-substitution,
taken only above ~150 KiB of work list -- an order no quick test reaches."""
import numpy as np
import pytest

import chol_util as cu

pytestmark = pytest.mark.gpu

PATHS = [1, 2, 3, 4]
PATH_NAME = {1: "chain", 2: "per-step", 3: "right-looking", 4: "left-looking"}
path_param = pytest.mark.parametrize("path", PATHS, ids=[PATH_NAME[p] for p in PATHS])


def _solve(pkg, As, bs, path, poison=True, **kw):
    return pkg.api.chol_solve_debug(As, bs, path=path, poison=poison, **kw)


def _counts(path):
    return (2, 9) if path in (3, 4) else (2,)


def _check_measured(pkg, path, tag, n, kappa, scaled):
    """count systems of one kind in one call: no failure, eta_s of every system, fwd of the two with an exact solution."""
    for count in _counts(path):
        sysm = [cu.case(n, kappa, scaled, s) if s < 2 else None for s in range(count)]
        mats = [(c["A"], c["b"]) if c else cu.make_spd(n, kappa, s, scaled) for s, c in enumerate(sysm)]
        x, fail = _solve(pkg, [m[0] for m in mats], [m[1] for m in mats], path)
        assert not fail.any(), (tag, n, count, fail)
        for s in range(count):
            c = sysm[s]
            star = c["x_star"] if c else x[s].astype(cu.LD)
            eta, fwd, ks = cu.measures(mats[s][0], mats[s][1], x[s], star, c["jac"] if c else None)
            print("CHOLSTAT %s %s n=%d count=%d sys=%d eta_s=%.3e fwd_over_kappa=%.3e kappa_s=%.3e" %
                  (PATH_NAME[path], tag, n, count, s, eta, fwd / ks if c else -1.0, ks))
            assert np.isfinite(x[s]).all(), (tag, n, count, s)
            assert eta <= cu.ETA_BOUND, (tag, n, count, s, eta)
            if c:
                assert fwd <= cu.FWD_BOUND * ks, (tag, n, count, s, fwd, ks)


@path_param
@pytest.mark.parametrize("n", cu.ORDERS)
def test_orders_at_block_and_tile_edges(pkg, path, n):
    """kappa 1e4 at every edge of a 16-block and a 64-tile, on both sides of the right-hand-side row (row n of the padded matrix)."""
    _check_measured(pkg, path, "k1e4", n, 1e4, False)


@path_param
@pytest.mark.parametrize("n", cu.LADDER_ORDERS)
@pytest.mark.parametrize("rung", [r for r in cu.LADDER if r[0] != "k1e4"], ids=lambda r: r[0])
def test_spectrum_ladder(pkg, path, n, rung):
    _check_measured(pkg, path, rung[0], n, rung[1], rung[2])


_REAL = {}


def _realistic(pkg, orc, ftype, radius):
    key = (ftype, radius)
    if key not in _REAL:
        S, rhs = cu.reduced_camera_system(orc, pkg.synth.make_scene(1, 20, 100, factor_type=ftype), radius)
        _, bad = cu.ld_cholesky(S)
        _REAL[key] = dict(A=S, b=rhs, pd=bad < 0, jac=cu.jacobi(S) if bad < 0 else None,
                          x_star=cu.mp_to_ld(cu.exact_solve(S, rhs)) if bad < 0 else None)
    return _REAL[key]


@path_param
@pytest.mark.parametrize("ftype", [0, 1])
@pytest.mark.parametrize("radius", [1e4, 1e8, 1e12])
def test_reduced_camera_system(pkg, orc, path, ftype, radius):
    """The system the solver exists for: 20 views x 100, one LM step's damped reduced camera system at trust-region radius r,
    formed in long double and rounded.  Where it is not positive definite in long double the solve must say so."""
    c = _realistic(pkg, orc, ftype, radius)
    x, fail = _solve(pkg, [c["A"]], [c["b"]], path)
    if not c["pd"]:
        print("CHOLSTAT %s real_f%d_r%g n=%d not positive definite in long double, fail=%d" % (PATH_NAME[path], ftype, radius, len(c["b"]), fail[0]))
        assert fail[0] == 1
        return
    eta, fwd, ks = cu.measures(c["A"], c["b"], x[0], c["x_star"], c["jac"])
    xl = np.linalg.solve(c["A"], c["b"])
    eta_l, fwd_l, _ = cu.measures(c["A"], c["b"], xl, c["x_star"], c["jac"])
    print("CHOLSTAT %s real_f%d_r%g n=%d count=1 sys=0 eta_s=%.3e fwd_over_kappa=%.3e kappa_s=%.3e lapack_eta_s=%.3e lapack_fwd_over_kappa=%.3e" %
          (PATH_NAME[path], ftype, radius, len(c["b"]), eta, fwd / ks, ks, eta_l, fwd_l / ks))
    assert fail[0] == 0
    assert eta <= cu.ETA_BOUND, eta
    assert fwd <= cu.FWD_BOUND * ks, (fwd, ks)


# ---- bits ------------------------------------------------------------------------------------------------------------------
RAGGED = [1, 17, 64, 65, 193, 33, 128]
_SOLO = {}


def _ragged_system(n):
    return cu.make_spd(n, 1e4, 11)


def _solo_bits(pkg, path, key, A, b):
    """x of the system solved alone on `path`, once per process."""
    if (path, key) not in _SOLO:
        x, fail = _solve(pkg, [A], [b], path)
        assert fail[0] == 0, (path, key)
        _SOLO[(path, key)] = x[0]
    return _SOLO[(path, key)]


def _same(a, b):
    return np.array_equal(cu.bits(a), cu.bits(b))


@path_param
def test_ragged_batch_has_the_bits_of_each_system_alone(pkg, path):
    """Seven orders in one call, np from the largest (whole padding tiles of identity behind the small ones), forwards, backwards,
    and with every other system switched off: a skipped system's x and fail come back untouched."""
    sysm = [_ragged_system(n) for n in RAGGED]
    solo = [_solo_bits(pkg, path, ("ragged", n), *sysm[i]) for i, n in enumerate(RAGGED)]
    for order in (list(range(7)), list(range(6, -1, -1))):
        x, fail = _solve(pkg, [sysm[i][0] for i in order], [sysm[i][1] for i in order], path)
        assert not fail.any(), fail
        for pos, i in enumerate(order):
            assert _same(x[pos], solo[i]), (RAGGED[i], pos, np.abs(x[pos] - solo[i]).max())
    active = [1, 0, 1, 0, 1, 0, 1]
    x0 = [np.full(n, 123.5) for n in RAGGED]
    x, fail = _solve(pkg, [s[0] for s in sysm], [s[1] for s in sysm], path, active=active, x0=x0, fail0=[7] * 7)
    for i, n in enumerate(RAGGED):
        if active[i]:
            assert fail[i] == 0 and _same(x[i], solo[i]), (n, fail[i])
        else:
            assert fail[i] == 7 and _same(x[i], x0[i]), (n, fail[i], x[i][:4])


def _bits_target():
    return cu.make_spd(193, 1e4, 0)


@path_param
def test_bits_do_not_depend_on_company_position_poison_or_repetition(pkg, path):
    A, b = _bits_target()
    ref = _solo_bits(pkg, path, "target193", A, b)
    for poison in (False, True, True):  # (the second poisoned call is the repeated one)
        x, fail = _solve(pkg, [A], [b], path, poison=poison)
        assert fail[0] == 0 and _same(x[0], ref), poison
    # the one-launch chain holds at most 32 systems (33 is PTZ_EINVAL, test_arguments): its largest batch is 32
    for count in (2, 7, 9, 32 if path == 1 else 33):
        at = sorted({0, count // 2, count - 1})
        mats = [(A, b) if i in at else cu.make_spd(193, 1e4, 100 + i) for i in range(count)]
        for poison in (True, False):
            x, fail = _solve(pkg, [m[0] for m in mats], [m[1] for m in mats], path, poison=poison)
            assert not fail.any(), (count, fail)
            for i in at:
                assert _same(x[i], ref), (count, i, poison, np.abs(x[i] - ref).max())


def test_all_four_families_return_the_same_bits(pkg):
    """What test_ba_one_launch_factorisation_has_the_bits_of_the_per_step_launches and
    test_ba_large_batch_matches_single_across_cholesky_variants claim through whole LM solves, on dense systems."""
    cases = [("target193", _bits_target())] + [(("ragged", n), _ragged_system(n)) for n in RAGGED]
    cases += [(("k1e8s", n), (cu.case(n, 1e8, True, 0)["A"], cu.case(n, 1e8, True, 0)["b"])) for n in cu.LADDER_ORDERS]
    report = []
    for key, (A, b) in cases:
        xs = {p: _solo_bits(pkg, p, key, A, b) for p in PATHS}
        if not all(_same(xs[p], xs[1]) for p in PATHS):
            star = cu.mp_to_ld(cu.exact_solve(A, b))
            report.append((key, {PATH_NAME[p]: (int((cu.bits(xs[p]) != cu.bits(xs[1])).sum()), cu.ulp_distance(xs[p], star)) for p in PATHS}))
    assert not report, "per family (values that differ from the chain's, largest distance from x* in ulp): %r" % (report,)


@path_param
def test_only_the_lower_triangle_is_read(pkg, path):
    for n in (65, 193):
        A, b = cu.make_spd(n, 1e4, 5)
        An = A.copy()
        An[np.triu_indices(n, 1)] = np.nan
        x, fail = _solve(pkg, [An, A], [b, b], path)
        assert not fail.any(), (n, fail)
        assert np.isfinite(x[0]).all() and _same(x[0], x[1]), n


# ---- failure ---------------------------------------------------------------------------------------------------------------
def _among_healthy(pkg, path, A_bad, b_bad, expect):
    """The bad system alone, then in the middle of a batch of healthy ones (7; 9 on the many-system paths), then a healthy call.
    expect(x, fail) judges the bad system; the healthy ones must not notice it."""
    n = cu.FAIL_ORDER
    count = 9 if path in (3, 4) else 7
    healthy = [cu.make_spd(n, 1e4, 40 + i) for i in range(count)]
    solo = [_solo_bits(pkg, path, ("healthy130", i), *healthy[i]) for i in range(count)]
    x, fail = _solve(pkg, [A_bad], [b_bad], path)
    expect(x[0], fail[0], "alone")
    mid = count // 2
    mats = [(A_bad, b_bad) if i == mid else healthy[i] for i in range(count)]
    x, fail = _solve(pkg, [m[0] for m in mats], [m[1] for m in mats], path)
    expect(x[mid], fail[mid], "in a batch")
    for i in range(count):
        if i != mid:
            assert fail[i] == 0 and _same(x[i], solo[i]), (i, fail[i])
    x, fail = _solve(pkg, [healthy[0][0]], [healthy[0][1]], path)
    assert fail[0] == 0 and _same(x[0], solo[0])


def _must_fail(x, fail, where):
    assert fail == 1, (where, fail)


@path_param
@pytest.mark.parametrize("p", cu.FAIL_PIVOTS)
def test_negative_pivot_is_reported(pkg, path, p):
    _among_healthy(pkg, path, *cu.make_indefinite(cu.FAIL_ORDER, p), _must_fail)


@path_param
@pytest.mark.parametrize("p", cu.FAIL_PIVOTS)
def test_exact_zero_pivot_is_reported(pkg, path, p):
    _among_healthy(pkg, path, *cu.make_zero_pivot(cu.FAIL_ORDER, p), _must_fail)


@path_param
@pytest.mark.parametrize("what", ["nan", "inf"])
def test_non_finite_matrix_entry_is_reported(pkg, path, what):
    A, b = cu.make_spd(cu.FAIL_ORDER, 1e4, 3)
    A[100, 20] = A[20, 100] = np.nan if what == "nan" else np.inf
    _among_healthy(pkg, path, A, b, _must_fail)


@path_param
@pytest.mark.parametrize("what", ["nan", "inf"])
def test_non_finite_right_hand_side_never_passes_quietly(pkg, path, what):
    """The two sweeps differ here by design.  The DPP sweep (paths 1 and 2) compares the last reciprocal root of every 16-block,
    the right-hand-side row's and the padding's included: a non-finite rhs fails the solve.  The read-lane sweep (paths 3 and 4)
    looks at the pivots of rows < n only: fail stays 0 and the NaN / Inf comes back in x."""
    A, b = cu.make_spd(cu.FAIL_ORDER, 1e4, 3)
    b = b.copy()
    b[70] = np.nan if what == "nan" else np.inf

    def never_quietly(x, fail, where):
        print("CHOLRHS %s %s rhs %s: fail=%d, x finite: %s" % (PATH_NAME[path], what, where, fail, bool(np.isfinite(x).all())))
        assert fail == 1 or not np.isfinite(x).all(), (where, fail)

    _among_healthy(pkg, path, A, b, never_quietly)


# ---- arguments -------------------------------------------------------------------------------------------------------------
def test_arguments(pkg):
    api = pkg.api
    A, b = cu.make_spd(5, 1.0, 0)

    def einval(call):
        with pytest.raises(api.PtzError) as e:
            call()
        assert e.value.code == -1, e.value

    for path in [0] + PATHS:
        einval(lambda: api.chol_solve_debug([], [], path=path))
        einval(lambda: api.chol_solve_debug([A, np.zeros((0, 0))], [b, np.zeros(0)], path=path))
        einval(lambda: api.chol_solve_debug([A], [b], path=path, ld=4))
    einval(lambda: api.chol_solve_debug([A], [b], path=-1))
    einval(lambda: api.chol_solve_debug([A], [b], path=5))
    einval(lambda: api.chol_solve_debug([A] * 33, [b] * 33, path=1))
    x, fail = api.chol_solve_debug([A] * 32, [b] * 32, path=1, poison=True)
    assert not fail.any() and all(_same(v, x[0]) for v in x)
    x0, fail0 = api.chol_solve_debug([A], [b], path=0, poison=True)  # path 0: what chol_factor_solve chooses -- the chain here
    assert fail0[0] == 0 and _same(x0[0], x[0])
