"""Inputs, the exact solve and the error measures of the direct tests of the batch Cholesky (test_gpu_chol_direct.py,
test_cpu_chol_reference.py).

The "exact solve" is the solution of the float64 data as given, to more digits than any float64 algorithm delivers: a
long-double Cholesky (plain numpy loops, a preconditioner only) and iterative refinement whose residual b - A x is formed with
mpmath at 50 digits, x kept in mpmath, until the correction is below 1e-25 relative.  Refinement in long double alone leaves
about three digits of head room over LAPACK (1.8e-9 against 1.7e-6 at kappa 1e12), hence the mpmath residual.

Both error measures are taken in long double on the Jacobi-scaled system D A D, D = diag(A)^-1/2, the scaling under which
Cholesky's error bounds hold and which the solver's real systems get (Ceres' jacobi_scaling):
    eta_s = ||D r||_2 / (||D A D||_2 ||D^-1 x||_2 + ||D b||_2),   r = b - A x
    fwd   = ||D^-1 (x - x*)||_2 / ||D^-1 x*||_2
and kappa_s = cond_2(D A D).  The bounds are the project's own (test_chol_solve_vs_numpy: residual 1e-13, solution 1e-9 at
kappa 1e4), made to scale: eta_s <= ETA_BOUND, fwd <= FWD_BOUND * kappa_s."""
import numpy as np

LD = np.longdouble
ETA_BOUND = 1e-13
FWD_BOUND = 1e-13
LADDER = [("k1", 1.0, False), ("k1e4", 1e4, False), ("k1e8", 1e8, False), ("k1e12", 1e12, False),
          ("k1e4_scaled", 1e4, True), ("k1e8_scaled", 1e8, True)]


ORDERS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 449]  # at kappa 1e4
LADDER_ORDERS = [65, 193]


def measured_cases():
    """(n, kappa, scaled) of every generated matrix whose solution is measured: the orders at kappa 1e4, the ladder at two orders."""
    return [(n, 1e4, False) for n in ORDERS] + [(n, k, sc) for n in LADDER_ORDERS for _, k, sc in LADDER if (k, sc) != (1e4, False)]


_CASES = {}


def case(n, kappa, scaled, seed):
    """One measured system with its exact solution, made once per process: dict A, b, x_star (long double), jac."""
    key = (int(n), float(kappa), bool(scaled), int(seed))
    if key not in _CASES:
        A, b = make_spd(n, kappa, seed, scaled)
        _CASES[key] = dict(A=A, b=b, x_star=mp_to_ld(exact_solve(A, b)), jac=jacobi(A))
    return _CASES[key]


def make_spd(n, kappa, seed, scaled=False):
    """Q diag(logspace(0, log10 kappa)) Q^T, symmetric to the bit; scaled: rows and columns times 10^U(-3, 3) (pixels against
    radians).  Returns (A, b)."""
    rng = np.random.default_rng([int(seed), int(n), int(round(np.log10(kappa))), int(scaled)])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(0, np.log10(kappa), n)) @ Q.T
    A = 0.5 * (A + A.T)
    b = rng.standard_normal(n)
    if scaled:
        s = 10.0 ** rng.uniform(-3, 3, n)
        A = A * s[:, None] * s[None, :]  # (each product rounded once, the same for (i, j) and (j, i): still symmetric)
        A = np.tril(A) + np.tril(A, -1).T
        b = b * s
    return A, b


FAIL_ORDER = 130                             # three tiles
FAIL_PIVOTS = [0, 15, 16, 63, 64, 127, 129]  # both sides of a 16-block and of a 64-tile edge, first and last


def make_indefinite(n, p, seed=7):
    """SPD (kappa 100) except that A[p][p] is lowered by twice the p-th pivot of its long-double factorisation: pivot p comes out
    as minus what it was, the pivots before it are untouched.  Returns (A, b)."""
    A, b = make_spd(n, 1e2, seed)
    A[p, p] -= float(2 * ld_pivots(A)[p])
    return A, b


def make_zero_pivot(n, p, seed=7):
    """L0 L0^T of an integer lower-triangular L0 with entries in {-2..2} (one in seven below the diagonal non-zero, diagonal 1 or 2)
    and L0[p][p] = 0: every product and sum of its factorisation is exact in float64, so pivot p is exactly zero and none before it is.
    (1 / sqrt of 1 and of 4 is exact after the Newton steps, so the columns of L are the integers of L0.)  Returns (A, b)."""
    rng = np.random.default_rng([int(seed), int(n), int(p)])
    L0 = np.tril(rng.integers(-2, 3, (n, n)) * (rng.random((n, n)) < 1.0 / 7), -1).astype(np.float64)
    L0[np.diag_indices(n)] = rng.integers(1, 3, n)
    L0[p, p] = 0.0
    return L0 @ L0.T, rng.integers(-3, 4, n).astype(np.float64)


def ld_cholesky(A):
    """Lower Cholesky factor in long double and the index of the first pivot that is not positive (or -1).  The factor is
    complete only when that index is -1."""
    A = np.tril(np.asarray(A, dtype=LD))
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        col = A[j:, j] - L[j:, :j] @ L[j, :j]
        d = col[0]
        if not d > 0:
            return L, j
        L[j:, j] = col / np.sqrt(d)
    return L, -1


def ld_pivots(A):
    """The pivots d_j = A_jj - sum_k L_jk^2 of the long-double factorisation up to and including the first non-positive one."""
    A = np.tril(np.asarray(A, dtype=LD))
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    piv = []
    for j in range(n):
        col = A[j:, j] - L[j:, :j] @ L[j, :j]
        piv.append(col[0])
        if not col[0] > 0:
            break
        L[j:, j] = col / np.sqrt(col[0])
    return np.array(piv, dtype=LD)


def _ld_solve(L, r):
    n = L.shape[0]
    y = np.zeros(n, dtype=LD)
    for i in range(n):
        y[i] = (r[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def _to_ld(v):
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


def exact_solve(A, b, tol=1e-25, max_iter=40):
    """Solution of the float64 system as given (lower triangle of A), as a list of mpmath numbers at 50 digits."""
    import mpmath
    A = np.tril(np.asarray(A, dtype=np.float64))
    A = A + np.tril(A, -1).T
    b = np.asarray(b, dtype=np.float64)
    n = A.shape[0]
    L, bad = ld_cholesky(A)
    if bad >= 0:
        raise ValueError("not positive definite in long double (pivot %d)" % bad)
    with mpmath.workdps(50):
        Am = [[mpmath.mpf(float(v)) for v in row] for row in A]
        bm = [mpmath.mpf(float(v)) for v in b]
        x = [mpmath.mpf(0)] * n
        for _ in range(max_iter):
            r = [bm[i] - mpmath.fdot(Am[i], x) for i in range(n)]
            dx = _ld_solve(L, np.array([_to_ld(v) for v in r], dtype=LD))
            dxm = [mpmath.mpf(float(v)) + mpmath.mpf(float(v - LD(float(v)))) for v in dx]
            x = [a + c for a, c in zip(x, dxm)]
            nx = mpmath.sqrt(mpmath.fsum(v * v for v in x))
            nd = mpmath.sqrt(mpmath.fsum(v * v for v in dxm))
            if nd <= tol * nx:
                return x
    raise RuntimeError("refinement did not converge")


def mp_to_ld(x):
    return np.array([_to_ld(v) for v in x], dtype=LD)


def jacobi(A):
    """(d, S, norm2(S), cond2(S)) of the Jacobi-scaled S = D A D, D = diag(d) = diag(A)^-1/2; S symmetric from the lower triangle."""
    A = np.tril(np.asarray(A, dtype=np.float64))
    A = A + np.tril(A, -1).T
    d = 1.0 / np.sqrt(np.diag(A))
    S = A * d[:, None] * d[None, :]
    ev = np.linalg.eigvalsh(0.5 * (S + S.T))
    return d, S, float(np.abs(ev).max()), float(np.abs(ev).max() / max(ev.min(), 1e-300))


def measures(A, b, x, x_star, jac=None):
    """(eta_s, fwd, kappa_s) of a computed float64 solution x against the exact one (long double array)."""
    d, S, nS, kappa = jacobi(A) if jac is None else jac
    Al = np.tril(np.asarray(A, dtype=LD))
    Al = Al + np.tril(Al, -1).T
    dl, xl, bl = d.astype(LD), np.asarray(x, dtype=LD), np.asarray(b, dtype=LD)
    r = bl - Al @ xl
    n2 = lambda v: float(np.sqrt((v * v).sum()))
    eta = n2(dl * r) / (nS * n2(xl / dl) + n2(dl * bl))
    fwd = n2((xl - x_star) / dl) / n2(x_star / dl)
    return eta, fwd, kappa


def reduced_camera_system(orc, scene, radius, min_diag=1e-6, max_diag=1e32):
    """The damped reduced camera system of one LM step at the scene's initial state, formed in long double from the oracle's
    linearisation: S = U + D_c^2 / r - sum_rays W (V + D_r^2 / r)^-1 W^T,  rhs = g_c - sum W (V + D_r^2 / r)^-1 g_r  (the step
    solves S dx = -rhs; the sign does not matter here), D^2 the diagonal of J^T J clamped to [min_diag, max_diag] as Ceres'
    Levenberg-Marquardt strategy does.  Returns (S, rhs) rounded to float64: the data the solver would be given."""
    lin = orc.ba_linearize(scene, scene.cam_init, scene.ray_init)
    U, V, W, g_c, g_r = (np.asarray(lin[k], dtype=LD) for k in ("U", "V", "W", "g_c", "g_r"))
    if scene.factor_type in (0, 1):  # the oracle keeps a dummy fy column (index 1, exactly zero) that the solver's block drops
        sel = [i for i in range(U.shape[1]) if i != 1]
        U, W, g_c = U[:, sel][:, :, sel], W[:, sel, :], g_c[:, sel]
    n_cam, nc = U.shape[0], U.shape[1]
    n = n_cam * nc
    S = np.zeros((n, n), dtype=LD)
    rhs = g_c.reshape(-1).copy()
    for c in range(n_cam):
        blk = U[c].copy()
        blk[np.diag_indices(nc)] += np.clip(np.diag(U[c]), min_diag, max_diag) / LD(radius)
        S[c * nc:(c + 1) * nc, c * nc:(c + 1) * nc] = blk
    obs_cam, obs_ray = np.asarray(scene.obs_cam), np.asarray(scene.obs_ray)
    for r in range(V.shape[0]):
        Vd = V[r].copy()
        Vd[np.diag_indices(Vd.shape[0])] += np.clip(np.diag(V[r]), min_diag, max_diag) / LD(radius)
        Vi = np.asarray(_ld_inv(Vd), dtype=LD)
        obs = np.nonzero(obs_ray == r)[0]
        Wr = [(int(obs_cam[o]), W[o]) for o in obs]  # W[o]: [nc, 3], the block of observation o
        for ca, Wa in Wr:
            rhs[ca * nc:(ca + 1) * nc] -= Wa @ (Vi @ g_r[r])
            for cb, Wb in Wr:
                S[ca * nc:(ca + 1) * nc, cb * nc:(cb + 1) * nc] -= Wa @ Vi @ Wb.T
    S = 0.5 * (S + S.T)
    return S.astype(np.float64), rhs.astype(np.float64)


def _ld_inv(M):
    """Inverse of a small SPD matrix in long double (Cholesky)."""
    L, bad = ld_cholesky(M)
    if bad >= 0:
        raise ValueError("ray block not positive definite")
    n = M.shape[0]
    return np.stack([_ld_solve(L, np.eye(n, dtype=LD)[i]) for i in range(n)], axis=1)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def ulp_distance(x, x_star):
    """Largest distance of x from the exact solution in units of the last place of the exact solution's float64 rounding."""
    xs = np.asarray(x_star, dtype=LD)
    ref = xs.astype(np.float64)
    return float(np.max(np.abs(np.asarray(x, dtype=LD) - xs) / np.spacing(np.abs(ref)).astype(LD)))
