"""The reduced camera system of one LM step, written from its definition, and the scenes of the direct tests of the Schur kernels
(test_gpu_schur_direct.py, test_cpu_schur_reference.py).

Inputs: the UNSCALED blocks U, g_c, V, g_r, W of one linearisation (W per observation, [NC, 3]), the observation lists, Jacobi
scales s_c [n_cam, NC] and s_r [n_ray, 3], the trust-region radius r and the two clamps of the LM diagonal.

    U' = s_c U s_c,  W'_a = s_c W_a s_r,  V' = s_r V s_r,  g'_c = s_c g_c,  g'_r = s_r g_r
    D_c^2 = clamp(diag U') / r,  D_r^2 = clamp(diag V') / r,  E_j = (V'_j + D_r,j^2)^-1
    S_ii = U'_i + D_c,i^2 - sum_a W'_a E W'_a^T        (a: observations of camera i)
    S_ij = -sum W'_a E W'_b^T                          (a of camera i, b of camera j, on a common ray)
    b_i  = g'_c,i - sum_a W'_a E g'_r

(the signs of the k_schur comment and of test_cpu_schur_factored.py).  system() evaluates this in the dtype it is given -- long
double: the reference; float64 with numpy.linalg.inv: what plain double precision makes of the same formula -- and mp_system() at 50
digits.  None of the kernels' factorings is used: W'_a E W'_b^T is three matrix products per pair of observations.

Beside the system, in the same pass, the YARDSTICK, entrywise:
    Y_pq = |U'|_pq + D_c^2 + sum_rays kappa_j (|W'_a| |E_j| |W'_b|^T)_pq,      Yb_p = |g'_c|_p + sum kappa_j (|W'_a| |E_j| |g'_r|)_p
kappa_j = cond_2(V'_j + D_r,j^2).  For the normalised-ray factors V is singular along the ray, so E carries a component about r
times larger than the rest, which W annihilates; any double-precision inverse of that 3 x 3 block loses about kappa ulps there, and
a bound without kappa is one that float64 numpy itself cannot meet at r = 1e4.

The bound is  K * 2^-52 * Y  entrywise.  K is not taken from the kernels: it is 8 times the worst ratio |S_float64 - S_longdouble| / Y
(and the same for b) that float64 NUMPY reaches over all cases of the GPU test, rounded up to a power of two (the factored kernel
does about three times the roundings per term of the direct product -- k_ray_prep's folding, the row, the entry, the pair's
transforms in test_cpu_schur_factored.py -- and the worst of several hundred thousand entries sits a factor of a few above the
typical one).  test_cpu_schur_reference.py recomputes the ratio and holds K to it."""
import dataclasses

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
NUMPY_WORST_RATIO = 9.35  # float64 numpy's worst |S - S_ld| / Y over numeric_cases(), in units of 2^-52 (edges, PTZRayFxfyDist, r = 1e-2)
K = 128                   # 8 * NUMPY_WORST_RATIO = 74.8, rounded up to a power of two
MIN_DIAG, MAX_DIAG = 1e-6, 1e32  # the solver's default clamps (ptz_lm_options_default)
RADII = [1e-2, 1e4, 1e8]


# ---- the system -------------------------------------------------------------------------------------------------------------
def drop_dummy_fy(lin, ftype):
    """The oracle keeps an always-zero fy column (index 1) for PTZRay / PTZRayDist that the solver's block does not have."""
    U, g_c, W = lin["U"], lin["g_c"], lin["W"]
    if ftype in (0, 1) and U.shape[1] == (5 if ftype == 0 else 6):
        sel = [i for i in range(U.shape[1]) if i != 1]
        U, g_c, W = U[:, sel][:, :, sel], g_c[:, sel], W[:, sel, :]
    return dict(U=U, g_c=g_c, V=lin["V"], g_r=lin["g_r"], W=W)


def _inv3_sym(M):
    """Inverses of symmetric 3 x 3 blocks [m, 3, 3] by cofactors, in the blocks' dtype."""
    a, b, c, d, e, f = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
    det = a * c00 + b * c01 + c * c02
    E = np.empty_like(M)
    E[:, 0, 0], E[:, 0, 1], E[:, 0, 2] = c00, c01, c02
    E[:, 1, 0], E[:, 1, 1], E[:, 1, 2] = c01, c11, c12
    E[:, 2, 0], E[:, 2, 1], E[:, 2, 2] = c02, c12, c22
    return E / det[:, None, None]


def system(lin, obs_cam, obs_ray, s_c, s_r, radius, min_diag=MIN_DIAG, max_diag=MAX_DIAG, dtype=LD, drop=None, swap=None, no_lm=False):
    """S [n, n], b [n], the yardsticks Y [n, n], Yb [n], the clamped diagonal diag_c [n_cam, NC] and kappa [n_ray], all in `dtype`
    (kappa in float64).  dtype float64 inverts with numpy.linalg.inv, long double by cofactors.
    The three perturbations of the sensitivity test (the reference alone): drop = (a, b): observations a, b of one ray whose term
    is left out of S_ij (and of S_ji); swap = (i, j): the cameras' Jacobi scales change places in the blocks S_ij / S_ji; no_lm: E
    without the LM term, (V')^-1."""
    T = dtype
    U, g_c, V, g_r, W = (np.asarray(lin[k], dtype=T) for k in ("U", "g_c", "V", "g_r", "W"))
    obs_cam, obs_ray = np.asarray(obs_cam), np.asarray(obs_ray)
    s_c, s_r = np.asarray(s_c, dtype=T), np.asarray(s_r, dtype=T)
    n_cam, nc = U.shape[0], U.shape[1]
    n_ray = V.shape[0]
    n = n_cam * nc
    r = T(radius)
    Us = s_c[:, :, None] * U * s_c[:, None, :]
    Vs = s_r[:, :, None] * V * s_r[:, None, :]
    Ws = s_c[obs_cam][:, :, None] * W * s_r[obs_ray][:, None, :]
    gcs, grs = s_c * g_c, s_r * g_r
    i3, ic = np.arange(3), np.arange(nc)
    diag_c = np.clip(Us[:, ic, ic], T(min_diag), T(max_diag))
    Dc2 = diag_c / r
    Dr2 = np.clip(Vs[:, i3, i3], T(min_diag), T(max_diag)) / r
    M = Vs.copy()
    M[:, i3, i3] += Dr2
    kappa = np.linalg.cond(M.astype(np.float64))
    if no_lm:
        with np.errstate(all="ignore"):
            E = np.linalg.inv(Vs) if T is np.float64 else _inv3_sym(Vs)
    else:
        E = np.linalg.inv(M) if T is np.float64 else _inv3_sym(M)
    S = np.zeros((n, n), dtype=T)
    Y = np.zeros((n, n), dtype=T)
    b = gcs.reshape(-1).copy()
    Yb = np.abs(gcs).reshape(-1).copy()
    for c in range(n_cam):
        sl = slice(c * nc, (c + 1) * nc)
        S[sl, sl] = Us[c]
        S[sl, sl][ic, ic] += Dc2[c]
        Y[sl, sl] = np.abs(Us[c])
        Y[sl, sl][ic, ic] += Dc2[c]
    Ws_swapped = None
    if swap is not None:  # W' of the pair's two cameras with the OTHER camera's scales
        i, j = swap
        other = {i: j, j: i}
        Ws_swapped = {a: s_c[other[int(obs_cam[a])]][:, None] * W[a] * s_r[obs_ray[a]][None, :]
                      for a in np.nonzero((obs_cam == i) | (obs_cam == j))[0]}
    order = np.argsort(obs_ray, kind="stable")
    first = np.searchsorted(obs_ray[order], np.arange(n_ray + 1))
    cols = ic[None, :]
    with np.errstate(all="ignore") if no_lm else np.errstate():
        for j in range(n_ray):
            oa = order[first[j]:first[j + 1]]
            if len(oa) == 0:
                continue
            Wm, Ej = Ws[oa], E[j]                                     # [m, nc, 3], [3, 3]
            Tm = Wm @ Ej                                              # T_a = W'_a E
            blk = np.einsum("aik,bjk->aibj", Tm, Wm)                   # T_a W'_b^T
            aW = np.abs(Wm)
            yblk = T(kappa[j]) * np.einsum("aik,bjk->aibj", aW @ np.abs(Ej), aW)
            m = len(oa)
            if drop is not None and drop[0] in oa and drop[1] in oa:
                pa, pb = int(np.nonzero(oa == drop[0])[0][0]), int(np.nonzero(oa == drop[1])[0][0])
                blk[pa, :, pb, :] = 0
                blk[pb, :, pa, :] = 0
            if Ws_swapped is not None:
                cams = obs_cam[oa]
                for pa in np.nonzero(cams == swap[0])[0]:
                    for pb in np.nonzero(cams == swap[1])[0]:
                        v = (Ws_swapped[int(oa[pa])] @ Ej) @ Ws_swapped[int(oa[pb])].T
                        blk[pa, :, pb, :] = v
                        blk[pb, :, pa, :] = v.T
            idx = (obs_cam[oa][:, None] * nc + cols).reshape(-1)
            S[np.ix_(idx, idx)] -= blk.reshape(m * nc, m * nc)
            Y[np.ix_(idx, idx)] += yblk.reshape(m * nc, m * nc)
            b[idx] -= (Tm @ grs[j]).reshape(-1)
            Yb[idx] += (T(kappa[j]) * ((aW @ np.abs(Ej)) @ np.abs(grs[j]))).reshape(-1)
    return S, b, Y, Yb, diag_c, kappa


def mp_system(lin, obs_cam, obs_ray, s_c, s_r, radius, min_diag=MIN_DIAG, max_diag=MAX_DIAG):
    """The same formula with mpmath at 50 digits, from the float64 inputs as given.  Returns (S, b) as nested lists of mpf."""
    import mpmath as mp
    with mp.workdps(50):
        f = lambda v: mp.mpf(float(v))
        U, g_c, V, g_r, W = (np.asarray(lin[k], dtype=np.float64) for k in ("U", "g_c", "V", "g_r", "W"))
        n_cam, nc = U.shape[0], U.shape[1]
        n_ray, n_obs = V.shape[0], W.shape[0]
        n = n_cam * nc
        r, lo, hi = f(radius), f(min_diag), f(max_diag)
        clamp = lambda v: min(max(v, lo), hi)
        sc = [[f(v) for v in row] for row in s_c]
        sr = [[f(v) for v in row] for row in s_r]
        S = [[mp.mpf(0)] * n for _ in range(n)]
        b = [mp.mpf(0)] * n
        for c in range(n_cam):
            for p in range(nc):
                b[c * nc + p] = sc[c][p] * f(g_c[c, p])
                for q in range(nc):
                    S[c * nc + p][c * nc + q] = sc[c][p] * f(U[c, p, q]) * sc[c][q]
                S[c * nc + p][c * nc + p] += clamp(S[c * nc + p][c * nc + p]) / r
        Wm = [mp.matrix([[sc[int(obs_cam[a])][p] * f(W[a, p, k]) * sr[int(obs_ray[a])][k] for k in range(3)] for p in range(nc)]) for a in range(n_obs)]
        for j in range(n_ray):
            M = mp.matrix([[sr[j][p] * f(V[j, p, q]) * sr[j][q] for q in range(3)] for p in range(3)])
            for p in range(3):
                M[p, p] += clamp(M[p, p]) / r
            E = M ** -1
            g = mp.matrix([sr[j][k] * f(g_r[j, k]) for k in range(3)])
            oa = [a for a in range(n_obs) if obs_ray[a] == j]
            for a in oa:
                Ta = Wm[a] * E
                z = Ta * g
                ca = int(obs_cam[a]) * nc
                for p in range(nc):
                    b[ca + p] -= z[p]
                for bb in oa:
                    P = Ta * Wm[bb].T
                    cb = int(obs_cam[bb]) * nc
                    for p in range(nc):
                        for q in range(nc):
                            S[ca + p][cb + q] -= P[p, q]
        return S, b


def mp_to_ld(x):
    def one(v):
        hi = float(v)
        return LD(hi) + LD(float(v - hi))
    return np.array([[one(v) for v in row] for row in x], dtype=LD) if isinstance(x[0], list) else np.array([one(v) for v in x], dtype=LD)


def ratios(S, b, S_ref, b_ref, Y, Yb):
    """Largest |S - S_ref| / Y and |b - b_ref| / Yb in units of 2^-52 (entries with a zero yardstick must agree exactly)."""
    def one(x, ref, y):
        d = np.abs(np.asarray(x, dtype=LD) - ref)
        if not np.isfinite(np.asarray(x, dtype=np.float64)).all():
            return np.inf
        zero = y == 0
        if (d[zero] != 0).any():
            return np.inf
        return float((d[~zero] / y[~zero]).max() / LD(EPS)) if (~zero).any() else 0.0
    return one(S, S_ref, Y), one(b, b_ref, Yb)


def scales(scene, nc, seed):
    """Seeded Jacobi scales that differ per column: uniform in [1e-3, 1] for the cameras, [1e-2, 1] for the rays."""
    rng = np.random.default_rng([int(seed), scene.n_cam, scene.n_ray])
    return rng.uniform(1e-3, 1.0, (scene.n_cam, nc)), rng.uniform(1e-2, 1.0, (scene.n_ray, 3))


def shares_ray(scene, nc):
    """[n, n] bool: the two columns' cameras are one camera or see a common ray (everywhere else S is exactly zero)."""
    inc = np.zeros((scene.n_cam, scene.n_ray), dtype=bool)
    inc[scene.obs_cam, scene.obs_ray] = True
    adj = (inc.astype(np.int32) @ inc.T.astype(np.int32)) > 0
    adj |= np.eye(scene.n_cam, dtype=bool)
    return np.kron(adj, np.ones((nc, nc), dtype=bool))


# ---- scenes -----------------------------------------------------------------------------------------------------------------
# A synth.make_scene rig gives the cameras (ground truth and the perturbed initial guess); the rays are a pool of directions in
# front of the rig and an observation is the ground-truth projection of a ray plus 0.5 px of seeded noise.  Which camera observes
# which ray is dealt by the case, not by the frame: a pixel may lie outside the 1920 x 1080 image (the residual and its Jacobians
# do not know the frame), so that every camera of a narrow rig can observe every ray of the pool and the lists can be cut to exact
# counts.
EDGE_COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 512, 769, 800]
RING_CAMS = {0: 128, 1: 104, 2: 86}  # eight 64-column tiles of cameras: the planner needs six free tiles to dissect a ring
_SCENES = {}


def _rodrigues(r):
    t = np.linalg.norm(r)
    if t < 1e-15:
        return np.eye(3)
    k = r / t
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(t) * np.eye(3) + (1 - np.cos(t)) * np.outer(k, k) + np.sin(t) * Kx


def _assemble(pkg, rig, X, lists, seed):
    """Scene of the rig's cameras, the rays X that are observed at all, and the observations lists[i] = rays of camera i."""
    rng = np.random.default_rng([int(seed), len(X), rig.n_cam])
    cam = np.concatenate([np.full(len(l), i, dtype=np.int64) for i, l in enumerate(lists)])
    ray = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists])
    used = np.unique(ray)
    ray = np.searchsorted(used, ray)
    X = X[used]
    o = np.lexsort((cam, ray))
    cam, ray = cam[o], ray[o]
    R = np.stack([_rodrigues(c[4:7]) for c in rig.cam_gt])
    P = np.einsum("nij,nj->ni", R[cam], X[ray])
    assert (P[:, 2] > 0.1).all()
    x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    rad = 1.0 + rig.cam_gt[cam, 10] * (x * x + y * y)
    uv = np.stack([rig.cam_gt[cam, 0] * x * rad + rig.cam_gt[cam, 2], rig.cam_gt[cam, 1] * y * rad + rig.cam_gt[cam, 3]], axis=1)
    uv = (uv + rng.normal(0.0, 0.5, uv.shape)).astype(np.float32)
    obs_cam, obs_ray = cam.astype(np.int32), ray.astype(np.int32)
    n_ray = len(used)
    # a camera without observations has no Pix2Ray share and no residual: its parameters only enter through their own (zero) blocks
    return dataclasses.replace(rig, n_ray=n_ray, obs_uv=uv, obs_cam=obs_cam, obs_ray=obs_ray,
                               ray_weight=np.bincount(obs_ray, minlength=n_ray).astype(np.float64), ray_gt=X,
                               ray_init=pkg.synth.pix2ray(uv, obs_cam, obs_ray, n_ray, rig.cam_init), meta={})


def _pool(n, az_lo, az_hi, el, seed):
    rng = np.random.default_rng([int(seed), int(n)])
    az = np.sort(rng.uniform(np.radians(az_lo), np.radians(az_hi), n))
    e = rng.uniform(-np.radians(el), np.radians(el), n)
    return np.stack([np.cos(e) * np.sin(az), np.sin(e), np.cos(e) * np.cos(az)], axis=1), az


def _pan(rig):
    """Azimuth each camera looks at (the direction R^T e_z in the world)."""
    d = np.stack([_rodrigues(c[4:7]).T[:, 2] for c in rig.cam_gt])
    return np.arctan2(d[:, 0], d[:, 2])


def scene(pkg, kind, ftype):
    """edges: 12 cameras with EDGE_COUNTS observations (camera 10 takes the LAST 769 rays of the 800, so every ray has two views);
    band: 40 cameras over a 60-degree sector, each seeing the rays within 9 degrees of its pan angle (camera 12 of PTZRayDist
    spans columns 60-64, camera 10 of PTZRayFxfyDist 60-65); ring: RING_CAMS cameras on the full circle, the same rule;
    rounds: 258 cameras that all see the same six rays (camera 257 has 257 lower-numbered partners);
    small5: 5 cameras, 30 rays; trio0..2: 9 / 23 cameras of the band kind and, last, 12 with camera 0 unobserved."""
    key = (kind, ftype)
    if key in _SCENES:
        return _SCENES[key]
    mk = lambda sid, n, pan: pkg.synth.make_scene(sid, n, 30, factor_type=ftype, pan_range_deg=pan)
    if kind in ("edges", "trio2"):
        rig = mk(901, 12, 2.0)
        X, _ = _pool(800, -6, 6, 5, 1)
        counts = EDGE_COUNTS if kind == "edges" else [0, 7, 3, 30, 1, 12, 40, 2, 40, 17, 33, 40]
        lists = [np.arange(c) for c in counts]
        if kind == "edges":
            lists[10] = np.arange(800 - 769, 800)
        sc = _assemble(pkg, rig, X, lists, 11)
    elif kind == "rounds":
        rig = mk(902, 258, 2.0)
        X, _ = _pool(6, -6, 6, 5, 2)
        sc = _assemble(pkg, rig, X, [np.arange(6)] * 258, 12)
    elif kind == "small5":
        rig = mk(903, 5, 2.0)
        X, _ = _pool(30, -6, 6, 5, 3)
        rng = np.random.default_rng(4)
        lists = [np.sort(rng.choice(30, 24, replace=False)) for _ in range(5)]
        sc = _assemble(pkg, rig, X, lists, 13)
    else:
        n_cam, span = {"band": (40, 60.0), "ring": (RING_CAMS[ftype], 360.0), "trio0": (9, 30.0), "trio1": (23, 60.0)}[kind]
        rig = mk(904 + n_cam, n_cam, span)
        pan = _pan(rig)
        half = 180.0 if span >= 360.0 else 0.5 * span + 6.0
        X, az = _pool(6 * n_cam, -half, half, 4, 5)
        dist = np.abs(np.angle(np.exp(1j * (az[None, :] - pan[:, None]))))
        lists = [np.nonzero(dist[i] < np.radians(9.0))[0] for i in range(n_cam)]
        sc = _assemble(pkg, rig, X, lists, 14)
    _SCENES[key] = sc
    return sc


# ---- the cases of the GPU test (test_cpu_schur_reference.py runs float64 numpy over the same list) ---------------------------
KERNELS = {0: "k_schur_w", 1: "k_schur", 2: "k_schur_f"}
PATHS = [(0, 2, {}), (0, 1, {"PTZ_BA_SCHUR_F": "0"}), (0, 0, {"PTZ_BA_SCHUR_W": "1"}),
         (1, 1, {}), (1, 0, {"PTZ_BA_SCHUR_W": "1"}), (2, 1, {})]  # (factor type, kernel, switches)


def numeric_cases():
    """(scene kind, factor type, radius, clamps or None) of every system the GPU test holds to the bound.  clamps = "inside":
    min / max_lm_diagonal at the 30th / 70th percentile of diag U' (lm_clamps)."""
    out = []
    for kind in ("edges", "band"):
        out += [(kind, ft, r, None) for ft in (0, 1, 2) for r in RADII]
    out += [("ring", ft, 1e4, None) for ft in (0, 1, 2)]
    out += [("rounds", 0, r, None) for r in RADII]
    out += [("trio1", ft, 1e4, "inside") for ft in (0, 1, 2)]
    out += [(k, ft, 1e4, None) for k in ("trio0", "trio1", "trio2") for ft in (0, 1, 2)]
    return out


def lm_clamps(lin, s_c):
    """min / max_lm_diagonal inside the range of diag U': its 30th and 70th percentile over the observed cameras' columns."""
    U = np.asarray(lin["U"], dtype=np.float64)
    nc = U.shape[1]
    dg = (s_c * s_c * U[:, np.arange(nc), np.arange(nc)])
    dg = dg[dg > 0]
    return float(np.percentile(dg, 30)), float(np.percentile(dg, 70))
