"""Shared by test_cpu_ba_covariance.py and test_gpu_ba_covariance.py: the scenes and the INDEPENDENT restatement of the
per-view covariance of bundle-adjusted cameras (ptz_ba_batch_covariance, ptz-calib_amd/csrc/ptz_ba_cov.h).

The restatement shares no code with the library.  Parameters: per camera p = [fx, (fy), d1, d2, d3, (k1)] with d applied as
R <- Exp(d) R (so nothing is converted afterwards), per ray two tangents: x <- |x| (x^ + a t1 + b t2) with t1, t2 an
orthonormal basis of the plane orthogonal to x^.  J by central differences of oracle.ba_residuals (unweighted residuals),
H = J^T W J, M = J^T W^2 J with the track weights, the gauge by deleting the anchor's three rotation columns,
C = s^2 H^-1 M H^-1 by numpy.linalg.inv on the unit-diagonal H, s^2 = |e|^2 / (m - columns) or pixel_sigma^2.
"""
import functools

import numpy as np

import __graft_entry__ as ge

OK, DOF, SINGULAR = 0, 1, 2
NF = {0: 4, 1: 5, 2: 6}
ROT0 = {0: 1, 1: 1, 2: 2}  # first rotation slot of p


@functools.lru_cache(maxsize=None)
def _orc():
    o = ge.load_oracle()
    o.build()
    return o


def _exp(d):
    return _orc().rodrigues(np.asarray(d, dtype=np.float64))


def _perturb_cams(ft, cam, k, h):
    """every camera's free parameter k (output order) moved by h (rotations: R <- Exp(h e) R)"""
    o = _orc()
    c = cam.copy()
    r0 = ROT0[ft]
    if k < r0:
        c[:, k] = cam[:, k] * (1.0 + h)  # (relative step in the focal lengths)
    elif k < r0 + 3:
        d = np.zeros(3); d[k - r0] = h
        E = _exp(d)
        for i in range(len(c)):
            c[i, 4:7] = o.rodrigues_inv(E @ o.rodrigues(cam[i, 4:7]))
    else:
        c[:, 10] += h
    return c


def _tangents(ray):
    x = ray / np.linalg.norm(ray, axis=1, keepdims=True)
    e = np.eye(3)[np.argmin(np.abs(x), axis=1)]
    t1 = np.cross(x, e); t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(x, t1)
    return x, t1, t2


def jacobian(sc, cam, ray, rel):
    """dense J [2 n_obs, NF n_cam + 2 n_ray] at (cam, ray), central differences with relative step `rel`"""
    o = _orc()
    ft, nf = sc.factor_type, NF[sc.factor_type]
    n_obs = len(sc.obs_cam)
    J = np.zeros((2 * n_obs, nf * sc.n_cam + 2 * sc.n_ray))
    rows = np.arange(n_obs)
    for k in range(nf):
        rp = o.ba_residuals(sc, _perturb_cams(ft, cam, k, rel), ray)
        rm = o.ba_residuals(sc, _perturb_cams(ft, cam, k, -rel), ray)
        step = (rel * cam[sc.obs_cam, k]).reshape(-1, 1) if k < ROT0[ft] else rel
        dr = (rp - rm) / (2 * step)
        J[2 * rows, nf * sc.obs_cam + k] = dr[:, 0]
        J[2 * rows + 1, nf * sc.obs_cam + k] = dr[:, 1]
    x, t1, t2 = _tangents(ray)
    nrm = np.linalg.norm(ray, axis=1, keepdims=True)
    for k, t in enumerate((t1, t2)):
        rp = o.ba_residuals(sc, cam, nrm * (x + rel * t))
        rm = o.ba_residuals(sc, cam, nrm * (x - rel * t))
        dr = (rp - rm) / (2 * rel)
        J[2 * rows, nf * sc.n_cam + 2 * sc.obs_ray + k] = dr[:, 0]
        J[2 * rows + 1, nf * sc.n_cam + 2 * sc.obs_ray + k] = dr[:, 1]
    return J


def _cov_from_J(sc, J, res, gauge, pixel_sigma):
    ft, nf = sc.factor_type, NF[sc.factor_type]
    n_obs = len(sc.obs_cam)
    w = np.repeat(np.asarray(sc.ray_weight, dtype=np.float64)[sc.obs_ray], 2)
    g0 = gauge * nf + ROT0[ft]
    keep = np.ones(J.shape[1], dtype=bool); keep[g0:g0 + 3] = False
    Jk = J[:, keep]
    m, p = 2 * n_obs, Jk.shape[1]
    assert p == nf * sc.n_cam - 3 + 2 * sc.n_ray
    if m <= p:
        return DOF, None, None, None
    H = Jk.T @ (w[:, None] * Jk)
    M = Jk.T @ ((w * w)[:, None] * Jk)
    dg = np.diag(H)
    sse = float((res ** 2).sum())
    if not (np.isfinite(dg).all() and (dg > 0).all() and np.isfinite(sse)):
        return SINGULAR, None, None, None
    s = 1.0 / np.sqrt(dg)
    Hs = H * s[:, None] * s[None, :]
    cond = np.linalg.cond(Hs)
    Hi = np.linalg.inv(Hs)
    Cfull = (Hi @ (M * s[:, None] * s[None, :]) @ Hi) * s[:, None] * s[None, :]
    s2 = sse / (m - p)
    var = pixel_sigma ** 2 if pixel_sigma > 0 else s2
    full = np.zeros((J.shape[1], J.shape[1]))
    full[np.ix_(keep, keep)] = var * Cfull
    cov = np.stack([full[nf * c:nf * c + nf, nf * c:nf * c + nf] for c in range(sc.n_cam)])
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))
    return OK, cov, np.sqrt(s2), cond


def restate(sc, cam, ray, gauge=0, pixel_sigma=0.0, check=True):
    """(status, cov [n_cam, NF, NF], sigma0, scaled cond(H)) of the problem `sc` at (cam, ray).  With `check` the two steps 1e-6
    and 1e-5 must agree below 1e-7 of the standard deviations: otherwise the 1e-6 bound of the tests cannot carry the scene."""
    cam = np.ascontiguousarray(cam, dtype=np.float64); ray = np.ascontiguousarray(ray, dtype=np.float64)
    res = _orc().ba_residuals(sc, cam, ray)
    st, cov, s0, cond = _cov_from_J(sc, jacobian(sc, cam, ray, 1e-6), res, gauge, pixel_sigma)
    if st != OK or not check:
        return st, cov, s0, cond
    st2, cov2, _, _ = _cov_from_J(sc, jacobian(sc, cam, ray, 1e-5), res, gauge, pixel_sigma)
    assert st2 == OK
    assert scaled_diff(cov2, cov) < 1e-7, ("the restatement's two steps disagree", scaled_diff(cov2, cov), cond)
    return st, cov, s0, cond


def scaled_diff(c, ref):
    """max |C_ij - Cref_ij| / sqrt(Cref_ii Cref_jj) over the entries whose standard deviations are non-zero"""
    sd = np.sqrt(np.maximum(np.einsum("cii->ci", ref), 0.0))
    den = sd[:, :, None] * sd[:, None, :]
    ok = den > 0
    assert (np.abs(np.asarray(c)[~ok]) == 0).all() and (ref[~ok] == 0).all()  # the anchor's rotation rows and columns
    return float((np.abs(np.asarray(c) - ref)[ok] / den[ok]).max())


@functools.lru_cache(maxsize=None)
def solved_scene(scene_id, n_views, obs_per_view, factor_type):
    """(scene, cam, ray) at the oracle's minimum"""
    pkg = ge.load_package()
    o = _orc()
    sc = pkg.synth.make_scene(scene_id, n_views, obs_per_view, factor_type=factor_type)
    cam, ray, _, summ, _ = o.ba_solve(sc, jacobian_mode=o.JAC_ANALYTIC, function_tolerance=1e-14, parameter_tolerance=1e-12,
                                      max_num_iterations=100)
    return sc, cam, ray


@functools.lru_cache(maxsize=None)
def restated(scene_id, n_views, obs_per_view, factor_type, gauge=0):
    sc, cam, ray = solved_scene(scene_id, n_views, obs_per_view, factor_type)
    return restate(sc, cam, ray, gauge)


def problem_args(sc):
    """contiguous arrays of a scene in the layout of ptz_ba_problem"""
    return (np.ascontiguousarray(sc.obs_uv, dtype=np.float32), np.ascontiguousarray(sc.obs_cam, dtype=np.int32),
            np.ascontiguousarray(sc.obs_ray, dtype=np.int32), np.ascontiguousarray(sc.ray_weight, dtype=np.float64))


# ---- the statistics test: N noisy copies of one geometry ----------------------------------------------------------------------
STAT_N, STAT_SIGMA, STAT_SEED = 400, 0.5, 20261017


@functools.lru_cache(maxsize=None)
def noisy_copies(n=STAT_N, sigma=STAT_SIGMA, seed=STAT_SEED):
    """n copies of a 6-view x 40-obs PTZRay geometry: exact projections of the ground truth plus N(0, sigma) on the pixels,
    float32; the initial guess of every copy is the scene's.  Returns (base scene with exact pixels, list of scenes)."""
    import copy
    pkg = ge.load_package()
    o = _orc()
    base = pkg.synth.make_scene(11, 6, 40, noise_px=0.0)
    # exact pixels: the oracle's residual at the ground truth is (pixel - projection)
    exact = base.obs_uv.astype(np.float64) - o.ba_residuals(base, base.cam_gt, base.ray_gt)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        s = copy.copy(base)
        s.obs_uv = (exact + rng.normal(0.0, sigma, exact.shape)).astype(np.float32)
        s.ray_init = pkg.synth.pix2ray(s.obs_uv, s.obs_cam, s.obs_ray, s.n_ray, s.cam_init)
        out.append(s)
    base = copy.copy(base)
    base.obs_uv = exact.astype(np.float32)
    return base, out


def stat_ratios(cams, covs, sigma0s, anchor=0, sigma=STAT_SIGMA, factor_type=0):
    """The ratios of the statistics test from the solved cameras [N, n_cam, 15], the predicted covariances [N, n_cam, NF, NF]
    and sigma0 [N]: scatter of fx over the mean predicted sigma_f per camera; per non-anchor camera and axis the scatter of
    Log(Q_i Qbar_i^T), Q_i = R_i R_anchor^T, over the mean predicted sigma_d; mean sigma0 over sigma."""
    o = _orc()
    cams = np.asarray(cams); covs = np.asarray(covs)
    N, n_cam = cams.shape[:2]
    r0 = ROT0[factor_type]
    ratios = {}
    sd = np.sqrt(np.einsum("ncii->nci", covs))
    for c in range(n_cam):
        ratios["f%d" % c] = cams[:, c, 0].std(ddof=1) / sd[:, c, 0].mean()
    R = np.array([[o.rodrigues(cams[i, c, 4:7]) for c in range(n_cam)] for i in range(N)])
    for c in range(n_cam):
        if c == anchor:
            continue
        Q = np.einsum("nij,nkj->nik", R[:, c], R[:, anchor])
        # the mean rotation: iterate Qbar <- Exp(mean Log(Q Qbar^T)) Qbar
        Qb = Q[0].copy()
        for _ in range(10):
            lg = np.array([o.rodrigues_inv(q @ Qb.T) for q in Q])
            Qb = o.rodrigues(lg.mean(axis=0)) @ Qb
        lg = np.array([o.rodrigues_inv(q @ Qb.T) for q in Q])
        for a in range(3):
            ratios["d%d%s" % (c, "xyz"[a])] = lg[:, a].std(ddof=1) / sd[:, c, r0 + a].mean()
    ratios["sigma0"] = float(np.mean(sigma0s)) / sigma
    return ratios
