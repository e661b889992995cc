"""Shared by test_cpu_ba_trim.py, test_gpu_ba_residuals.py and test_gpu_ba_trim.py: the contaminated rigs, the numpy restatements
of the re-packing (ptz_ba_problem_trim) and of the selection rule (ptz-calib_amd/csrc/ptz_ba_trim.h), the host instantiation of
that header (tests/cpu_harness/ba_trim_harness.cc), and the trimmed loop written on the CPU oracle alone.

Nothing here shares code with the library except the two things under test that the oracle loop is defined with: the C
re-packing and the host selection.  Every oracle loop is computed once per process and shared (lru_cache); callers copy."""
import copy
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYLEIGH_MEDIAN = 1.1774
ENOOBS, EINVAL, EUNSUPPORTED = -6, -1, -4

# (scene id, views, observations per view, factor type, fraction displaced)
CONTAMINATED = [(11, 8, 60, 0, 0.05), (11, 8, 60, 1, 0.05), (12, 20, 100, 0, 0.10), (15, 12, 60, 0, 0.20), (13, 6, 40, 2, 0.05)]
CLEAN = (14, 6, 40, 0)
CONTAMINATION_SEED = 1


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def orc():
    o = ge.load_oracle()
    o.build()
    return o


@functools.lru_cache(maxsize=None)
def pkg():
    return ge.load_package()


@functools.lru_cache(maxsize=None)
def harness():
    so = os.path.join(ROOT, "tests", "cpu_harness", "libba_trim_harness.so")
    src = os.path.join(ROOT, "tests", "cpu_harness", "ba_trim_harness.cc")
    srcs = [src, os.path.join(ROOT, "ptz-calib_amd", "csrc", "ptz_ba_trim.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    return C.CDLL(so)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clean_scene(scene_id, views, per_view, factor_type):
    return pkg().synth.make_scene(scene_id, views, per_view, factor_type=factor_type)


@functools.lru_cache(maxsize=None)
def contaminated_scene(scene_id, views, per_view, factor_type, frac, seed=CONTAMINATION_SEED):
    """(scene, displaced [n_obs] bool): round(frac n_obs) observations chosen without replacement, moved by 20..80 px in a uniform
    direction (angles drawn first, then magnitudes), added to obs_uv in float32; ray_init recomputed by Pix2Ray."""
    sc = copy.copy(clean_scene(scene_id, views, per_view, factor_type))
    rng = np.random.default_rng(seed)
    n = sc.n_obs
    idx = rng.choice(n, size=int(round(frac * n)), replace=False)
    ang = rng.uniform(0.0, 2.0 * np.pi, len(idx))
    mag = rng.uniform(20.0, 80.0, len(idx))
    uv = np.array(sc.obs_uv, dtype=np.float32).copy()
    uv[idx] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1).astype(np.float32)
    sc.obs_uv = uv
    sc.ray_init = pkg().synth.pix2ray(sc.obs_uv, sc.obs_cam, sc.obs_ray, sc.n_ray, sc.cam_init)
    bad = np.zeros(n, dtype=bool)
    bad[idx] = True
    return sc, bad


# ---- restatements ------------------------------------------------------------------------------------------------------------------
def err_norm(res):
    """|e_o| of the oracle's residual pairs"""
    res = np.asarray(res, dtype=np.float64)
    return np.sqrt(res[:, 0] * res[:, 0] + res[:, 1] * res[:, 1])


def trim_restated(sc, reject):
    """numpy restatement of ptz_ba_problem_trim: dict(uv, cam, ray, w, ray_map), or None where a camera is emptied"""
    reject = np.asarray(reject) != 0
    obs_ray = np.asarray(sc.obs_ray)
    total = np.bincount(obs_ray, minlength=sc.n_ray)
    left = np.bincount(obs_ray[~reject], minlength=sc.n_ray)
    alive = left >= 2
    keep = ~reject & alive[obs_ray]
    if (np.bincount(np.asarray(sc.obs_cam)[keep], minlength=sc.n_cam) == 0).any():
        return None
    ray_map = np.where(alive, np.cumsum(alive) - 1, -1).astype(np.int32)
    return dict(uv=np.asarray(sc.obs_uv, dtype=np.float32)[keep], cam=np.asarray(sc.obs_cam, dtype=np.int32)[keep],
                ray=ray_map[obs_ray[keep]], w=(np.asarray(sc.ray_weight, dtype=np.float64) - (total - left))[alive], ray_map=ray_map,
                keep=keep)


def select_restated(obs_ray, n_ray, err, trim_px, k_sigma):
    """numpy restatement of the rule: (reject uint8 [n_obs], threshold, median or None, ray_max, ray_worst)"""
    err = np.asarray(err, dtype=np.float64)
    obs_ray = np.asarray(obs_ray)
    n = len(err)
    med = None
    t = float(trim_px)
    if k_sigma > 0:
        med = float(np.sort(err)[(n - 1) // 2])
        t = max(float(trim_px), k_sigma * med / RAYLEIGH_MEDIAN)
    reject = np.zeros(n, dtype=np.uint8)
    ray_max = np.zeros(n_ray)
    ray_worst = -np.ones(n_ray, dtype=np.int32)
    start = np.searchsorted(obs_ray, np.arange(n_ray + 1))
    for r in range(n_ray):
        a0, a1 = start[r], start[r + 1]
        if a1 == a0:
            continue
        k = a0 + int(np.argmax(err[a0:a1]))  # (argmax: the first of equal maxima)
        ray_max[r], ray_worst[r] = err[k], k
        if err[k] > t:
            reject[k] = 1
    return reject, t, med, ray_max, ray_worst


def select_host(obs_ray, n_ray, err, trim_px, k_sigma):
    """the header's rule on the host (ba_trim_harness.cc): the same tuple as select_restated, median NaN when none is taken"""
    err = np.ascontiguousarray(err, dtype=np.float64)
    obs_ray = np.ascontiguousarray(obs_ray, dtype=np.int32)
    n = len(err)
    reject = np.zeros(n, dtype=np.uint8)
    ray_max = np.zeros(n_ray)
    ray_worst = np.zeros(n_ray, dtype=np.int32)
    t, med = C.c_double(), C.c_double()
    nrej = harness().ba_trim_harness_select(C.c_int64(n), C.c_int32(n_ray), _p(obs_ray), _p(err), C.c_double(trim_px), C.c_double(k_sigma),
                                            _p(reject), _p(ray_max), _p(ray_worst), C.byref(t), C.byref(med))
    assert nrej == int(reject.sum())
    return reject, t.value, med.value, ray_max, ray_worst


# ---- the trimmed loop on the oracle ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_loop(scene_id, views, per_view, factor_type, frac, trim_px=4.0, k_sigma=3.0, max_rounds=8, seed=CONTAMINATION_SEED):
    """solve (oracle_py.ba_solve), measure (ba_residuals), select (the header on the host), re-pack (the C re-packing), solve again
    from where the last round ended.  Returns dict(cam, kept, rounds, n_obs_removed, n_ray_removed, threshold, margin, flagged,
    rms_first, rms_last); margin = the smallest |ray_max - threshold| over all rounds."""
    o, api = orc(), pkg().api
    sc = contaminated_scene(scene_id, views, per_view, factor_type, frac, seed)[0] if frac > 0 else clean_scene(scene_id, views, per_view, factor_type)
    cur, cam, ray = sc, np.array(sc.cam_init, dtype=np.float64), np.array(sc.ray_init, dtype=np.float64)
    obs_orig = np.arange(sc.n_obs)
    rounds, margin, flagged, rms_first, t = 0, np.inf, False, None, None
    while True:
        cam, ray, _, _, _ = o.ba_solve(cur, cam0=cam, ray0=ray, jacobian_mode=o.JAC_ANALYTIC)
        rounds += 1
        err = err_norm(o.ba_residuals(cur, cam, ray))
        rms = float(np.sqrt(np.mean(err * err)))
        rms_first = rms if rms_first is None else rms_first
        reject, t, _, ray_max, _ = select_host(cur.obs_ray, cur.n_ray, err, trim_px, k_sigma)
        margin = min(margin, float(np.abs(ray_max - t).min()))
        if reject.sum() == 0:
            break
        if rounds >= max_rounds:
            flagged = True
            break
        try:
            new, ray_map = api.ba_trim_problem(cur, reject)
        except api.PtzError as e:
            assert e.code == ENOOBS
            flagged = True
            break
        keep = (reject == 0) & (ray_map[cur.obs_ray] >= 0)
        obs_orig, ray, cur = obs_orig[keep], ray[ray_map >= 0], new
    kept = np.zeros(sc.n_obs, dtype=np.uint8)
    kept[obs_orig] = 1
    return dict(cam=cam, kept=kept, rounds=rounds, n_obs_removed=sc.n_obs - cur.n_obs, n_ray_removed=sc.n_ray - cur.n_ray, threshold=t,
                margin=margin, flagged=flagged, rms_first=rms_first, rms_last=rms)


@functools.lru_cache(maxsize=None)
def clean_fit_focal_error(scene_id, views, per_view, factor_type):
    """largest focal error of the oracle's fit of the rig without contamination"""
    o = orc()
    sc = clean_scene(scene_id, views, per_view, factor_type)
    cam = o.ba_solve(sc, jacobian_mode=o.JAC_ANALYTIC)[0]
    return focal_error(sc, cam)


def focal_error(sc, cam):
    return float(np.abs(np.asarray(cam)[:, 0] - sc.cam_gt[:, 0]).max())
