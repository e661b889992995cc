"""The landmark view's contract (ptz-calib_amd/csrc/ptz_landmark_prior.h) restated in numpy: the prediction m = R_q L in float64 with
every product, sum and quotient rounded on its own and in the header's order, the visibility rule on the doubles, the view as the
visible landmarks in ascending index.  The yardstick of the CPU harness (tests/cpu_harness/landmark_prior_harness.cc) and, through
it, of the device; nothing here is shared with either.  Every figure is reproduced bit for bit: all outputs are compared
array-equal, no ulp bound is needed."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import reloc_assemble_util as U
import reloc_prior_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("vis_ptr", "vis_lm", "vis_uv")
_h = None


# ------------------------------------------------------------------------------------------------------------- the restatement
def predict(K4, R_q, w, h, radius_px, L):
    """landmark_predict for rays L [n, 3]: (pixels float32 [n, 2], visible bool [n])."""
    L = np.asarray(L, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(R_q, dtype=np.float64).reshape(9)
    rad = float(radius_px)
    with np.errstate(all="ignore"):
        mx = R[0] * L[:, 0] + R[1] * L[:, 1] + R[2] * L[:, 2]
        my = R[3] * L[:, 0] + R[4] * L[:, 1] + R[5] * L[:, 2]
        mz = R[6] * L[:, 0] + R[7] * L[:, 1] + R[8] * L[:, 2]
        ok = (mz > 0) & np.isfinite(mx) & np.isfinite(my) & np.isfinite(mz)
        px = K4[0] * (mx / mz) + K4[2]
        py = K4[1] * (my / mz) + K4[3]
        vis = ok & (px >= -rad) & (px < float(w) + rad) & (py >= -rad) & (py < float(h) + rad)
        uv = np.stack([px, py], axis=1).astype(np.float32)
    return uv, vis


def visible(lm_ray, prior_cams, query_wh, factor_type=0, radius_px=40.0, prior_R=None):
    """The dict api.LandmarkView.arrays() returns."""
    L = np.asarray(lm_ray, dtype=np.float64).reshape(-1, 3)
    pri = np.asarray(prior_cams, dtype=np.float64).reshape(-1, 15)
    R = U.rotations(pri) if prior_R is None else np.asarray(prior_R, dtype=np.float64).reshape(-1, 9)
    wh = np.asarray(query_wh).reshape(-1, 2)
    ptr, lm, uv = [0], [], []
    for q in range(len(pri)):
        K4 = PU.query_K(pri[q], wh[q, 0], wh[q, 1], factor_type)
        p, vis = predict(K4, R[q], int(wh[q, 0]), int(wh[q, 1]), radius_px, L)
        idx = np.nonzero(vis)[0]
        lm.append(idx.astype(np.int32))
        uv.append(p[idx])
        ptr.append(ptr[-1] + len(idx))
    return dict(vis_ptr=np.asarray(ptr, dtype=np.int64), vis_lm=np.concatenate(lm).astype(np.int32) if lm else np.zeros(0, dtype=np.int32),
                vis_uv=np.concatenate(uv).astype(np.float32).reshape(-1, 2) if uv else np.zeros((0, 2), dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------ the host harness
def harness():
    global _h
    if _h is None:
        _h = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "liblandmark_prior_harness.so"))
        _h.h_landmark_visible.restype = C.c_int64
    return _h


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness_visible(lm_ray, prior_cams, query_wh, factor_type=0, radius_px=40.0, prior_R=None, capacity=None):
    """The harness's view; capacity: only that many entries of vis_lm / vis_uv are written (vis_ptr stays complete)."""
    L = np.ascontiguousarray(lm_ray, dtype=np.float64).reshape(-1, 3)
    pri = np.ascontiguousarray(prior_cams, dtype=np.float64).reshape(-1, 15)
    R = U.harness_rotations(pri) if prior_R is None else np.ascontiguousarray(prior_R, dtype=np.float64).reshape(-1, 9)
    wh = np.ascontiguousarray(query_wh, dtype=np.int32).reshape(-1, 2)
    nq = len(pri)
    ptr = np.zeros(nq + 1, dtype=np.int64)
    args = (len(L), _p(L), nq, _p(pri), _p(R), _p(wh), int(factor_type), C.c_double(float(radius_px)), _p(ptr))
    n = int(harness().h_landmark_visible(*args, None, None, C.c_int64(0)))
    k = n if capacity is None else min(n, int(capacity))
    lm, uv = np.zeros(max(k, 1), dtype=np.int32), np.zeros((max(k, 1), 2), dtype=np.float32)
    harness().h_landmark_visible(*args, _p(lm), _p(uv), C.c_int64(k))
    return dict(vis_ptr=ptr, vis_lm=lm[:k], vis_uv=uv[:k])


def assert_equal(got, want, what="", keys=KEYS):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, k)


def per_query(view, q):
    """The view of query q alone."""
    sl = slice(int(view["vis_ptr"][q]), int(view["vis_ptr"][q + 1]))
    return dict(vis_lm=view["vis_lm"][sl], vis_uv=view["vis_uv"][sl])


# ------------------------------------------------------------------------------------------------------------------ test data
def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def make_priors(n_query, factor_type, seed=0):
    """n_query prior cameras around pan 0 with sizes of their own; distortion set (it must not enter), fy != fx (it enters for
    Fxfy / FxfyDist only).  The LAST query looks the other way: it sees what is behind the others."""
    rng = np.random.default_rng(seed)
    cams = np.zeros((n_query, 15))
    cams[:, 0] = rng.uniform(1500, 4000, n_query)
    cams[:, 1] = cams[:, 0] * rng.uniform(0.9, 1.1, n_query)
    cams[:, 4:7] = rng.uniform(-0.25, 0.25, (n_query, 3))
    cams[:, 10:12] = rng.uniform(-0.1, 0.1, (n_query, 2))
    wh = np.stack([rng.integers(600, 4000, n_query), rng.integers(400, 2200, n_query)], axis=1).astype(np.int32)
    cams[:, 2], cams[:, 3] = 0.5 * wh[:, 0], 0.5 * wh[:, 1]
    if n_query > 1:
        cams[-1, 4:7] = (0.0, np.pi, 0.0)
    if n_query > 2:  # the middle query looks straight up through a very long lens: it sees nothing
        cams[n_query // 2, 4:7] = (0.5 * np.pi, 0.0, 0.0)
        cams[n_query // 2, 0:2] = 1e7
    return cams, wh


def edge_rays(prior, R_q, w, h, factor_type, radius_px):
    """Rays that land just inside and just outside each of the four margins of one query, one behind it, one on its optical axis:
    pixel (px, py) back-projected as R_q^T ((px - cx) / fx, (py - cy) / fy, 1)."""
    K4 = PU.query_K(prior, w, h, factor_type)
    R = np.asarray(R_q, dtype=np.float64).reshape(3, 3)
    cx, cy, r, e = K4[2], K4[3], float(radius_px), 0.25
    pix = [(-r + e, cy), (-r - e, cy), (w + r - e, cy), (w + r + e, cy), (cx, -r + e), (cx, -r - e), (cx, h + r - e), (cx, h + r + e), (cx, cy)]
    n = np.array([[(px - cx) / K4[0], (py - cy) / K4[1], 1.0] for px, py in pix])
    rays = unit(n @ R)  # R^T n per row
    behind = -rays[-1]
    return np.concatenate([rays, behind[None]])


def random_rays(n, seed=0, cone=0.6):
    """n unit rays around +z (the priors' pan 0), some far off."""
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.uniform(-cone, cone, (n, 2)), np.ones((n, 1))], axis=1)
    far = rng.random(n) < 0.1
    v[far] = rng.normal(size=(int(far.sum()), 3))
    return unit(v)


def nasty_rays(seed=0):
    """Rays no map holds but the device form may be fed: m_z <= 0, NaN, infinities and huge components, zero."""
    return np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [np.nan, 0.0, 1.0], [0.0, np.nan, 1.0], [0.0, 0.0, np.nan], [np.inf, 0.0, 1.0],
                     [0.0, 0.0, np.inf], [1e308, 1e308, 1e308], [-1e308, 1e308, 1e308], [1e300, 0.0, 1e-300], [0.0, 0.0, 0.0],
                     [0.0, 0.0, 1e-320], [0.0, 0.0, 1.0]])


def make_case(n_lm, n_query, factor_type, seed=0, radius_px=40.0):
    """(rays [n_lm, 3], prior_cams, query_wh): the edge rays of query 0, the nasty rays, then random ones -- cut to n_lm."""
    cams, wh = make_priors(n_query, factor_type, seed) if n_query else (np.zeros((0, 15)), np.zeros((0, 2), dtype=np.int32))
    parts = [nasty_rays(seed)]
    if n_query:
        parts.insert(0, edge_rays(cams[0], U.rotations(cams[:1])[0], int(wh[0, 0]), int(wh[0, 1]), factor_type, radius_px))
    parts.append(random_rays(max(n_lm, 1), seed + 1))
    return np.concatenate(parts)[:n_lm].copy(), cams, wh
