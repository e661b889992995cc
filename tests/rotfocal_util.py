"""The rotation-and-focal gate's contract (ptz-calib_amd/csrc/ptz_rotfocal.h) restated in numpy, its host harness
(tests/cpu_harness/rotfocal_harness.cc) behind ctypes, the gate's compaction restated on integers, and the generator the tests share.

The restatement works on IEEE doubles with + - * / sqrt only and sums left to right, so it returns the header's bits: per hypothesis the
scalar part runs on np.float64 scalars, the inlier test elementwise over the matches (numpy's elementwise ufuncs round every operation
on its own)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS_SRC = os.path.join(ROOT, "tests", "cpu_harness", "rotfocal_harness.cc")
SEED = 0x50545A48
M64 = (1 << 64) - 1
VIRTUAL = np.array([1500.0, 1500.0, 8192.0, 8192.0] + [0.0] * 11)   # the virtual anchor [fa, fa, S, S] of the K > 1 assemblies
REAL = np.array([2200.0, 2210.0, 960.0, 540.0] + [0.0] * 11)        # a real 1920 x 1080 anchor, fx != fy
_h = None


def harness():
    global _h
    if _h is None:
        _h = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "librotfocal_harness.so"))
        _h.h_rotfocal_sample.restype = None
        _h.h_rotfocal_batch.restype = None
        _h.h_rotfocal_find.restype = C.c_int32
        _h.h_rotfocal_hypothesis.restype = C.c_int32
    return _h


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------
def _next(s):
    s = (s + 0x9E3779B97F4A7C15) & M64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return s, z ^ (z >> 31)


def sample(it, n):
    s = (SEED + (it + 1) * 0xD1342543DE82EF95) & M64
    s, z = _next(s)
    i = z % n
    s, z = _next(s)
    j = z % (n - 1)
    if j >= i:
        j += 1
    return int(i), int(j)


def lift(uv_a, uv_b, cam_a, cxq, cyq):
    """[n, 4] doubles (a_x, a_y, q_x, q_y)"""
    a = np.asarray(uv_a, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    b = np.asarray(uv_b, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    cam = np.asarray(cam_a, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.stack([(a[:, 0] - cam[2]) / cam[0], (a[:, 1] - cam[3]) / cam[1], b[:, 0] - np.float64(cxq), b[:, 1] - np.float64(cyq)], axis=1)


def _triad(v, w):
    nv = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    e1 = [v[0] / nv, v[1] / nv, v[2] / nv]
    c = [v[1] * w[2] - v[2] * w[1], v[2] * w[0] - v[0] * w[2], v[0] * w[1] - v[1] * w[0]]
    nc = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    e3 = [c[0] / nc, c[1] / nc, c[2] / nc]
    e2 = [e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]]
    return e1, e2, e3


def hypothesis(li, lj, root):
    """model [10] = f, R row-major, or None"""
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        ai, aj = [li[0], li[1], one], [lj[0], lj[1], one]
        nai = ai[0] * ai[0] + ai[1] * ai[1] + ai[2] * ai[2]
        naj = aj[0] * aj[0] + aj[1] * aj[1] + aj[2] * aj[2]
        A = nai * naj
        c0, c1, c2 = ai[1] * aj[2] - ai[2] * aj[1], ai[2] * aj[0] - ai[0] * aj[2], ai[0] * aj[1] - ai[1] * aj[0]
        X = c0 * c0 + c1 * c1 + c2 * c2
        n1, n2 = li[2] * li[2] + li[3] * li[3], lj[2] * lj[2] + lj[3] * lj[3]
        dx, dy = li[2] - lj[2], li[3] - lj[3]
        e = dx * dx + dy * dy
        kk = li[2] * lj[3] - li[3] * lj[2]
        k = kk * kk
        b = X * (n1 + n2) - A * e
        c = X * (n1 * n2) - A * k
        disc = b * b - (np.float64(4.0) * X) * c
        if not (X > 0.0) or not (disc >= 0.0):
            return None
        sq = np.sqrt(disc)
        t = np.float64(-0.5) * (b + (sq if b >= 0.0 else -sq))
        if not (t != 0.0):
            return None
        F = t / X if root == 0 else c / t
        dq = li[2] * lj[2] + li[3] * lj[3]
        da = ai[0] * aj[0] + ai[1] * aj[1] + ai[2] * aj[2]
        if not np.isfinite(F) or not (F > 0.0) or not ((dq + F) * da > 0.0):
            return None
        f = np.sqrt(F)
        E = _triad(ai, aj)
        G = _triad([li[2], li[3], f], [lj[2], lj[3], f])
        m = np.empty(10)
        m[0] = f
        for r in range(3):
            for cc in range(3):
                m[1 + 3 * r + cc] = G[0][r] * E[0][cc] + G[1][r] * E[1][cc] + G[2][r] * E[2][cc]
    return m if np.isfinite(m).all() else None


def inliers(m, L, thresh):
    thr2 = np.float64(thresh) * np.float64(thresh)
    ax, ay, qx, qy = L[:, 0], L[:, 1], L[:, 2], L[:, 3]
    with np.errstate(all="ignore"):
        mx = m[1] * ax + m[2] * ay + m[3]
        my = m[4] * ax + m[5] * ay + m[6]
        mz = m[7] * ax + m[8] * ay + m[9]
        ex = (m[0] * mx) / mz - qx
        ey = (m[0] * my) / mz - qy
        return (mz > 0.0) & (ex * ex + ey * ey <= thr2)


def homography(m, cam_a, cxq, cyq):
    cam = np.asarray(cam_a, dtype=np.float64)
    f, R = m[0], m[1:]
    N = np.empty(9)
    with np.errstate(all="ignore"):
        for i in range(3):
            N[3 * i] = R[3 * i] / cam[0]
            N[3 * i + 1] = R[3 * i + 1] / cam[1]
            N[3 * i + 2] = (R[3 * i + 2] - N[3 * i] * cam[2]) - N[3 * i + 1] * cam[3]
        G = np.empty(9)
        for j in range(3):
            G[j] = f * N[j] + np.float64(cxq) * N[6 + j]
            G[3 + j] = f * N[3 + j] + np.float64(cyq) * N[6 + j]
            G[6 + j] = N[6 + j]
        return G / G[8] if abs(G[8]) > 1e-300 else np.full(9, np.nan)


def find(uv_a, uv_b, cam_a, cxq, cyq, thresh=4.0, iters=128):
    """dict(found, model [10], H [9], mask uint8 [n], best_count, best_h); model / H / mask are None unless found"""
    L = lift(uv_a, uv_b, cam_a, cxq, cyq)
    n = len(L)
    out = dict(found=0, model=None, H=None, mask=None, best_count=-1, best_h=-1)
    if n < 2:
        return out
    best, best_h, best_m, best_in = -1, -1, None, None
    for it in range(iters):
        i, j = sample(it, n)
        for root in (0, 1):
            m = hypothesis(L[i], L[j], root)
            if m is None:
                continue
            inl = inliers(m, L, thresh)
            c = int(inl.sum())
            if c > best:
                best, best_h, best_m, best_in = c, 2 * it + root, m, inl
    out["best_count"], out["best_h"] = best, best_h
    if best < 3:
        return out
    out.update(found=1, model=best_m, H=homography(best_m, cam_a, cxq, cyq), mask=best_in.astype(np.uint8))
    return out


# ---- the host harness ------------------------------------------------------------------------------------------------------------------
def harness_find(uv_a, uv_b, cam_a, cxq, cyq, thresh=4.0, iters=128):
    a = np.ascontiguousarray(uv_a, dtype=np.float32).reshape(-1, 2)
    b = np.ascontiguousarray(uv_b, dtype=np.float32).reshape(-1, 2)
    cam = np.ascontiguousarray(cam_a, dtype=np.float64)
    n = len(a)
    model, H, mask, best = np.full(10, -7.0), np.full(9, -7.0), np.full(n + 1, 9, dtype=np.uint8), C.c_int32(0)
    found = harness().h_rotfocal_find(n, _p(a), _p(b), _p(cam), C.c_double(cxq), C.c_double(cyq), C.c_double(thresh), int(iters), _p(model), _p(H),
                                      _p(mask), C.byref(best))
    assert mask[n] == 9
    if not found:  # nothing but the flag and the count is written
        assert (model == -7.0).all() and (H == -7.0).all() and (mask == 9).all()
        return dict(found=0, model=None, H=None, mask=None, best_count=best.value)
    return dict(found=1, model=model, H=H, mask=mask[:n], best_count=best.value)


def harness_inliers(model, uv_a, uv_b, cam_a, cxq, cyq, thresh=4.0):
    """the header's inlier test under a given model [f, R]: bool [n]"""
    a = np.ascontiguousarray(uv_a, dtype=np.float32).reshape(-1, 2)
    b = np.ascontiguousarray(uv_b, dtype=np.float32).reshape(-1, 2)
    m, cam = np.ascontiguousarray(model, dtype=np.float64), np.ascontiguousarray(cam_a, dtype=np.float64)
    mask = np.full(len(a) + 1, 9, dtype=np.uint8)
    harness().h_rotfocal_inliers.restype = None
    harness().h_rotfocal_inliers(_p(m), len(a), _p(a), _p(b), _p(cam), C.c_double(cxq), C.c_double(cyq), C.c_double(thresh), _p(mask))
    assert mask[-1] == 9
    return mask[:-1].astype(bool)


def harness_batch(match_ptr, uv_a, uv_b, cam_ref, cam_cur, thresh=4.0, iters=128, fill=0):
    """the estimator's outputs of a CSR of queries; model / H / mask of a query without a model keep `fill`"""
    ptr = np.ascontiguousarray(match_ptr, dtype=np.int64)
    a = np.ascontiguousarray(uv_a, dtype=np.float32).reshape(-1, 2)
    b = np.ascontiguousarray(uv_b, dtype=np.float32).reshape(-1, 2)
    cr = np.ascontiguousarray(cam_ref, dtype=np.float64).reshape(-1, 15)
    cc = np.ascontiguousarray(cam_cur, dtype=np.float64).reshape(-1, 15)
    nq = len(ptr) - 1
    model, H = np.full((nq, 10), float(fill)), np.full((nq, 9), float(fill))
    found, best = np.zeros(nq, dtype=np.int32), np.zeros(nq, dtype=np.int32)
    mask = np.full(max(len(a), 1), fill, dtype=np.uint8)
    harness().h_rotfocal_batch(nq, _p(ptr), _p(a), _p(b), _p(cr), _p(cc), C.c_double(thresh), int(iters), _p(model), _p(H), _p(found), _p(mask),
                               _p(best))
    return dict(model=model, H=H, found=found, mask=mask[:len(a)], best_count=best)


def compact(match_ptr, found, mask, uv_a, uv_b, min_inliers):
    """the gate's integer stages: a query passes with found = 1 and at least max(min_inliers, 4) mask ones and keeps those matches in
    their order.  (out_ptr, out_uv_a, out_uv_b, out_index)"""
    ptr = np.asarray(match_ptr, dtype=np.int64)
    a, b = np.asarray(uv_a, dtype=np.float32).reshape(-1, 2), np.asarray(uv_b, dtype=np.float32).reshape(-1, 2)
    need = max(int(min_inliers), 4)
    keep = []
    cnt = np.zeros(len(ptr) - 1, dtype=np.int64)
    for p in range(len(ptr) - 1):
        if found[p] != 1:
            continue
        idx = ptr[p] + np.flatnonzero(mask[ptr[p]:ptr[p + 1]])
        if len(idx) >= need:
            keep.append(idx)
            cnt[p] = len(idx)
    idx = np.concatenate(keep).astype(np.int32) if keep else np.zeros(0, dtype=np.int32)
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), a[idx], b[idx], idx


# ---- the generator -----------------------------------------------------------------------------------------------------------------------
def rot(tilt, pan, roll):
    cx, sx, cy, sy, cz, sz = np.cos(tilt), np.sin(tilt), np.cos(pan), np.sin(pan), np.cos(roll), np.sin(roll)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


def to_anchor(ub, f, R, cam_a, cxq, cyq):
    """the anchor's pixels of the query pixels ub [n, 2] of a query with focal f and rotation R against the anchor"""
    ub = np.asarray(ub, dtype=np.float64).reshape(-1, 2)
    ray = np.stack([(ub[:, 0] - cxq) / f, (ub[:, 1] - cyq) / f, np.ones(len(ub))], axis=1) @ R  # R^T b: the anchor frame's ray, row by row
    return np.stack([cam_a[0] * ray[:, 0] / ray[:, 2] + cam_a[2], cam_a[1] * ray[:, 1] / ray[:, 2] + cam_a[3]], axis=1)


def make_query(n, wrong_share, seed, cam_a=VIRTUAL, w=1920, h=1080, noise=0.5, f_range=(0.75, 4.0 / 3.0)):
    """One assembled query: n matches between the anchor cam_a and a w x h query of focal f_true rotated against the anchor by up to
    30 degrees of pan, 10 of tilt and 1 of roll; `noise` px of Gaussian noise in both images; a share of the matches made wrong by
    replacing the query pixel with a uniform random one.  f_true is drawn from f_range times the anchor's fx: the anchor of an assembled
    query is a view of the same rig at a comparable zoom, and a pixel of anchor noise is f_true / fx pixels in the query (more off axis),
    so that a query zoomed far beyond its anchor would put true matches outside a 4 px threshold by its noise alone.  dict(uv_a, uv_b float32 [n, 2], wrong bool [n], f_true, R_true, cxq, cyq)"""
    rng = np.random.default_rng([seed, n, int(round(1000 * wrong_share))])
    f = cam_a[0] * rng.uniform(*f_range)
    R = rot(np.radians(rng.uniform(-10, 10)), np.radians(rng.uniform(-30, 30)), np.radians(rng.uniform(-1, 1)))
    cxq, cyq = 0.5 * w, 0.5 * h
    ub = rng.uniform([0, 0], [w, h], (n, 2))
    ua = to_anchor(ub, f, R, cam_a, cxq, cyq) + rng.normal(0, noise, (n, 2))
    ub = ub + rng.normal(0, noise, (n, 2))
    wrong = rng.random(n) < wrong_share
    ub[wrong] = rng.uniform([0, 0], [w, h], (int(wrong.sum()), 2))
    return dict(uv_a=ua.astype(np.float32), uv_b=ub.astype(np.float32), wrong=wrong, f_true=f, R_true=R, cxq=cxq, cyq=cyq)


def make_batch(sizes, seed, cam_a=VIRTUAL, wrong_share=0.3):
    """a CSR of queries of the given sizes: (match_ptr, uv_a, uv_b, cam_ref [nq, 15], cam_cur [nq, 15], wrong)"""
    qs = [make_query(n, wrong_share, seed + 17 * k, cam_a=cam_a) for k, n in enumerate(sizes)]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cam_ref = np.tile(np.asarray(cam_a, dtype=np.float64), (len(sizes), 1))
    cam_cur = np.zeros((len(sizes), 15))
    cam_cur[:, 0] = cam_cur[:, 1] = 2000.0
    cam_cur[:, 2] = [q["cxq"] for q in qs]
    cam_cur[:, 3] = [q["cyq"] for q in qs]
    cat = lambda k, dt: np.concatenate([q[k] for q in qs]).astype(dt) if qs else np.zeros((0, 2), dtype=dt)
    return ptr, cat("uv_a", np.float32).reshape(-1, 2), cat("uv_b", np.float32).reshape(-1, 2), cam_ref, cam_cur, cat("wrong", bool).reshape(-1)
