"""The assembly's contract (ptz-calib_amd/csrc/ptz_reloc_assemble.h) restated in numpy: the ranking as a stable sort, the transfer
in float64 with every product and sum rounded on its own and in the header's order, the cameras.  The yardstick of the CPU harness
(tests/cpu_harness/reloc_assemble_harness.cc) and, through it, of the device; nothing here is shared with either.  Every figure is
reproduced bit for bit: the transferred pixels are compared array-equal, no ulp bound is needed."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 8192.0
KEYS = ("sel_pair", "n_sel", "match_ptr", "uv_ref", "uv_cur", "src", "cam_ref", "cam_init")
_h = None


def rodrigues(r):
    """ptz_factor.h's rodrigues, operation for operation (python floats are IEEE doubles)."""
    r0, r1, r2 = float(r[0]), float(r[1]), float(r[2])
    theta = math.sqrt(r0 * r0 + r1 * r1 + r2 * r2)
    if theta < 2.220446049250313e-16:
        return np.eye(3).reshape(9)
    c, s = math.cos(theta), math.sin(theta)
    c1, it = 1.0 - c, 1.0 / theta
    x, y, z = r0 * it, r1 * it, r2 * it
    return np.array([c + c1 * x * x, c1 * x * y - s * z, c1 * x * z + s * y,
                     c1 * x * y + s * z, c + c1 * y * y, c1 * y * z - s * x,
                     c1 * x * z - s * y, c1 * y * z + s * x, c + c1 * z * z])


def rotations(ref_cams):
    return np.stack([rodrigues(c[4:7]) for c in np.asarray(ref_cams, dtype=np.float64).reshape(-1, 15)]).reshape(-1, 9)


def undistort(cam, u, v):
    """ptz_factor.h's undistort_point for float32 arrays u, v: (ou, ov) float32."""
    fx, fy, cx, cy = (float(cam[k]) for k in range(4))
    d = [float(cam[10 + k]) for k in range(5)]
    ifx, ify = 1.0 / fx, 1.0 / fy
    u64, v64 = u.astype(np.float64), v.astype(np.float64)
    with np.errstate(all="ignore"):
        x = (u64 - cx) * ifx
        y = (v64 - cy) * ify
        x0, y0 = x.copy(), y.copy()
        done = np.zeros(len(x), dtype=bool)
        for _ in range(5):
            r2 = x * x + y * y
            icdist = 1.0 / (1 + ((d[4] * r2 + d[1]) * r2 + d[0]) * r2)
            stop = ~done & (icdist < 0)
            dX = 2 * d[2] * x * y + d[3] * (r2 + 2 * x * x)
            dY = d[2] * (r2 + 2 * y * y) + 2 * d[3] * x * y
            nx = np.where(stop, x0, (x0 - dX) * icdist)
            ny = np.where(stop, y0, (y0 - dY) * icdist)
            x = np.where(done, x, nx)
            y = np.where(done, y, ny)
            done |= stop
        return (x * fx + cx).astype(np.float32), (y * fy + cy).astype(np.float32)


def transfer(cam_r, R_r, R_a, fa, dist, uv):
    """steps 1 - 5 for the float32 pixels uv [n, 2] of reference r: (pixels float32 [n, 2], keep bool [n])."""
    uv = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
    cam_r = np.asarray(cam_r, dtype=np.float64)
    ou, ov = uv[:, 0].copy(), uv[:, 1].copy()
    keep = np.ones(len(uv), dtype=bool)
    with np.errstate(all="ignore"):
        if dist:
            ou, ov = undistort(cam_r, ou, ov)
            keep &= ~((ou < 0) | (ou >= cam_r[2] * 2) | (ov < 0) | (ov >= cam_r[3] * 2))
        nx = (ou.astype(np.float64) - cam_r[2]) / cam_r[0]
        ny = (ov.astype(np.float64) - cam_r[3]) / cam_r[1]
        w0 = R_r[0] * nx + R_r[3] * ny + R_r[6]
        w1 = R_r[1] * nx + R_r[4] * ny + R_r[7]
        w2 = R_r[2] * nx + R_r[5] * ny + R_r[8]
        mx = R_a[0] * w0 + R_a[1] * w1 + R_a[2] * w2
        my = R_a[3] * w0 + R_a[4] * w1 + R_a[5] * w2
        mz = R_a[6] * w0 + R_a[7] * w1 + R_a[8] * w2
        keep &= (mz > 0) & np.isfinite(mx) & np.isfinite(my) & np.isfinite(mz)
        up = (fa * (mx / mz) + S).astype(np.float32)
        vp = (fa * (my / mz) + S).astype(np.float32)
        lim = np.float32(2 * S)
        keep &= (up >= 0) & (up < lim) & (vp >= 0) & (vp < lim)
    return np.stack([up, vp], axis=1), keep


def select(counts, K):
    """positions of the first K pairs of a list by (count descending, position ascending), pairs without matches left out."""
    counts = np.asarray(counts, dtype=np.int64)
    order = np.argsort(-counts, kind="stable")
    return [int(j) for j in order if counts[j] > 0][:K]


def cameras(anchor, w, h, K):
    anchor = np.asarray(anchor, dtype=np.float64)
    cur = anchor.copy()
    cur[1] = anchor[0]
    cur[2], cur[3] = 0.5 * w, 0.5 * h
    if K == 1:
        return anchor.copy(), cur
    ref = np.zeros(15)
    ref[0] = ref[1] = anchor[0]
    ref[2] = ref[3] = S
    ref[4:10] = anchor[4:10]
    return ref, cur


def assemble(match_ptr, uv_ref, uv_cur, pair_ref, query_ptr, ref_cams, query_wh, factor_type=0, max_refs=1, ref_R=None):
    """The dict api.reloc_assemble returns (without device_ms)."""
    ptr = np.asarray(match_ptr, dtype=np.int64)
    a = np.asarray(uv_ref, dtype=np.float32).reshape(-1, 2)
    b = np.asarray(uv_cur, dtype=np.float32).reshape(-1, 2)
    cams = np.asarray(ref_cams, dtype=np.float64).reshape(-1, 15)
    R = rotations(cams) if ref_R is None else np.asarray(ref_R, dtype=np.float64).reshape(-1, 9)
    wh = np.asarray(query_wh).reshape(-1, 2)
    K, nq = int(max_refs), len(query_ptr) - 1
    sel = np.full((nq, K), -1, dtype=np.int32)
    nsel = np.zeros(nq, dtype=np.int32)
    optr = [0]
    oa, ob, osrc = [], [], []
    cref, ccur = np.zeros((nq, 15)), np.zeros((nq, 15))
    for q in range(nq):
        lo, hi = int(query_ptr[q]), int(query_ptr[q + 1])
        pos = select(np.diff(ptr[lo:hi + 1]), K)
        nsel[q] = len(pos)
        sel[q, :len(pos)] = [lo + j for j in pos]
        r0 = int(pair_ref[lo + pos[0]]) if pos else (int(pair_ref[lo]) if hi > lo else 0)
        cref[q], ccur[q] = cameras(cams[r0], int(wh[q, 0]), int(wh[q, 1]), K)
        n = 0
        for j in pos:
            p = lo + j
            idx = np.arange(int(ptr[p]), int(ptr[p + 1]))
            r = int(pair_ref[p])
            if K == 1:
                px, keep = a[idx], np.ones(len(idx), dtype=bool)
            else:
                px, keep = transfer(cams[r], R[r], R[r0], cams[r0, 0], factor_type & 1, a[idx])
            oa.append(px[keep]); ob.append(b[idx[keep]]); osrc.append(idx[keep])
            n += int(keep.sum())
        optr.append(optr[-1] + n)
    cat2 = lambda v: np.concatenate(v).astype(np.float32).reshape(-1, 2) if v else np.zeros((0, 2), dtype=np.float32)
    return dict(sel_pair=sel, n_sel=nsel, match_ptr=np.asarray(optr, dtype=np.int64), uv_ref=cat2(oa), uv_cur=cat2(ob),
                src=np.concatenate(osrc).astype(np.int32) if osrc else np.zeros(0, dtype=np.int32), cam_ref=cref, cam_init=ccur)


# ------------------------------------------------------------------------------------------------------------ the host harness
def harness():
    global _h
    if _h is None:
        _h = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "libreloc_assemble_harness.so"))
        _h.h_reloc_assemble.restype = C.c_int64
        _h.h_reloc_rotations.restype = None
    return _h


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness_rotations(ref_cams):
    cams = np.ascontiguousarray(ref_cams, dtype=np.float64).reshape(-1, 15)
    R = np.zeros((len(cams), 9))
    harness().h_reloc_rotations(len(cams), _p(cams), _p(R))
    return R


def harness_assemble(match_ptr, uv_ref, uv_cur, pair_ref, query_ptr, ref_cams, query_wh, factor_type=0, max_refs=1, ref_R=None):
    ptr = np.ascontiguousarray(match_ptr, dtype=np.int64)
    a = np.ascontiguousarray(uv_ref, dtype=np.float32).reshape(-1, 2)
    b = np.ascontiguousarray(uv_cur, dtype=np.float32).reshape(-1, 2)
    pref = np.ascontiguousarray(pair_ref, dtype=np.int32)
    qptr = np.ascontiguousarray(query_ptr, dtype=np.int64)
    cams = np.ascontiguousarray(ref_cams, dtype=np.float64).reshape(-1, 15)
    wh = np.ascontiguousarray(query_wh, dtype=np.int32).reshape(-1, 2)
    R = harness_rotations(cams) if ref_R is None else np.ascontiguousarray(ref_R, dtype=np.float64).reshape(-1, 9)
    nq, nm, K = len(qptr) - 1, len(a), int(max_refs)
    sel = np.full((nq, K), -1, dtype=np.int32)
    nsel = np.zeros(nq, dtype=np.int32)
    optr = np.zeros(nq + 1, dtype=np.int64)
    oa, ob = np.zeros((max(nm, 1), 2), dtype=np.float32), np.zeros((max(nm, 1), 2), dtype=np.float32)
    osrc = np.zeros(max(nm, 1), dtype=np.int32)
    cref, ccur = np.zeros((nq, 15)), np.zeros((nq, 15))
    k = harness().h_reloc_assemble(nq, len(ptr) - 1, len(cams), _p(ptr), _p(a), _p(b), _p(pref), _p(qptr), _p(cams), _p(R), _p(wh),
                                   int(factor_type), K, _p(sel), _p(nsel), _p(optr), _p(oa), _p(ob), _p(osrc), _p(cref), _p(ccur))
    return dict(sel_pair=sel, n_sel=nsel, match_ptr=optr, uv_ref=oa[:k], uv_cur=ob[:k], src=osrc[:k], cam_ref=cref, cam_init=ccur)


def assert_equal(got, want, what=""):
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, k)


# ------------------------------------------------------------------------------------------------------------------ test data
def make_rig(dist, seed=0):
    """Twelve references on one centre: ten around pan 0 (5 degrees apart, three tilts), one 75 degrees away (its pixels leave the
    virtual frame of an anchor near pan 0) and one behind (pan 180)."""
    rng = np.random.default_rng(seed)
    pans = list(np.arange(-25, 25, 5.0)) + [75.0, 180.0]
    cams = np.zeros((len(pans), 15))
    for i, pan in enumerate(pans):
        a, t = math.radians(pan + rng.uniform(-0.3, 0.3)), math.radians([-8.0, 0.0, 8.0][i % 3])
        cams[i, 0] = cams[i, 1] = rng.uniform(1800, 3200)
        cams[i, 2], cams[i, 3] = 960.0, 540.0
        cams[i, 4:7] = [t, a, 0.01 * i]  # (any rotation vector serves: the assembly takes them as they are)
        cams[i, 7:10] = rng.uniform(-1, 1, 3)
        if dist:
            cams[i, 10] = rng.uniform(-0.05, 0.05)
            cams[i, 11:15] = rng.uniform(-1e-3, 1e-3, 4)
    return cams


def make_csr(list_lens, counts_of, n_ref, seed=0, width=1920, height=1080, refs_of=None):
    """A synthetic match table: query q has list_lens[q] pairs, pair j of it counts_of(q, j) matches and reference refs_of(q, j)
    (default: drawn at random, so a reference may appear twice in a list); pixels uniform over a frame 40 px larger than the image
    on every side, so that some fall outside the border guard."""
    rng = np.random.default_rng(seed)
    qptr = np.concatenate([[0], np.cumsum(list_lens)]).astype(np.int64)
    counts, pref = [], []
    for q, n in enumerate(list_lens):
        for j in range(n):
            counts.append(int(counts_of(q, j)))
            pref.append(int(refs_of(q, j)) if refs_of else int(rng.integers(0, n_ref)))
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    nm = int(ptr[-1])
    uv_ref = rng.uniform([-40, -40], [width + 40, height + 40], (nm, 2)).astype(np.float32)
    uv_cur = rng.uniform([0, 0], [width, height], (nm, 2)).astype(np.float32)
    wh = np.stack([rng.integers(600, 4000, len(list_lens)), rng.integers(400, 2200, len(list_lens))], axis=1).astype(np.int32)
    return dict(match_ptr=ptr, uv_ref=uv_ref, uv_cur=uv_cur, pair_ref=np.asarray(pref, dtype=np.int32), query_ptr=qptr, query_wh=wh)


def slice_queries(csr, qs):
    """The table of the queries qs (in that order) alone."""
    ptr, qptr = csr["match_ptr"], csr["query_ptr"]
    pairs = np.concatenate([np.arange(qptr[q], qptr[q + 1]) for q in qs]).astype(np.int64) if len(qs) else np.zeros(0, np.int64)
    idx = np.concatenate([np.arange(ptr[p], ptr[p + 1]) for p in pairs]).astype(np.int64) if len(pairs) else np.zeros(0, np.int64)
    return dict(match_ptr=np.concatenate([[0], np.cumsum(np.diff(ptr)[pairs])]).astype(np.int64), uv_ref=csr["uv_ref"][idx],
                uv_cur=csr["uv_cur"][idx], pair_ref=csr["pair_ref"][pairs],
                query_ptr=np.concatenate([[0], np.cumsum(np.diff(qptr)[list(qs)])]).astype(np.int64), query_wh=csr["query_wh"][list(qs)]), idx


def per_query(out, q):
    """The outputs of query q, its src left as it is."""
    sl = slice(int(out["match_ptr"][q]), int(out["match_ptr"][q + 1]))
    return dict(n_sel=out["n_sel"][q], uv_ref=out["uv_ref"][sl], uv_cur=out["uv_cur"][sl], src=out["src"][sl], cam_ref=out["cam_ref"][q],
                cam_init=out["cam_init"][q], sel_pair=out["sel_pair"][q])
