"""The landmark map's contract (ptz-calib_amd/csrc/ptz_landmark.h) restated in numpy: per-view rays in float64 with every product,
sum and sqrt rounded on its own and in the header's order, the ray sum as a cumulative (left to right) sum, the byte means in
integers, the home and anchor searches as first-wins arg-maxes.  The yardstick of the CPU harness
(tests/cpu_harness/landmark_harness.cc) and, through it, of the device; nothing here is shared with either.  Every figure is
reproduced bit for bit: all outputs are compared array-equal, no ulp bound is needed."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import reloc_assemble_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 8192.0
MAP_KEYS = ("lm_track", "lm_ray", "lm_home", "lm_views", "lm_desc")
ASM_KEYS = ("anchor_ref", "match_ptr", "uv_ref", "uv_cur", "src", "cam_ref", "cam_init")
_h = None


# ------------------------------------------------------------------------------------------------------------- the restatement
def feature_rays(feat_ptr, kp, ref_cams, ref_R, dist):
    """(ray float64 [n_feat, 3], ok bool [n_feat]) of every feature of every reference: landmark_view_ray, image by image."""
    kp = np.asarray(kp, dtype=np.float32).reshape(-1, 2)
    ray, ok = np.zeros((len(kp), 3)), np.ones(len(kp), dtype=bool)
    for r in range(len(feat_ptr) - 1):
        sl = slice(int(feat_ptr[r]), int(feat_ptr[r + 1]))
        cam, R = np.asarray(ref_cams[r], dtype=np.float64), np.asarray(ref_R[r], dtype=np.float64)
        ou, ov = kp[sl, 0].copy(), kp[sl, 1].copy()
        with np.errstate(all="ignore"):
            if dist:
                ou, ov = U.undistort(cam, ou, ov)
                ok[sl] = ~((ou < 0) | (ou >= cam[2] * 2) | (ov < 0) | (ov >= cam[3] * 2))
            nx = (ou.astype(np.float64) - cam[2]) / cam[0]
            ny = (ov.astype(np.float64) - cam[3]) / cam[1]
            w0 = R[0] * nx + R[3] * ny + R[6]
            w1 = R[1] * nx + R[4] * ny + R[7]
            w2 = R[2] * nx + R[5] * ny + R[8]
            ln = np.sqrt(w0 * w0 + w1 * w1 + w2 * w2)
            ray[sl] = np.stack([w0 / ln, w1 / ln, w2 / ln], axis=1)
    return ray, ok


def build(feat_ptr, desc, kp, ref_cams, trk_ptr, trk_img, trk_feat, factor_type=0, min_views=1, ref_R=None):
    """The dict api.LandmarkMap.arrays() returns."""
    feat_ptr = np.asarray(feat_ptr, dtype=np.int64)
    desc = np.asarray(desc, dtype=np.uint8)
    cams = np.asarray(ref_cams, dtype=np.float64).reshape(-1, 15)
    R = U.rotations(cams) if ref_R is None else np.asarray(ref_R, dtype=np.float64).reshape(-1, 9)
    n_ref, D = len(cams), desc.shape[1]
    ray, ok = feature_rays(feat_ptr, kp, cams, R, factor_type & 1)
    trk_img, trk_feat = np.asarray(trk_img, dtype=np.int64), np.asarray(trk_feat, dtype=np.int64)
    out = dict(lm_track=[], lm_ray=[], lm_home=[], lm_views=[], lm_desc=[])
    for t in range(len(trk_ptr) - 1):
        img, feat = trk_img[int(trk_ptr[t]):int(trk_ptr[t + 1])], trk_feat[int(trk_ptr[t]):int(trk_ptr[t + 1])]
        valid = (img >= 0) & (img < n_ref)
        rc = np.where(valid, img, 0)
        valid &= (feat >= 0) & (feat < feat_ptr[rc + 1] - feat_ptr[rc])
        row = np.where(valid, feat_ptr[rc] + feat, 0)
        valid &= ok[row]
        img, row = img[valid], row[valid]
        n = len(img)
        if n < max(int(min_views), 1):
            continue
        with np.errstate(all="ignore"):
            s = np.cumsum(np.concatenate([np.zeros((1, 3)), ray[row]]), axis=0)[-1]  # left to right, from (0, 0, 0)
            L = s / np.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2])
            if not np.isfinite(L).all():
                continue
            z = R[img, 6] * L[0] + R[img, 7] * L[1] + R[img, 8] * L[2]
        z = np.where(z > -np.inf, z, -np.inf)
        Sk = desc[row].astype(np.int64).sum(axis=0)
        out["lm_track"].append(t)
        out["lm_ray"].append(L)
        out["lm_home"].append(int(img[int(np.argmax(z))]) if z.max() > -np.inf else int(img[0]))
        out["lm_views"].append(n)
        out["lm_desc"].append(((2 * Sk + n) // (2 * n)).astype(np.uint8))
    return dict(lm_track=np.asarray(out["lm_track"], dtype=np.int32), lm_ray=np.asarray(out["lm_ray"], dtype=np.float64).reshape(-1, 3),
                lm_home=np.asarray(out["lm_home"], dtype=np.int32), lm_views=np.asarray(out["lm_views"], dtype=np.int32),
                lm_desc=np.asarray(out["lm_desc"], dtype=np.uint8).reshape(-1, D))


def transfer(R_a, fa, L):
    """landmark_transfer for rays L [n, 3]: (pixels float32 [n, 2], keep bool [n])."""
    L = np.asarray(L, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        mx = R_a[0] * L[:, 0] + R_a[1] * L[:, 1] + R_a[2] * L[:, 2]
        my = R_a[3] * L[:, 0] + R_a[4] * L[:, 1] + R_a[5] * L[:, 2]
        mz = R_a[6] * L[:, 0] + R_a[7] * L[:, 1] + R_a[8] * L[:, 2]
        keep = (mz > 0) & np.isfinite(mx) & np.isfinite(my) & np.isfinite(mz)
        up = (fa * (mx / mz) + S).astype(np.float32)
        vp = (fa * (my / mz) + S).astype(np.float32)
        lim = np.float32(2 * S)
        keep &= (up >= 0) & (up < lim) & (vp >= 0) & (vp < lim)
    return np.stack([up, vp], axis=1), keep


def assemble(lm, match_ptr, idx_a, uv_b, ref_cams, query_wh, ref_R=None):
    """The dict api.landmark_assemble returns (without device_ms); lm: the map's arrays."""
    ptr = np.asarray(match_ptr, dtype=np.int64)
    ia = np.asarray(idx_a, dtype=np.int64)
    b = np.asarray(uv_b, dtype=np.float32).reshape(-1, 2)
    cams = np.asarray(ref_cams, dtype=np.float64).reshape(-1, 15)
    R = U.rotations(cams) if ref_R is None else np.asarray(ref_R, dtype=np.float64).reshape(-1, 9)
    wh = np.asarray(query_wh).reshape(-1, 2)
    n_ref, n_lm, nq = len(cams), len(lm["lm_home"]), len(ptr) - 1
    anchor = np.full(nq, -1, dtype=np.int32)
    optr, oa, ob, osrc = [0], [], [], []
    cref, ccur = np.zeros((nq, 15)), np.zeros((nq, 15))
    for q in range(nq):
        idx = np.arange(int(ptr[q]), int(ptr[q + 1]))
        l = ia[idx]
        votes = (l >= 0) & (l < n_lm)
        home = np.where(votes, lm["lm_home"][np.where(votes, l, 0)] if n_lm else -1, -1)
        votes &= (home >= 0) & (home < n_ref)
        counts = np.bincount(home[votes], minlength=n_ref)
        a = int(np.argmax(counts)) if counts.max(initial=0) > 0 else -1  # the first of the largest: the lowest index
        anchor[q] = a
        cref[q], ccur[q] = U.cameras(cams[max(a, 0)], int(wh[q, 0]), int(wh[q, 1]), 2)
        n = 0
        if a >= 0:
            idx = idx[votes]
            px, keep = transfer(R[a], cams[a, 0], lm["lm_ray"][ia[idx]])
            oa.append(px[keep]); ob.append(b[idx[keep]]); osrc.append(idx[keep])
            n = int(keep.sum())
        optr.append(optr[-1] + n)
    cat2 = lambda v: np.concatenate(v).astype(np.float32).reshape(-1, 2) if v else np.zeros((0, 2), dtype=np.float32)
    return dict(anchor_ref=anchor, match_ptr=np.asarray(optr, dtype=np.int64), uv_ref=cat2(oa), uv_cur=cat2(ob),
                src=np.concatenate(osrc).astype(np.int32) if osrc else np.zeros(0, dtype=np.int32), cam_ref=cref, cam_init=ccur)


# ------------------------------------------------------------------------------------------------------------ the host harness
def harness():
    global _h
    if _h is None:
        _h = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "liblandmark_harness.so"))
        _h.h_landmark_build.restype = C.c_int32
        _h.h_landmark_assemble.restype = C.c_int64
    return _h


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness_build(feat_ptr, desc, kp, ref_cams, trk_ptr, trk_img, trk_feat, factor_type=0, min_views=1, ref_R=None):
    fp = np.ascontiguousarray(feat_ptr, dtype=np.int64)
    d = np.ascontiguousarray(desc, dtype=np.uint8)
    k = np.ascontiguousarray(kp, dtype=np.float32).reshape(-1, 2)
    cams = np.ascontiguousarray(ref_cams, dtype=np.float64).reshape(-1, 15)
    R = U.harness_rotations(cams) if ref_R is None else np.ascontiguousarray(ref_R, dtype=np.float64).reshape(-1, 9)
    tp = np.ascontiguousarray(trk_ptr, dtype=np.int64)
    ti, tf = np.ascontiguousarray(trk_img, dtype=np.int32), np.ascontiguousarray(trk_feat, dtype=np.int32)
    nt, D = len(tp) - 1, d.shape[1]
    trk, home, views = (np.zeros(max(nt, 1), dtype=np.int32) for _ in range(3))
    ray, od = np.zeros((max(nt, 1), 3)), np.zeros((max(nt, 1), D), dtype=np.uint8)
    n = harness().h_landmark_build(len(cams), _p(fp), _p(d), D, _p(k), _p(cams), _p(R), nt, _p(tp), _p(ti), _p(tf), int(factor_type) & 1,
                                   int(min_views), _p(trk), _p(ray), _p(home), _p(views), _p(od))
    return dict(lm_track=trk[:n], lm_ray=ray[:n], lm_home=home[:n], lm_views=views[:n], lm_desc=od[:n])


def harness_assemble(lm, match_ptr, idx_a, uv_b, ref_cams, query_wh, ref_R=None):
    ptr = np.ascontiguousarray(match_ptr, dtype=np.int64)
    ia = np.ascontiguousarray(idx_a, dtype=np.int32)
    b = np.ascontiguousarray(uv_b, dtype=np.float32).reshape(-1, 2)
    cams = np.ascontiguousarray(ref_cams, dtype=np.float64).reshape(-1, 15)
    R = U.harness_rotations(cams) if ref_R is None else np.ascontiguousarray(ref_R, dtype=np.float64).reshape(-1, 9)
    wh = np.ascontiguousarray(query_wh, dtype=np.int32).reshape(-1, 2)
    ray, home = np.ascontiguousarray(lm["lm_ray"], dtype=np.float64), np.ascontiguousarray(lm["lm_home"], dtype=np.int32)
    nq, nm = len(ptr) - 1, len(ia)
    anchor = np.full(nq, -1, dtype=np.int32)
    optr = np.zeros(nq + 1, dtype=np.int64)
    oa, ob = np.zeros((max(nm, 1), 2), dtype=np.float32), np.zeros((max(nm, 1), 2), dtype=np.float32)
    osrc = np.zeros(max(nm, 1), dtype=np.int32)
    cref, ccur = np.zeros((nq, 15)), np.zeros((nq, 15))
    k = harness().h_landmark_assemble(nq, len(cams), len(home), _p(ptr), _p(ia), _p(b), _p(ray), _p(home), _p(cams), _p(R), _p(wh), _p(anchor),
                                      _p(optr), _p(oa), _p(ob), _p(osrc), _p(cref), _p(ccur))
    return dict(anchor_ref=anchor, match_ptr=optr, uv_ref=oa[:k], uv_cur=ob[:k], src=osrc[:k], cam_ref=cref, cam_init=ccur)


def assert_equal(got, want, keys, what=""):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, k)


# ------------------------------------------------------------------------------------------------------------------ test data
def make_rig(dist, seed=0):
    """reloc_assemble_util.make_rig's twelve references (ten around pan 0, one 75 degrees away, one behind) and a thirteenth with
    the ROTATION of reference 3 and another focal: two views with exactly equal (R_r L)_z, the home tie."""
    cams = U.make_rig(dist, seed)
    twin = cams[3].copy()
    twin[0] = twin[1] = cams[3, 0] * 1.25
    return np.concatenate([cams, twin[None]])


def make_features(n_ref, D, n_feat, seed=0, width=1920, height=1080):
    """n_feat features per reference: random descriptors, pixels uniform over a frame 40 px larger than the image on every side
    (with distortion some undistort outside).  The first four features of every image are fixed for the rounding cases: bytes all 0,
    all 1, all 255, all 254, at the image centre."""
    rng = np.random.default_rng(seed)
    feat_ptr = (np.arange(n_ref + 1) * n_feat).astype(np.int64)
    desc = rng.integers(0, 256, (n_ref * n_feat, D), dtype=np.uint8)
    kp = rng.uniform([-40, -40], [width + 40, height + 40], (n_ref * n_feat, 2)).astype(np.float32)
    for r in range(n_ref):
        for j, v in enumerate((0, 1, 255, 254)):
            desc[r * n_feat + j] = v
            kp[r * n_feat + j] = (0.5 * width + 3 * j, 0.5 * height - 2 * j)
        kp[r * n_feat + 4] = (-35.0, 0.5 * height)  # with distortion: undistorts outside the frame; without: a valid view
        kp[r * n_feat + 5:r * n_feat + 16] = rng.uniform([300, 200], [width - 300, height - 200], (11, 2))  # inside under any distortion here
    return feat_ptr, desc, kp


def make_tracks(n_ref, n_feat, seed=0):
    """The tracks of the build cases, as (trk_ptr, trk_img, trk_feat, names)."""
    rng = np.random.default_rng(seed)
    tracks, names = [], []

    def add(name, views):
        names.append(name)
        tracks.append([(int(i), int(f)) for i, f in views])

    near = list(range(10))  # the references around pan 0
    for n in (1, 2, 3, 63, 64, 65):
        add(f"len{n}", [(rng.choice(near), rng.integers(5, 16)) for _ in range(n)])  # (pixels inside under any distortion: the length holds)
    add("half_up", [(0, 0), (1, 1)])                  # bytes 0 and 1: the mean 0.5 rounds to 1
    add("half_up_254_255", [(0, 3), (1, 2)])          # 254.5 -> 255
    add("three_halves", [(0, 0), (1, 1), (2, 1), (3, 0)])  # 0, 1, 1, 0: the mean 0.5 -> 1
    add("mean0", [(0, 0), (1, 0), (2, 0)])
    add("mean255", [(0, 2), (1, 2)])
    add("all_invalid", [(-1, 0), (n_ref, 0), (0, n_feat), (0, -1)])
    add("one_valid_of_two", [(0, 7), (n_ref + 5, 7)])  # min_views = 2: one short
    add("single", [(2, 9)])
    add("bad_image_inside", [(0, 10), (-3, 10), (1, 10)])
    add("bad_feature_inside", [(0, 11), (1, n_feat + 100), (2, 11)])
    add("outside_with_dist", [(0, 4), (1, 12)])
    add("only_outside_with_dist", [(0, 4)])
    add("home_tie_twin_first", [(12, 0), (3, 0)])     # the same rotation twice: equal z, the first view wins
    add("home_tie_twin_last", [(3, 0), (12, 0)])
    add("empty", [])
    add("behind", [(11, 0)])                          # a landmark behind every anchor near pan 0
    add("far", [(10, 0)])                             # 75 degrees away: its pixel leaves [0, 2S)
    for _ in range(40):
        add("bulk", [(rng.choice(near), rng.integers(5, n_feat)) for _ in range(int(rng.integers(1, 6)))])
    trk_ptr = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    flat = [v for t in tracks for v in t]
    return (trk_ptr, np.asarray([v[0] for v in flat], dtype=np.int32), np.asarray([v[1] for v in flat], dtype=np.int32), names)


def make_queries(lm, names, counts, seed=0, width=1920, height=1080):
    """A match CSR against the map lm (its arrays; names: make_tracks's): query q has counts[q] matches to landmarks drawn at
    random, among them the one behind and the one far away; then one query built by hand of the landmark behind, the one far away
    and up to five whose home is reference 4 (pan -5 degrees: its anchor, 80 degrees from the far landmark, so that one is in front
    with its pixel beyond 2S while the other is behind: each dropping rule meets its own landmark); the last two queries are anchor
    ties, built by hand."""
    rng = np.random.default_rng(seed)
    n_lm = len(lm["lm_home"])
    ptr, ia = [0], []
    for c in counts:
        ia.append(rng.integers(0, n_lm, c))
        ptr.append(ptr[-1] + c)
    # an anchor tie between two references: as many matches of home A as of home B, the higher reference first
    homes = np.unique(lm["lm_home"])
    a, b = int(homes[0]), int(homes[1])
    la, lb = np.nonzero(lm["lm_home"] == a)[0], np.nonzero(lm["lm_home"] == b)[0]
    k = min(len(la), len(lb), 3)
    at = {names[t]: i for i, t in enumerate(lm["lm_track"].tolist()) if names[t] in ("behind", "far")}
    own = np.nonzero(lm["lm_home"] == 4)[0][:5]
    assert len(own) >= 2, "the hand-made query needs two landmarks of reference 4 to outvote the two it drops"
    for hand in (np.concatenate([[at["behind"], at["far"]], own]),):
        ia.append(hand)
        ptr.append(ptr[-1] + len(hand))
    for tie in (np.concatenate([lb[:k], la[:k]]), np.concatenate([la[:k], lb[:k]])):
        ia.append(tie)
        ptr.append(ptr[-1] + len(tie))
    ia = np.concatenate(ia).astype(np.int32) if ia else np.zeros(0, np.int32)
    nq = len(ptr) - 1
    uv_b = rng.uniform([0, 0], [width, height], (len(ia), 2)).astype(np.float32)
    wh = np.stack([rng.integers(600, 4000, nq), rng.integers(400, 2200, nq)], axis=1).astype(np.int32)
    return dict(match_ptr=np.asarray(ptr, dtype=np.int64), idx_a=ia, uv_b=uv_b, query_wh=wh)


def slice_queries(csr, qs):
    """The CSR of the queries qs (in that order) alone, and the input index of each of its matches."""
    ptr = csr["match_ptr"]
    idx = np.concatenate([np.arange(ptr[q], ptr[q + 1]) for q in qs]).astype(np.int64) if len(qs) else np.zeros(0, np.int64)
    return dict(match_ptr=np.concatenate([[0], np.cumsum(np.diff(ptr)[list(qs)])]).astype(np.int64), idx_a=csr["idx_a"][idx],
                uv_b=csr["uv_b"][idx], query_wh=csr["query_wh"][list(qs)]), idx


def per_query(out, q):
    """The outputs of query q, its src left as it is."""
    sl = slice(int(out["match_ptr"][q]), int(out["match_ptr"][q + 1]))
    return dict(anchor_ref=out["anchor_ref"][q], uv_ref=out["uv_ref"][sl], uv_cur=out["uv_cur"][sl], src=out["src"][sl], cam_ref=out["cam_ref"][q],
                cam_init=out["cam_init"][q])
