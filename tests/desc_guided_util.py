"""The guided matcher's contract (ptz-calib_amd/csrc/ptz_desc_match.h, desc_guide_*) restated in numpy: the warp in float64 with
every product and sum rounded on its own, the admissibility test in float32 with three roundings, then the rules of
desc_match_util over the admissible candidates only.  The yardstick of the CPU harness and of the device's guided pass; nothing
here is shared with either."""
from __future__ import annotations

import ctypes as C

import numpy as np

import desc_match_util as du

INT32_MAX = du.INT32_MAX
_BIG = np.iinfo(np.int64).max
SIZES = (1, 2, 15, 16, 17, 63, 64, 65, 257)
WG_QUERIES = 256   # queries of a workgroup of k_desc_top2_guided (DESC_WG)
LDS_TILE = 1024    # positions it stages at a time (DESC_G_TILE)


def warp(H, xy):
    """(wx float32 [n], wy float32 [n], ok bool [n]) of float32 points xy [n, 2] under H (9 float64, b ~ H a)."""
    H = np.asarray(H, dtype=np.float64).reshape(9)
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    x = xy[:, 0].astype(np.float64)
    y = xy[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        X = H[0] * x + H[1] * y + H[2]
        Y = H[3] * x + H[4] * y + H[5]
        Z = H[6] * x + H[7] * y + H[8]
        ok = (Z > 0) & np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
        return (X / Z).astype(np.float32), (Y / Z).astype(np.float32), ok


def r2f_of(radius_px):
    return np.float32(float(radius_px) * float(radius_px))


def admissible(H, kp_a, kp_b, radius_px):
    """bool [n_a, n_b]: ok(i) and |warp(a_i) - b_j|^2 <= (float32)(radius^2), in float32 without fma."""
    wx, wy, ok = warp(H, kp_a)
    b = np.asarray(kp_b, dtype=np.float32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        dx = wx[:, None] - b[None, :, 0]
        dy = wy[:, None] - b[None, :, 1]
        e2 = dx * dx + dy * dy
        assert e2.dtype == np.float32
        return ok[:, None] & (e2 <= r2f_of(radius_px))


def top2_masked(d2, adm):
    """du.top2 over the admissible entries of each row; (INT32_MAX, INT32_MAX, INT32_MAX) for a row without any."""
    n, m = d2.shape
    f = np.full(n, INT32_MAX, dtype=np.int64)
    if m == 0:
        return f, f.copy(), f.copy()
    x = np.where(adm, d2, _BIG)
    rows = np.arange(n)
    j = np.argmin(x, axis=1)  # the first of equal minima: the lowest j
    d = x[rows, j]
    x[rows, j] = _BIG
    s = x.min(axis=1)
    none = d == _BIG
    return np.where(none, INT32_MAX, d), np.where(none, INT32_MAX, j).astype(np.int64), np.where(s == _BIG, INT32_MAX, s)


def pair_top2(a, b, kp_a, kp_b, H, radius_px):
    """(d_a, j_a, s_a, d_b, j_b, s_b): both directions over ONE admissible set."""
    d2 = du.dist2(a, b)
    adm = admissible(H, kp_a, kp_b, radius_px)
    return top2_masked(d2, adm) + top2_masked(d2.T.copy(), adm.T)


def accept(t, ratio=0.8, max_dist2=0, cross_check=True, min_matches=0):
    """du.accept for states that may be empty (best j = INT32_MAX)."""
    e = np.zeros(0, dtype=np.int64)
    if t is None:
        return e, e.copy(), e.copy()
    da, ja, sa, db, jb, sb = t
    r2 = float(ratio) * float(ratio)
    i = np.arange(len(da))
    ok = ja != INT32_MAX
    if len(db) == 0 or len(da) == 0:
        return e, e.copy(), e.copy()
    js = np.where(ok, ja, 0)
    if cross_check:
        ok &= jb[js] == i
    if ratio > 0:
        ok &= da.astype(np.float64) < r2 * sa.astype(np.float64)
        if cross_check:
            ok &= da.astype(np.float64) < r2 * sb[js].astype(np.float64)
    if max_dist2 != 0:
        ok &= da <= max_dist2
    if ok.sum() < min_matches:
        return e, e.copy(), e.copy()
    return i[ok], ja[ok], da[ok]


def match_pairs_guided(desc_a, ptr_a, kp_a, desc_b, ptr_b, kp_b, img_a, img_b, H, found=None, radius_px=4.0, cache=None, **opt):
    """CSR of a batch in the layout api.match_descriptors_guided returns: match_ptr, idx_a, idx_b, dist2, uv_a, uv_b.
    cache: a dict keeping the pairs' top-2 between calls with the same images, H and radius (the options do not enter it)."""
    H = np.asarray(H, dtype=np.float64).reshape(-1, 9)
    kp_a = np.asarray(kp_a, dtype=np.float32).reshape(-1, 2)
    kp_b = np.asarray(kp_b, dtype=np.float32).reshape(-1, 2)
    ptr = [0]
    ia, ib, dd, ua, ub = [], [], [], [], []
    for p, (x, y) in enumerate(zip(img_a, img_b)):
        sa, sb = slice(int(ptr_a[x]), int(ptr_a[x + 1])), slice(int(ptr_b[y]), int(ptr_b[y + 1]))
        key = (int(x), int(y), H[p].tobytes(), float(radius_px))
        t = None
        if (found is None or int(found[p]) == 1) and sa.stop > sa.start and sb.stop > sb.start:
            if cache is not None and key in cache:
                t = cache[key]
            else:
                t = pair_top2(desc_a[sa], desc_b[sb], kp_a[sa], kp_b[sb], H[p], radius_px)
                if cache is not None:
                    cache[key] = t
        i, j, d = accept(t, **opt)
        ia.append(i); ib.append(j); dd.append(d)
        ua.append(kp_a[sa][i]); ub.append(kp_b[sb][j])
        ptr.append(ptr[-1] + len(i))
    cat = lambda v: np.concatenate(v).astype(np.int32) if v else np.zeros(0, dtype=np.int32)
    cat2 = lambda v: np.concatenate(v).astype(np.float32).reshape(-1, 2) if v else np.zeros((0, 2), dtype=np.float32)
    return dict(match_ptr=np.asarray(ptr, dtype=np.int64), idx_a=cat(ia), idx_b=cat(ib), dist2=cat(dd), uv_a=cat2(ua), uv_b=cat2(ub))


KEYS = ("match_ptr", "idx_a", "idx_b", "dist2", "uv_a", "uv_b")


def assert_equal(got, want, what=""):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k)


# ------------------------------------------------------------------------------------------------------- the two-pass flow
def host_homography(host_lib, uv_a, uv_b, thresh=4.0):
    """The project's host estimator (FindHomographyRansac through the host library): (found, H [9], mask uint8 [n])."""
    a = np.ascontiguousarray(uv_a, dtype=np.float32)
    b = np.ascontiguousarray(uv_b, dtype=np.float32)
    H = np.zeros(9, dtype=np.float64)
    H[[0, 4, 8]] = 1.0
    mask = np.zeros(max(len(a), 1), dtype=np.uint8)
    host_lib.ptzh_find_homography.restype = C.c_int32
    found = host_lib.ptzh_find_homography(len(a), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.c_double(thresh),
                                          H.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p))
    return int(found), H, mask[:len(a)]


def pair_models(host_lib, first, kp_a, ptr_a, kp_b, ptr_b, img_a, img_b, ransac_thresh=4.0, min_inliers=6):
    """(H [n_pair, 9], found int32 [n_pair]) for the guided pass from a first pass's CSR: found = 1 where the pair's RANSAC
    homography exists and has at least max(min_inliers, 4) mask-1 matches -- the gate's rule."""
    n = len(img_a)
    H = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.float64), (n, 1))
    found = np.zeros(n, dtype=np.int32)
    for p, (x, y) in enumerate(zip(img_a, img_b)):
        sl = slice(int(first["match_ptr"][p]), int(first["match_ptr"][p + 1]))
        if sl.stop - sl.start < 4:
            continue
        ua = kp_a[int(ptr_a[x]) + first["idx_a"][sl]]
        ub = kp_b[int(ptr_b[y]) + first["idx_b"][sl]]
        f, h, mask = host_homography(host_lib, ua, ub, ransac_thresh)
        if f == 1 and int(mask.sum()) >= max(min_inliers, 4):
            found[p], H[p] = 1, h
    return H, found


def two_pass(host_lib, desc_a, ptr_a, kp_a, desc_b, ptr_b, kp_b, img_a, img_b, radius_px=4.0, ransac_thresh=4.0, min_inliers=6, **opt):
    """(first pass, H, found, guided pass): what MatchDescriptors computes with guided_radius > 0."""
    first = du.match_pairs(desc_a, ptr_a, desc_b, ptr_b, img_a, img_b, **opt)
    H, found = pair_models(host_lib, first, kp_a, ptr_a, kp_b, ptr_b, img_a, img_b, ransac_thresh, min_inliers)
    return first, H, found, match_pairs_guided(desc_a, ptr_a, kp_a, desc_b, ptr_b, kp_b, img_a, img_b, H, found, radius_px, **opt)


def table_score(csr, img_a, img_b, table):
    """(matches, matches that are in the table, table matches of the listed pairs): table = {(s, d): set of (q, t)}."""
    n = hit = 0
    for p, (x, y) in enumerate(zip(np.asarray(img_a).tolist(), np.asarray(img_b).tolist())):
        sl = slice(int(csr["match_ptr"][p]), int(csr["match_ptr"][p + 1]))
        got = set(zip(csr["idx_a"][sl].tolist(), csr["idx_b"][sl].tolist()))
        n += len(got)
        hit += len(got & table.get((x, y), set()))
    return n, hit, sum(len(table.get((x, y), ())) for x, y in zip(np.asarray(img_a).tolist(), np.asarray(img_b).tolist()))


# ------------------------------------------------------------------------------------------------ data sets of the chain tests
REPEAT = dict(D=128, noise=12, n_distractors=50, repeat_share=0.7, repeat_group=4, repeat_noise=6)


def repeated_reloc(pkg, root, n_query=24, n_match=96, D=128, noise=12, n_distractors=40, repeat_share=0.7, repeat_group=4, repeat_noise=6):
    """du.chain_reloc with repeated descriptors: of a query's matches, repeat_share (at random) are put in groups of repeat_group
    that share one base descriptor, each member with a perturbation of its own.  Returns (batch, (ptr, desc, kp) of the references,
    (ptr, desc, kp) of the tests, paths)."""
    rb = pkg.synth.make_reloc_batch(n_query, n_match, seed_id=6, factor_type=0)
    paths = pkg.dataset_io.write_reloc_set(root, rb)
    rng = np.random.default_rng(17)
    base = rng.integers(0, 256, (len(rb.uv_ref), D))
    for q in range(n_query):
        lo, hi = int(rb.match_ptr[q]), int(rb.match_ptr[q + 1])
        n_rep = int(repeat_share * (hi - lo)) // repeat_group * repeat_group
        groups = lo + rng.permutation(hi - lo)[:n_rep].reshape(-1, repeat_group)
        if len(groups):
            base[groups] = np.clip(base[groups[:, 0]][:, None, :] + rng.integers(-repeat_noise, repeat_noise + 1, (len(groups), repeat_group, D)), 0, 255)
    out = []
    for uv, names, d in ((rb.uv_ref, paths["ref_names"], paths["ref_features"]), (rb.uv_cur, paths["test_names"], paths["test_features"])):
        descs, kps = [], []
        for q in range(n_query):
            sl = slice(int(rb.match_ptr[q]), int(rb.match_ptr[q + 1]))
            descs += [np.clip(base[sl] + rng.integers(-noise, noise + 1, (sl.stop - sl.start, D)), 0, 255).astype(np.uint8),
                      rng.integers(0, 256, (n_distractors, D), dtype=np.uint8)]
            kps += [np.asarray(uv[sl], dtype=np.float32), rng.uniform([0, 0], [1920, 1080], (n_distractors, 2)).astype(np.float32)]
        ptr = (np.asarray(rb.match_ptr, dtype=np.int64) + n_distractors * np.arange(n_query + 1)).astype(np.int64)
        desc, kp = np.concatenate(descs), np.concatenate(kps)
        pkg.dataset_io.write_features(d, names, ptr, kp, desc=desc)
        out.append((ptr, desc, kp))
    return rb, out[0], out[1], paths


def repeated_rig(pkg, root=None):
    """The 20-view x 100 rig with repeated descriptors: (scene, table, feat_ptr, desc, key points, paths or None)."""
    sc = pkg.synth.add_annotations(pkg.synth.make_scene(0, 20, 100))
    tb = pkg.synth.make_match_table(sc, min_pair_matches=8)
    ptr, desc, kp = pkg.synth.make_repeated_descriptors(sc, seed=7, **REPEAT)
    paths = None
    if root is not None:
        paths = pkg.dataset_io.write_rig(root, sc, tb, annotations=sc.obs3d)
        pkg.dataset_io.write_features(paths["features"], paths["names"], ptr, kp, desc=desc)
    return sc, tb, ptr, desc, kp, paths
