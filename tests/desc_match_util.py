"""The descriptor matcher's contract (ptz-calib_amd/csrc/ptz_desc_match.h) restated in numpy, int64 throughout: brute-force
distances, top-2 with the lowest index on ties, the acceptance rule, min_matches.  The yardstick of the CPU harness and of the
device matcher; nothing here is shared with either."""
from __future__ import annotations

import numpy as np

INT32_MAX = 2**31 - 1
SIZES = (1, 2, 15, 16, 17, 63, 64, 65, 130, 257)
DIMS = (1, 32, 64, 96, 128, 130, 256, 512)
MATCH_DIMS = DIMS + (300, 350, 400)  # + one D behind each k-step count that the listed ones leave out (5, 6 and 7 steps of 64)


def dist2(a, b):
    """d2 [n_a, n_b] int64 of uint8 descriptors a [n_a, D], b [n_b, D]."""
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)


def top2(d2):
    """(best d2, best j, second d2) per row of d2 [n, m]; (INT32_MAX, INT32_MAX, INT32_MAX) if m == 0."""
    n, m = d2.shape
    if m == 0:
        f = np.full(n, INT32_MAX, dtype=np.int64)
        return f, f.copy(), f.copy()
    j = np.argmin(d2, axis=1)  # the first of equal minima: the lowest j
    rows = np.arange(n)
    d = d2[rows, j]
    if m == 1:
        return d, j.astype(np.int64), np.full(n, INT32_MAX, dtype=np.int64)
    rest = d2.copy()
    rest[rows, j] = np.iinfo(np.int64).max
    return d, j.astype(np.int64), rest.min(axis=1)


def pair_top2(a, b):
    """The two directions' top-2 of one pair (both images non-empty): (d_a, j_a, s_a, d_b, j_b, s_b)."""
    d2 = dist2(a, b)
    return top2(d2) + top2(d2.T)


def accept(t, ratio=0.8, max_dist2=0, cross_check=True, min_matches=0):
    """(idx_a, idx_b, dist2) int64 arrays of one pair from its top-2, ascending idx_a."""
    e = np.zeros(0, dtype=np.int64)
    if t is None:
        return e, e.copy(), e.copy()
    da, ja, sa, db, jb, sb = t
    r2 = float(ratio) * float(ratio)
    i = np.arange(len(da))
    ok = np.ones(len(da), dtype=bool)
    if cross_check:
        ok &= jb[ja] == i
    if ratio > 0:
        ok &= da.astype(np.float64) < r2 * sa.astype(np.float64)
        if cross_check:
            ok &= da.astype(np.float64) < r2 * sb[ja].astype(np.float64)
    if max_dist2 != 0:
        ok &= da <= max_dist2
    if ok.sum() < min_matches:
        return e, e.copy(), e.copy()
    return i[ok], ja[ok], da[ok]


def match_pair(a, b, **opt):
    a = np.asarray(a)
    b = np.asarray(b)
    return accept(pair_top2(a, b) if len(a) and len(b) else None, **opt)


def match_pairs(desc_a, ptr_a, desc_b, ptr_b, img_a, img_b, cache=None, **opt):
    """CSR of a batch: dict(match_ptr, idx_a, idx_b, dist2) in the layout api.match_descriptors returns.  cache: a dict that keeps
    the pairs' top-2 between calls on the same sets (the options do not enter it)."""
    ptr = [0]
    ia, ib, dd = [], [], []
    for x, y in zip(img_a, img_b):
        key = (int(x), int(y))
        if cache is not None and key in cache:
            t = cache[key]
        else:
            a, b = desc_a[ptr_a[x]:ptr_a[x + 1]], desc_b[ptr_b[y]:ptr_b[y + 1]]
            t = pair_top2(a, b) if len(a) and len(b) else None
            if cache is not None:
                cache[key] = t
        i, j, d = accept(t, **opt)
        ia.append(i); ib.append(j); dd.append(d)
        ptr.append(ptr[-1] + len(i))
    cat = lambda v: np.concatenate(v).astype(np.int32) if v else np.zeros(0, dtype=np.int32)
    return dict(match_ptr=np.asarray(ptr, dtype=np.int64), idx_a=cat(ia), idx_b=cat(ib), dist2=cat(dd))


def structured(n_a, n_b, D):
    """The asymmetric integer data of the layout checks."""
    i = np.arange(n_a)[:, None]
    j = np.arange(n_b)[:, None]
    k = np.arange(D)[None, :]
    return ((7 * i + 3 * k) % 251).astype(np.uint8), ((13 * j + 5 * k + 1) % 241).astype(np.uint8)


def random_desc(rng, n, D):
    """uint8 [n, D] that contains the values 0 and 255 (when it has two elements at least)."""
    x = rng.integers(0, 256, (n, D), dtype=np.uint8)
    if x.size >= 2:
        x.flat[0] = 0
        x.flat[x.size - 1] = 255
    return x


def mixed_sets(seed, D, sizes=SIZES + (0,), near=0.5, noise=6):
    """Two sets of images of the given sizes whose descriptors partly correspond (so that ratio and mutual tests have something to
    accept and something to refuse): image m of B holds noisy copies of some of A's image m's rows, shuffled, and random rows.
    Returns (desc_a, ptr_a, desc_b, ptr_b)."""
    rng = np.random.default_rng(seed)
    A, B = [], []
    for n in sizes:
        a = random_desc(rng, n, D)
        nb = sizes[(sizes.index(n) + 3) % len(sizes)]
        b = random_desc(rng, nb, D)
        k = int(min(n, nb) * near)
        if k:
            src = rng.permutation(n)[:k]
            dst = rng.permutation(nb)[:k]
            b[dst] = np.clip(a[src].astype(np.int64) + rng.integers(-noise, noise + 1, (k, D)), 0, 255).astype(np.uint8)
        A.append(a); B.append(b)
    pa = np.concatenate([[0], np.cumsum([len(x) for x in A])]).astype(np.int64)
    pb = np.concatenate([[0], np.cumsum([len(x) for x in B])]).astype(np.int64)
    return np.concatenate(A), pa, np.concatenate(B), pb


# ------------------------------------------------------------------------------------------------ data sets of the chain tests
def chain_rig(pkg, root):
    """The 20-view x 100 rig with descriptors on disk: (scene, table, feat_ptr, desc, key points, paths).  pairs_matches.txt is the
    generator's own match file."""
    sc = pkg.synth.add_annotations(pkg.synth.make_scene(0, 20, 100))
    tb = pkg.synth.make_match_table(sc, min_pair_matches=8)
    ptr, desc, kp = pkg.synth.make_descriptors(sc, D=128, noise=12, n_distractors=50, seed=7)
    paths = pkg.dataset_io.write_rig(root, sc, tb, annotations=sc.obs3d)
    pkg.dataset_io.write_features(paths["features"], paths["names"], ptr, kp, desc=desc)
    return sc, tb, ptr, desc, kp, paths


def chain_reloc(pkg, root, n_query=24, n_match=96, D=128, noise=12, n_distractors=40):
    """24 relocalization queries with descriptors on disk: match k of query q is feature k of reference image q and of test image q
    (noisy copies of one random descriptor); every image gets unmatched distractors behind them.  pairs_matches.txt is the
    generator's own.  Returns (batch, (ptr, desc) of the references, (ptr, desc) of the tests, paths)."""
    rb = pkg.synth.make_reloc_batch(n_query, n_match, seed_id=6, factor_type=0)
    paths = pkg.dataset_io.write_reloc_set(root, rb)
    rng = np.random.default_rng(17)
    out = []
    base = rng.integers(0, 256, (len(rb.uv_ref), D))
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
        out.append((ptr, desc))
    return rb, out[0], out[1], paths


def read_matches_file(path):
    """{(name_a, name_b): [(i, j), ...]} in file order, as ReadColmapMatches commits them."""
    blocks, cur, name = {}, [], None
    for line in open(path).read().split("\n"):
        if not line:
            if cur:
                blocks[name] = cur
            cur, name = [], None
            continue
        x, y = line.split()
        if x.endswith((".png", ".jpg", ".jpeg")):
            name = (x, y)
        else:
            cur.append((int(x), int(y)))
    return blocks
