"""Seeded correspondence sets for the batched homography estimator (ptz-calib_amd/csrc/ptz_homography.h / .hip) and the
host estimator it reproduces (host/homography.cc, through libptzcalib_host.so's ptzh_find_homography)."""
import ctypes as C

import numpy as np

W, H = 1920.0, 1080.0


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def random_homography(rng):
    a, s = rng.uniform(-0.3, 0.3), rng.uniform(0.7, 1.4)
    return np.array([[s * np.cos(a), -s * np.sin(a), rng.uniform(-200, 200)],
                     [s * np.sin(a), s * np.cos(a), rng.uniform(-100, 100)],
                     [rng.uniform(-2e-4, 2e-4), rng.uniform(-2e-4, 2e-4), 1.0]])


def make_pair(rng, n, outliers, noise=0.5):
    """n correspondences b ~ H a with `noise` px of Gaussian noise, a fraction `outliers` of b replaced by uniform pixels."""
    a = rng.uniform([0, 0], [W, H], size=(n, 2))
    Hm = random_homography(rng)
    ah = np.c_[a, np.ones(n)] @ Hm.T
    b = ah[:, :2] / ah[:, 2:] + rng.normal(0, noise, (n, 2))
    k = rng.random(n) < outliers
    b[k] = rng.uniform([0, 0], [W, H], size=(int(k.sum()), 2))
    return a.astype(np.float32), b.astype(np.float32)


def special_pairs(rng):
    """Small inputs, degenerate and duplicated points, a NaN pixel, and the pure-outlier sets whose first accepted model has
    so few inliers that the host's bound overflows int (x86 INT_MIN: the loop stops after that iteration)."""
    out = [make_pair(rng, n, 0.0) for n in (0, 1, 2, 3, 4, 4, 5, 5, 6)]
    out += [make_pair(rng, 4, 0.5), make_pair(rng, 5, 0.4)]
    t = rng.uniform(0, 1, 60)
    line = np.c_[100 + 1500 * t, 200 + 600 * t].astype(np.float32)          # every point on one line: every sample degenerate
    out.append((line, make_pair(rng, 60, 0.0)[1]))
    a, b = make_pair(rng, 80, 0.2)
    t2 = rng.uniform(0, 1, 64)
    a[:64] = np.c_[100 + 1500 * t2, 300 + 400 * t2]
    out.append((a, b))                                                       # most points collinear
    a, b = make_pair(rng, 40, 0.1)
    out.append((np.repeat(a, 2, axis=0), np.repeat(b, 2, axis=0)))          # every correspondence twice
    a, b = make_pair(rng, 5, 0.0)
    out.append((np.repeat(a[:1], 5, axis=0), b))                             # five copies of one source point
    a, b = make_pair(rng, 50, 0.2)
    a[7, 0] = np.nan                                                         # a NaN pixel
    out.append((a, b))
    a, b = make_pair(rng, 30, 0.0)
    b[3, 1] = np.nan
    out.append((a, b))
    for n in (1000, 1500, 3000):                                             # pure outliers: the INT_MIN bound
        out.append(make_pair(rng, n, 1.0))
    out.append(make_pair(rng, 400, 0.8))                                     # runs the full 2000 iterations
    return out


def corpus(seed=0, n_pairs=2000):
    """At least n_pairs sets: the special ones, then sizes 4-3000 (exactly 4 and 5 included) at 0-80 % outliers (at most 50 %
    above 400 matches)."""
    rng = np.random.default_rng(seed)
    pairs = special_pairs(rng)
    while len(pairs) < n_pairs:
        u = rng.random()
        n = int(rng.integers(4, 12)) if u < 0.15 else int(rng.integers(12, 400)) if u < 0.97 else int(rng.integers(400, 3001))
        # outlier rates of 60-80 % run hundreds to 2000 iterations: fewer of them keep the host side of the tests short
        out = float(rng.choice([0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8], p=[.2, .17, .17, .17, .13, .1, .03, .02, .01]))
        pairs.append(make_pair(rng, n, out if n <= 400 else min(out, 0.5)))
    return pack(pairs)


def pack(pairs):
    ptr = np.concatenate([[0], np.cumsum([len(a) for a, _ in pairs])]).astype(np.int64)
    src = np.ascontiguousarray(np.concatenate([a.reshape(-1, 2) for a, _ in pairs]), dtype=np.float32) if pairs else np.zeros((0, 2), np.float32)
    dst = np.ascontiguousarray(np.concatenate([b.reshape(-1, 2) for _, b in pairs]), dtype=np.float32) if pairs else np.zeros((0, 2), np.float32)
    return ptr, src, dst


def run_per_pair(fn, ptr, src, dst, thresh=4.0):
    """fn = ptzh_find_homography (host library) or h_find_homography (harness), one pair at a time.
    Returns (H [n,3,3] zeros where not found, found [n], mask [n_match] zeros where not found)."""
    n = len(ptr) - 1
    H = np.zeros((n, 3, 3))
    found = np.zeros(n, dtype=np.int32)
    mask = np.zeros(int(ptr[-1]), dtype=np.uint8)
    for p in range(n):
        a, b = ptr[p], ptr[p + 1]
        s = np.ascontiguousarray(src[a:b]); d = np.ascontiguousarray(dst[a:b])
        h = np.zeros(9); m = np.zeros(max(b - a, 1), dtype=np.uint8)
        found[p] = fn(int(b - a), _p(s), _p(d), C.c_double(thresh), _p(h), _p(m))
        if found[p]:
            H[p] = h.reshape(3, 3)
            mask[a:b] = m[:b - a]
    return H, found, mask


def table_arrays(tb):
    """A synth.MatchTable as the flat arrays of ptz_homography_ransac_batch: (match_ptr, src_uv, dst_uv)."""
    src = tb.kp_xy[tb.kp_ptr[tb.src[np.repeat(np.arange(tb.n_pairs), np.diff(tb.match_ptr))]] + tb.q]
    dst = tb.kp_xy[tb.kp_ptr[tb.dst[np.repeat(np.arange(tb.n_pairs), np.diff(tb.match_ptr))]] + tb.t]
    return tb.match_ptr.astype(np.int64), np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32)


def inject_outliers(tb, frac, seed=0):
    """Replace a fraction of every pair's matches by matches to a random key point of the destination image (in place)."""
    rng = np.random.default_rng(seed)
    pair_of = np.repeat(np.arange(tb.n_pairs), np.diff(tb.match_ptr))
    k = np.flatnonzero(rng.random(len(tb.t)) < frac)
    nkp = np.diff(tb.kp_ptr)[tb.dst[pair_of[k]]]
    tb.t[k] = (rng.random(len(k)) * nkp).astype(np.int32)
    return tb
