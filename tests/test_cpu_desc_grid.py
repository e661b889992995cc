"""CPU tests of the grid-binned guided matcher's contract (ptz-calib_amd/csrc/ptz_desc_grid.h) instantiated on the host by
tests/cpu_harness/desc_grid_harness.cc: the harness against the numpy restatement of the guided contract (desc_guided_util.py, which
knows nothing of grids), the conservativeness of the cell ranges as a property, the order-free top-2 update, and the parts of the
C-ABI that need no device."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import desc_guided_util as gu
import desc_match_util as du
from test_gpu_desc_guided import HS, IDENTITY, OPTIONS, ROT_ZOOM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_h = None
RADII = (0.5, 4.0, 40.0, 1e9)


def harness():
    global _h
    if _h is None:
        _h = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "libdesc_grid_harness.so"))
        _h.h_desc_match_pair_grid.restype = C.c_int64
        _h.h_desc_grid_reach.restype = C.c_double
        _h.h_desc_grid_reach.argtypes = [C.c_double]
        _h.h_desc_grid_cells.restype = None
        _h.h_desc_top2_take_keyed.restype = None
    return _h


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def grid_pair(a, b, kp_a, kp_b, H, radius, S, ratio=0.8, max_dist2=0, cross_check=True, min_matches=0):
    a = np.ascontiguousarray(a, dtype=np.uint8); b = np.ascontiguousarray(b, dtype=np.uint8)
    kp_a = np.ascontiguousarray(kp_a, dtype=np.float32); kp_b = np.ascontiguousarray(kp_b, dtype=np.float32)
    H = np.ascontiguousarray(H, dtype=np.float64)
    na, nb, D = len(a), len(b), a.shape[1]
    ta = np.zeros((max(na, 1), 3), dtype=np.int32); tb = np.zeros((max(nb, 1), 3), dtype=np.int32)
    ia, ib, dd = (np.zeros(max(na, 1), dtype=np.int32) for _ in range(3))
    n = harness().h_desc_match_pair_grid(_p(a), na, _p(b), nb, D, _p(kp_a), _p(kp_b), _p(H), C.c_double(radius), int(S), C.c_double(ratio),
                                         int(max_dist2), int(cross_check), int(min_matches), _p(ta), _p(tb), _p(ia), _p(ib), _p(dd))
    return ta[:na], tb[:nb], ia[:n], ib[:n], dd[:n]


def cells(searched, queries, radius):
    """(cell [n, 2] of every searched position, -1: not indexed; range [nq, 4] = cx0, cx1, cy0, cy1 of every query)"""
    s = np.ascontiguousarray(searched, dtype=np.float32).reshape(-1, 2)
    q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 2)
    cell = np.zeros((max(len(s), 1), 2), dtype=np.int32)
    rng = np.zeros((max(len(q), 1), 4), dtype=np.int32)
    harness().h_desc_grid_cells(len(s), _p(s), len(q), _p(q), C.c_double(radius), _p(cell), _p(rng))
    return cell[:len(s)], rng[:len(q)]


def take_keyed(d2, j):
    d2 = np.ascontiguousarray(d2, dtype=np.int32); j = np.ascontiguousarray(j, dtype=np.int32)
    out = np.zeros(3, dtype=np.int32)
    harness().h_desc_top2_take_keyed(len(d2), _p(d2), _p(j), _p(out))
    return tuple(out.tolist())


def test_constants():
    h = harness()
    assert h.h_desc_grid_g() in (16, 32, 64) and h.h_desc_grid_slab() in (2048, 4096)
    for r in (0.5, 4.0, 40.0, 1e9):
        assert h.h_desc_grid_reach(r) == r * (1.0 + 2.0 ** -10)
    assert h.h_desc_grid_reach(1e-300) > 0  # the floor under a radius whose square underflows


# ------------------------------------------------------------------------------------------- the harness against the restatement
def _points(rng, na, nb, H):
    """A's key points on integer pixels of a 40-px window; B's: the warped point of one of A's plus an integer offset of a few pixels
    (under the identity and the shift distances hit the bound exactly and repeat), one in ten far away."""
    kp_a = rng.integers(0, 40, (na, 2)).astype(np.float32)
    if nb == 0 or na == 0:
        return kp_a, rng.integers(0, 40, (nb, 2)).astype(np.float32)
    wx, wy, ok = gu.warp(H, kp_a)
    src = rng.integers(0, na, nb)
    base = np.where(ok[src, None], np.stack([wx, wy], 1)[src], kp_a[src])
    kp_b = (base + rng.integers(-4, 5, (nb, 2))).astype(np.float32)
    kp_b[rng.random(nb) < 0.1] += 500
    return kp_a, kp_b


@pytest.mark.parametrize("D", (1, 64, 130))
def test_grid_harness_equals_numpy(D):
    """both directions' top-2 for every image size, H, radius and slab size (the slab never enters the result), and the accepted
    matches for every option set"""
    rng = np.random.default_rng(200 + D)
    sizes = gu.SIZES + (0, 255)
    S_full = harness().h_desc_grid_slab()
    n_hit = n_multi = 0
    for p, (na, nb) in enumerate(itertools.product(sizes, sizes)):
        a = rng.integers(0, 4 if D == 1 else 256, (na, D), dtype=np.uint8)
        b = rng.integers(0, 4 if D == 1 else 256, (nb, D), dtype=np.uint8)
        k = min(na, nb) // 2
        if k and D > 1:
            b[rng.permutation(nb)[:k]] = np.clip(a[rng.permutation(na)[:k]].astype(np.int64) + rng.integers(-5, 6, (k, D)), 0, 255)
        H = HS[p % len(HS)]
        kp_a, kp_b = _points(rng, na, nb, H)
        d2 = du.dist2(a, b) if na and nb else None
        for radius in RADII:
            if d2 is None:
                fa, fb = np.full(na, gu.INT32_MAX, dtype=np.int64), np.full(nb, gu.INT32_MAX, dtype=np.int64)
                want = (fa, fa, fa, fb, fb, fb)
            else:
                adm = gu.admissible(H, kp_a, kp_b, radius)
                want = gu.top2_masked(d2, adm) + gu.top2_masked(d2.T.copy(), adm.T)
                n_hit += int(adm.sum())
                n_multi += int((adm.sum(1) > 1).sum())
            for S in (8, 64, S_full):
                ta, tb = grid_pair(a, b, kp_a, kp_b, H, radius, S, ratio=0.0)[:2]
                assert np.array_equal(ta, np.stack(want[:3], 1)) and np.array_equal(tb, np.stack(want[3:], 1)), (D, na, nb, radius, S)
            found = want[0][want[0] != gu.INT32_MAX]
            for n_o, o in enumerate(OPTIONS):
                o = dict(o)
                if o.get("max_dist2") == -1:
                    o["max_dist2"] = int(np.median(found)) + 1 if len(found) else 1
                ia, ib, dd = grid_pair(a, b, kp_a, kp_b, H, radius, (8, 64, S_full)[(p + n_o) % 3], **o)[2:]
                wi, wj, wd = gu.accept(want if d2 is not None else None, **o)
                assert np.array_equal(ia, wi) and np.array_equal(ib, wj) and np.array_equal(dd, wd), (D, na, nb, radius, o)
    assert n_hit > 1000 and n_multi > 100


# --------------------------------------------------------------------------------------------------- conservativeness, a property
def _assert_conservative(searched, queries, radius, what):
    """every pair the restatement admits (queries are warped points: identity H) lies inside the query's cell range"""
    s = np.asarray(searched, dtype=np.float32).reshape(-1, 2)
    q = np.asarray(queries, dtype=np.float32).reshape(-1, 2)
    adm = gu.admissible(IDENTITY, q, s, radius)
    cell, rng = cells(s, q, radius)
    G = harness().h_desc_grid_g()
    finite = np.isfinite(s).all(1)
    assert ((cell >= 0).all(1) == finite).all() and (cell < G).all(), what   # the finite positions are indexed, and only they
    assert not adm[:, ~finite].any() or not np.isfinite(gu.r2f_of(radius))
    qi, sj = np.nonzero(adm)
    inside = (rng[qi, 0] <= cell[sj, 0]) & (cell[sj, 0] <= rng[qi, 1]) & (rng[qi, 2] <= cell[sj, 1]) & (cell[sj, 1] <= rng[qi, 3])
    assert inside.all(), (what, radius, q[qi[~inside]][:3], s[sj[~inside]][:3])
    return int(adm.sum())


def test_ranges_are_conservative_random():
    rng = np.random.default_rng(31)
    n = 0
    for radius in RADII + (2.5, 7.0):
        for scale, off in ((40, 0), (1920, 0), (1920, -900), (64, 1e6), (4096, 1e7)):
            s = (rng.uniform(0, scale, (400, 2)) + off).astype(np.float32)
            # queries: near searched positions at about the radius (both sides of it), and uniform ones
            ang = rng.uniform(0, 2 * np.pi, 300)
            near = s[rng.integers(0, len(s), 300)].astype(np.float64) + (radius * rng.uniform(0.9, 1.1, 300))[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
            q = np.concatenate([near, rng.uniform(-0.2 * scale, 1.2 * scale, (100, 2)) + off]).astype(np.float32)
            n += _assert_conservative(s, q, radius, (scale, off))
    assert n > 2000


def test_ranges_are_conservative_adversarial():
    h = harness()
    G = h.h_desc_grid_g()
    n = 0
    # exactly on the radius on integer pixels: the 3-4-5 triangle and (0, r), (r, 0), around queries at many places
    for r, offs in ((5.0, [(3, 4), (4, 3), (-3, 4), (3, -4), (-4, -3), (0, 5), (5, 0), (0, -5), (-5, 0)]), (4.0, [(0, 4), (4, 0), (0, -4), (-4, 0)])):
        q = np.stack(np.meshgrid(np.arange(0, 200, 7), np.arange(0, 120, 11)), -1).reshape(-1, 2).astype(np.float32)
        s = np.concatenate([q + np.float32(o) for o in offs])
        assert gu.admissible(IDENTITY, q[:1], q[:1] + np.float32(offs[0]), r)[0, 0]
        n += _assert_conservative(s, q, r, "on the radius")
        for base in (1e6, 1e7, -3000.0):  # float spacing a sixteenth of a pixel, a whole pixel; negative coordinates
            n += _assert_conservative(s + np.float32(base), q + np.float32(base), r, ("on the radius", base))
    # positions exactly on cell boundaries: the frame's own cell size from a bounding box of G cells of 8 px, radius 4 < 8
    edge = np.arange(G + 1, dtype=np.float32) * 8
    s = np.stack(np.meshgrid(edge, edge), -1).reshape(-1, 2)
    cell, _ = cells(s, s[:1], 4.0)
    assert np.array_equal(cell[:, 0], np.minimum(s[:, 0] // 8, G - 1)) and np.array_equal(cell[:, 1], np.minimum(s[:, 1] // 8, G - 1))
    q = np.concatenate([s + np.float32((4, 0)), s + np.float32((0, -4)), s + np.float32((-2.5, 3)), s])
    n += _assert_conservative(s, q, 4.0, "cell boundaries")
    # where the cell size is the reach: boundaries at multiples of r' -- candidates one float on either side of them
    reach = h.h_desc_grid_reach(4.0)
    b = np.float32(reach * np.arange(1, 9))
    xs = np.concatenate([b, np.nextafter(b, np.float32(0)), np.nextafter(b, np.float32(1e9)), [np.float32(0)]]).astype(np.float32)
    s = np.stack(np.meshgrid(xs, xs[:6]), -1).reshape(-1, 2)
    q = np.concatenate([s + np.float32((4, 0)), s + np.float32((-4, 0)), s + np.float32((0, 4)), s + np.float32((2.5, -3))])
    n += _assert_conservative(s, q, 4.0, "reach boundaries")
    # a warped query far outside the searched side's bounding box, next to one that is inside
    s = np.random.default_rng(3).integers(0, 640, (300, 2)).astype(np.float32)
    q = np.array([[5000, -7000], [-1e6, 1e6], [1e30, 0], [320, 240], [-3, 100], [643, 100], [np.inf, 5], [np.nan, 5]], dtype=np.float32)
    n += _assert_conservative(s, q, 4.0, "far queries")
    _, rng = cells(s, q, 4.0)
    assert rng[6].tolist() == [1, 0, 1, 0] and rng[7].tolist() == [1, 0, 1, 0]  # a query that is not finite does not search
    # a searched side holding NaN, +inf and 1e30 key points: never admissible, the non-finite ones not indexed, the others unaffected
    bad = np.array([[np.nan, 10], [10, np.nan], [np.inf, 10], [10, -np.inf], [np.nan, np.nan]], dtype=np.float32)
    s2 = np.concatenate([s[:150], bad, s[150:]])
    cell2, _ = cells(s2, q, 4.0)
    cell0, _ = cells(s, q, 4.0)
    keep = np.r_[0:150, 155:305]
    assert (cell2[150:155] == -1).all() and np.array_equal(cell2[keep], cell0)
    n += _assert_conservative(s2, np.concatenate([q, s + np.float32((0, 4))]), 4.0, "non-finite searched positions")
    s3 = np.concatenate([s2, np.array([[1e30, 5], [7, -1e30]], dtype=np.float32)])  # finite: indexed, in a frame that is all but one cell
    n += _assert_conservative(s3, np.concatenate([q, s + np.float32((0, 4))]), 4.0, "1e30")
    assert not gu.admissible(IDENTITY, s + np.float32((0, 4)), s3[-2:], 4.0).any()
    # all searched points on one pixel: zero extent
    s = np.full((50, 2), 77, dtype=np.float32)
    q = np.array([[77, 77], [77, 81], [73, 77], [80, 81], [81, 81], [1000, 1000]], dtype=np.float32)
    assert _assert_conservative(s, q, 4.0, "zero extent") == 3 * 50
    assert _assert_conservative(s, q, 5.0, "zero extent") == 4 * 50
    assert n > 3000


def test_non_finite_positions_through_the_harness():
    """the whole pair: NaN, inf and 1e30 key points on either side leave the other features' top-2 what the restatement says"""
    rng = np.random.default_rng(12)
    a, b = du.random_desc(rng, 90, 32), du.random_desc(rng, 70, 32)
    kp_a = rng.integers(0, 60, (90, 2)).astype(np.float32)
    kp_b = rng.integers(0, 60, (70, 2)).astype(np.float32)
    kp_a[[3, 40]] = [[np.nan, 1], [1e30, 2]]
    kp_a[41] = [np.inf, 3]
    kp_b[[0, 9, 33, 69]] = [[np.nan, np.nan], [np.inf, 4], [1e30, 1e30], [-1e30, 7]]
    for H in (IDENTITY, ROT_ZOOM):
        for radius in RADII:
            want = gu.pair_top2(a, b, kp_a, kp_b, H, radius)
            for S in (8, 64, 2048):
                ta, tb = grid_pair(a, b, kp_a, kp_b, H, radius, S, ratio=0.0)[:2]
                assert np.array_equal(ta, np.stack(want[:3], 1)) and np.array_equal(tb, np.stack(want[3:], 1)), (radius, S)
            assert (want[0][[3, 41]] == gu.INT32_MAX).all() and (want[3][[0, 9]] == gu.INT32_MAX).all()


# ------------------------------------------------------------------------------------------------------- the order-free update
def _top2_ascending(d2, j):
    """the contract: best = smallest key (d2, j), second = smallest d2 over the others"""
    order = sorted(zip(d2, j))
    if not order:
        return (gu.INT32_MAX,) * 3
    return (order[0][0], order[0][1], order[1][0] if len(order) > 1 else gu.INT32_MAX)


def test_take_keyed_is_order_free():
    assert take_keyed([], []) == (gu.INT32_MAX,) * 3
    lists = [[5], [5, 5], [7, 5, 5], [5, 5, 5, 5], [9, 3, 3, 9, 1], [4, 4, 2, 2, 4, 2], [0, 0, 33000000, 1, 1, 0]]
    for d2 in lists:
        j = list(range(10, 10 + len(d2)))
        want = _top2_ascending(d2, j)
        assert take_keyed(d2, j) == want                                     # the ascending order is the scan kernel's
        for perm in itertools.permutations(range(len(d2))):
            assert take_keyed([d2[k] for k in perm], [j[k] for k in perm]) == want, (d2, perm)
    rng = np.random.default_rng(4)
    d2 = rng.integers(0, 12, 200).tolist()
    j = rng.permutation(1000)[:200].tolist()
    want = _top2_ascending(d2, j)
    for _ in range(20):
        perm = rng.permutation(200)
        assert take_keyed([d2[k] for k in perm], [j[k] for k in perm]) == want
    # a tie of two equal descriptors: the LOWEST j wins and second == best
    assert take_keyed([6, 6], [9, 2]) == (6, 2, 6) and take_keyed([6, 6], [2, 9]) == (6, 2, 6)


# ------------------------------------------------------------------------------------------- C-ABI parts that need no device
def test_abi(pkg):
    L = pkg.api.lib()
    EINVAL = -1
    h = C.c_void_p()
    ia = np.zeros(1, dtype=np.int32)
    H = IDENTITY.copy()
    for f in (L.ptz_desc_match_pairs_guided_grid, L.ptz_desc_match_pairs_guided_grid_device):
        assert f(None, None, 1, _p(ia), _p(ia), _p(H), None, C.c_double(4.0), None, C.byref(h)) == EINVAL
        assert f(None, None, 0, None, None, None, None, C.c_double(4.0), None, C.byref(h)) == EINVAL
        assert f(None, None, 0, None, None, None, None, C.c_double(4.0), None, None) == EINVAL
    assert not h.value
    assert "ptz_desc_match_pairs_guided_grid" in pkg.api.EXPORTS and "ptz_desc_match_pairs_guided_grid_device" in pkg.api.EXPORTS
    o = pkg.api.RelocOptions()
    o.guided_grid = 7
    L.ptz_reloc_options_default(C.byref(o))
    assert o.guided_grid == 0
    # the parent commit's layout: the field took the place of reserved_
    assert C.sizeof(pkg.api.RelocOptions) == 208 and pkg.api.RelocOptions.lm.offset == 112 and pkg.api.RelocOptions.guided_grid.offset == 108
    # guided_grid = 2 is refused with the other option errors, before the relocalizer is looked at (the pointers are never
    # dereferenced); that 0 and 1 pass and -1 does not is test_gpu_relocalizer_grid.py's
    fake = C.c_void_p(1)
    r = pkg.api.RelocResult()
    o.guided_grid = 2
    assert L.ptz_relocalizer_run(fake, fake, 0, None, C.byref(o), C.byref(r)) == EINVAL
