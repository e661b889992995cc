"""GPU tests of the guided matcher (ptz_desc_match_pairs_guided, ptz_desc_match_pairs_guided_device) against the numpy restatement
of its contract (desc_guided_util.py).  The warp and the admissibility test are restated bit for bit, everything behind them is
integer arithmetic: every comparison is array-equal, on match_ptr, idx_a, idx_b, dist2, uv_a and uv_b."""
import os
import subprocess
import sys

import numpy as np
import pytest

import desc_guided_util as gu
import desc_match_util as du

pytestmark = pytest.mark.gpu

IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.float64)
SHIFT = np.array([1, 0, 3, 0, 1, -4, 0, 0, 1], dtype=np.float64)
_c, _s = 1.1 * np.cos(0.05), 1.1 * np.sin(0.05)
ROT_ZOOM = np.array([_c, -_s, 2.25, _s, _c, -3.5, 1e-4, -2e-4, 1], dtype=np.float64)
BEHIND = np.array([1, 0, 0, 0, 1, 0, -1.0 / 32, 0, 1], dtype=np.float64)  # Z = 1 - x / 32: part of the window is behind it
NAN_H = np.array([1, 0, 0, 0, np.nan, 0, 0, 0, 1], dtype=np.float64)
HS = (IDENTITY, SHIFT, ROT_ZOOM, BEHIND, NAN_H)

# ratio 0 / 0.8 / 1, cross_check 0 / 1, max_dist2 (-1: a value that cuts the set), min_matches
OPTIONS = [dict(ratio=0.8, cross_check=1), dict(ratio=0.0, cross_check=1), dict(ratio=1.0, cross_check=1), dict(ratio=0.8, cross_check=0),
           dict(ratio=0.0, cross_check=0), dict(ratio=1.0, cross_check=0), dict(ratio=0.0, cross_check=1, max_dist2=-1),
           dict(ratio=0.0, cross_check=1, min_matches=9), dict(ratio=0.0, cross_check=0, min_matches=20)]


def key_points(seed, n, window=40):
    """integer pixels of a small window: under IDENTITY and SHIFT candidates coincide with the warped point, sit exactly on the
    radius (offsets (0, 4), (4, 0)) and repeat, and a few pixels admit a handful of candidates"""
    return np.random.default_rng(seed).integers(0, window, (n, 2)).astype(np.float32)


def batch(n_img_a, n_img_b):
    """all images of A against all of B: (img_a, img_b, H [n, 9] cycling through HS, found cycling 1, 1, 0, 1, 2)"""
    ia, ib = (x.astype(np.int32) for x in np.divmod(np.arange(n_img_a * n_img_b), n_img_b))
    H = np.stack([HS[(3 * p + p // 7) % len(HS)] for p in range(len(ia))])
    found = np.array([(1, 1, 0, 1, 2)[p % 5] for p in range(len(ia))], dtype=np.int32)
    return ia, ib, H, found


def run_options(pkg, sa, sb, da, pa, ka, db, pb, kb, ia, ib, H, found, radius, options, what):
    cache = {}
    loose = gu.match_pairs_guided(da, pa, ka, db, pb, kb, ia, ib, H, found, radius, cache=cache, ratio=0.0)
    cut = max(int(np.median(loose["dist2"])), 1) if len(loose["dist2"]) else 1
    for o in options:
        o = dict(o)
        if o.get("max_dist2") == -1:
            o["max_dist2"] = cut
        got = pkg.api.match_descriptors_guided(sa, sb, ia, ib, H, found, radius, **o)
        want = gu.match_pairs_guided(da, pa, ka, db, pb, kb, ia, ib, H, found, radius, cache=cache, **o)
        gu.assert_equal(got, want, (what, radius, o))
        if o.get("max_dist2"):
            assert 0 < len(want["idx_a"]) < len(loose["idx_a"])
        if o.get("min_matches"):
            n = np.diff(want["match_ptr"])
            assert (n == 0).any() and (n > 0).any(), "min_matches must empty some pairs and not others"
    return loose


# ------------------------------------------------------------------------------------------------------------ mixed batches
@pytest.mark.parametrize("D", (1, 64, 128, 130, 512))
def test_mixed_batch_two_sets(pkg, D):
    """images of every size of the list, of 0 features and of the workgroup's queries - 1 (257 is + 1), all against all; every H of
    the list, found = 1 / 0 / 2 and NULL, every option; radius 4 for all options, 0.5 and the open radius for two of them"""
    sizes = gu.SIZES + (0, gu.WG_QUERIES - 1)
    da, pa, db, pb = du.mixed_sets(D, D, sizes=sizes)
    ka, kb = key_points(1, len(da)), key_points(2, len(db))
    ia, ib, H, found = batch(len(sizes), len(sizes))
    with pkg.api.DescSet(pa, da, ka) as sa, pkg.api.DescSet(pb, db, kb) as sb:
        loose = run_options(pkg, sa, sb, da, pa, ka, db, pb, kb, ia, ib, H, found, 4.0, OPTIONS, D)
        n = np.diff(loose["match_ptr"])
        assert (n[found != 1] == 0).all() and (n[(found == 1) & np.isnan(H).any(1)] == 0).all() and len(loose["idx_a"]) > 100
        behind = (found == 1) & (H == BEHIND).all(1)
        assert 0 < n[behind].sum()
        run_options(pkg, sa, sb, da, pa, ka, db, pb, kb, ia, ib, H, None, 4.0, OPTIONS[:2], D)   # found = NULL: all 1
        run_options(pkg, sa, sb, da, pa, ka, db, pb, kb, ia, ib, H, found, 0.5, OPTIONS[:2], D)
        run_options(pkg, sa, sb, da, pa, ka, db, pb, kb, ia, ib, H, found, 1e9, OPTIONS[:1] + OPTIONS[4:5], D)


def test_lds_tile_plus_one(pkg):
    """an image of one position more than the workgroup stages at a time (and one of a tile exactly), D = 32: the second LDS tile
    holds one candidate, in both directions"""
    sizes = (gu.LDS_TILE + 1, gu.LDS_TILE, 17)
    da, pa, db, pb = du.mixed_sets(32, 32, sizes=sizes)
    ka, kb = key_points(3, len(da), 120), key_points(4, len(db), 120)
    ia, ib, H, _ = batch(3, 3)
    H[:] = SHIFT
    H[4] = ROT_ZOOM
    # the last feature of the long images is somebody's only candidate: alone in a far corner, with a partner under H
    ka[pa[1] - 1] = (500, 500)
    kb[pb[1] - 1] = (503, 496)
    with pkg.api.DescSet(pa, da, ka) as sa, pkg.api.DescSet(pb, db, kb) as sb:
        loose = run_options(pkg, sa, sb, da, pa, ka, db, pb, kb, ia, ib, H, None, 4.0, OPTIONS[:5], "lds tile")
        last = int(loose["match_ptr"][1]) - 1  # pair 0: feature 1024 of A against feature 1024 of B, each the other's only candidate
        assert loose["idx_a"][last] == gu.LDS_TILE and loose["idx_b"][last] == gu.LDS_TILE


def test_one_set_empty_and_one_feature_images(pkg):
    """set_a == set_b, self pairs included: under the identity at radius 0.5 and ratio 0 a feature's candidates are the features on
    its own pixel, itself among them"""
    sizes = (0, 1, 2, 17, 65)
    da, pa, _, _ = du.mixed_sets(5, 64, sizes=sizes)
    ka = key_points(6, len(da))
    ia, ib, H, found = batch(len(sizes), len(sizes))
    with pkg.api.DescSet(pa, da, ka) as s:
        run_options(pkg, s, s, da, pa, ka, da, pa, ka, ia, ib, H, found, 4.0, OPTIONS[:5], "one set")
        Hi = np.tile(IDENTITY, (len(ia), 1))
        got = pkg.api.match_descriptors_guided(s, s, ia, ib, Hi, None, 0.5, ratio=0.0)
        gu.assert_equal(got, gu.match_pairs_guided(da, pa, ka, da, pa, ka, ia, ib, Hi, None, 0.5, ratio=0.0), "identity")
        for p in np.flatnonzero(ia == ib):
            sl = slice(int(got["match_ptr"][p]), int(got["match_ptr"][p + 1]))
            assert (got["dist2"][sl] == 0).all() and sl.stop - sl.start > 0 or sizes[ia[p]] == 0


def test_ties_and_the_inclusive_bound(pkg):
    """duplicate descriptors at two admissible positions: the lowest index wins and the second equals the best; the 3-4-5 triangle:
    radius 5 admits the candidate, the radius just below does not"""
    rng = np.random.default_rng(8)
    a = du.random_desc(rng, 3, 128)
    b = du.random_desc(rng, 6, 128)
    b[4] = a[0]; b[2] = a[0]                       # two exact copies of a_0 ...
    ka = np.array([[10, 20], [100, 100], [200, 50]], dtype=np.float32)
    kb = np.array([[300, 300], [400, 10], [11, 21], [9, 19], [12, 20], [13, 24]], dtype=np.float32)  # ... both within 4 px; b_5 at (3, 4)
    b[1] = a[0]                                    # a third copy, not admissible
    ia = ib = np.zeros(1, dtype=np.int32)
    below = float(np.nextafter(np.float32(5.0), np.float32(0.0)))
    with pkg.api.DescSet([0, 3], a, ka) as sa, pkg.api.DescSet([0, 6], b, kb) as sb:
        for radius, n_adm in ((4.0, 3), (below, 3), (5.0, 4)):
            assert int(gu.admissible(IDENTITY, ka, kb, radius)[0].sum()) == n_adm
            for o in (dict(ratio=0.0, cross_check=0), dict(ratio=0.0, cross_check=1), dict(ratio=0.8, cross_check=0)):
                got = pkg.api.match_descriptors_guided(sa, sb, ia, ib, IDENTITY[None], None, radius, **o)
                gu.assert_equal(got, gu.match_pairs_guided(a, [0, 3], ka, b, [0, 6], kb, ia, ib, IDENTITY[None], None, radius, **o), (radius, o))
                if o["ratio"] == 0.0 and o["cross_check"] == 0:
                    assert got["idx_a"].tolist() == [0] and got["idx_b"].tolist() == [2] and got["dist2"].tolist() == [0]
                if o["ratio"] == 0.8:
                    assert len(got["idx_a"]) == 0  # the second is the other copy: d2 = 0 fails any ratio
        # the bound alone: b_5 is a_0's only candidate once the copies are gone
        kb2 = kb.copy(); kb2[[2, 3, 4]] += 1000
        with pkg.api.DescSet([0, 6], b, kb2) as sb2:
            hit = pkg.api.match_descriptors_guided(sa, sb2, ia, ib, IDENTITY[None], None, 5.0, ratio=0.8)
            miss = pkg.api.match_descriptors_guided(sa, sb2, ia, ib, IDENTITY[None], None, below, ratio=0.8)
            assert hit["idx_a"].tolist() == [0] and hit["idx_b"].tolist() == [5] and len(miss["idx_a"]) == 0
            assert np.array_equal(hit["uv_a"], ka[:1]) and np.array_equal(hit["uv_b"], kb2[5:6])


# ------------------------------------------------------------------------------------------------- independence of context
def test_a_pairs_bits_do_not_depend_on_how_it_is_run(pkg):
    sizes = (65, 17, 130, 64, 1)
    da, pa, db, pb = du.mixed_sets(21, 128, sizes=sizes)
    ka, kb = key_points(9, len(da)), key_points(10, len(db))
    ia, ib, H, found = batch(len(sizes), len(sizes))
    o = dict(ratio=1.0, cross_check=1)
    want = gu.match_pairs_guided(da, pa, ka, db, pb, kb, ia, ib, H, found, 4.0, **o)
    blocks = lambda c: [tuple(c[k][int(c["match_ptr"][p]):int(c["match_ptr"][p + 1])].tolist() for k in gu.KEYS[1:]) for p in range(len(c["match_ptr"]) - 1)]
    wb = blocks(want)
    assert sum(len(x[0]) > 0 for x in wb) >= 5
    with pkg.api.DescSet(pa, da, ka) as sa, pkg.api.DescSet(pb, db, kb) as sb:
        whole = pkg.api.match_descriptors_guided(sa, sb, ia, ib, H, found, 4.0, **o)
        gu.assert_equal(whole, want, "whole")
        assert whole["n_chunks"] == 1
        # reversed order
        r = slice(None, None, -1)
        rev = pkg.api.match_descriptors_guided(sa, sb, ia[r], ib[r], H[r], found[r], 4.0, **o)
        assert blocks(rev) == wb[::-1]
        # chunked: a workspace that holds about a third of the batch
        total = sum(12 * (sizes[x] + sizes[(y + 3) % len(sizes)]) + sizes[x] for x, y in zip(ia, ib))
        ch = pkg.api.match_descriptors_guided(sa, sb, ia, ib, H, found, 4.0, workspace_bytes=total // 3, **o)
        assert ch["n_chunks"] >= 3
        gu.assert_equal(ch, want, "chunked")
        # alone
        for p in (0, 3, 7, 13, 24):
            one = pkg.api.match_descriptors_guided(sa, sb, ia[p:p + 1], ib[p:p + 1], H[p:p + 1], found[p:p + 1], 4.0, **o)
            assert blocks(one) == wb[p:p + 1], p
        # transposed roles under the SAME H: B's features asking A over the same admissible set accept the transposed matches
        cache = {}
        gu.match_pairs_guided(da, pa, ka, db, pb, kb, ia, ib, H, found, 4.0, cache=cache, **o)
        for p in range(len(ia)):
            t = next((v for k, v in cache.items() if k[0] == ia[p] and k[1] == ib[p] and k[2] == H[p].tobytes()), None)
            if t is None or found[p] != 1:
                assert len(wb[p][0]) == 0
                continue
            j, i, d = gu.accept(t[3:] + t[:3], **{**o, "cross_check": True})
            order = np.argsort(i, kind="stable")
            assert (i[order].tolist(), j[order].tolist(), d[order].tolist()) == (list(wb[p][0]), list(wb[p][1]), list(wb[p][2])), p
        # the stale state: one pair per chunk, so the pair with matches, the same pair with found = 0 and with a NaN H use the
        # same slot of the reused workspace one after the other; and again in a second call
        p = int(np.argmax([len(x[0]) for x in wb]))
        i3, j3 = np.repeat(ia[p:p + 1], 3), np.repeat(ib[p:p + 1], 3)
        H3 = np.stack([H[p], H[p], NAN_H])
        f3 = np.array([1, 0, 1], dtype=np.int32)
        st = pkg.api.match_descriptors_guided(sa, sb, i3, j3, H3, f3, 4.0, workspace_bytes=1, ratio=0.0, cross_check=0)
        assert st["n_chunks"] == 3 and np.diff(st["match_ptr"])[0] > 0 and np.diff(st["match_ptr"])[1:].tolist() == [0, 0]
        again = pkg.api.match_descriptors_guided(sa, sb, i3[1:2], j3[1:2], H3[1:2], f3[1:2], 4.0, ratio=0.0, cross_check=0)
        assert len(again["idx_a"]) == 0 and again["match_ptr"].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------- open radius, device H
def test_open_radius_equals_the_dense_matcher(pkg):
    sizes = gu.SIZES + (0, 130)
    da, pa, db, pb = du.mixed_sets(33, 128, sizes=sizes)
    ka, kb = key_points(11, len(da)), key_points(12, len(db))
    ia, ib, _, _ = batch(len(sizes), len(sizes))
    H = np.tile(ROT_ZOOM, (len(ia), 1))
    with pkg.api.DescSet(pa, da, ka) as sa, pkg.api.DescSet(pb, db, kb) as sb:
        for o in (dict(ratio=0.8, cross_check=1), dict(ratio=0.0, cross_check=0), dict(ratio=1.0, cross_check=1, min_matches=9)):
            got = pkg.api.match_descriptors_guided(sa, sb, ia, ib, H, None, 1e9, **o)
            dense = pkg.api.match_descriptors(sa, sb, ia, ib, **o)
            gu.assert_equal(got, dense, o)
            assert len(got["idx_a"]) > 0


def test_argument_errors_on_the_device(pkg):
    import ctypes as C
    L = pkg.api.lib()
    a = du.random_desc(np.random.default_rng(0), 4, 8)
    k = key_points(0, 4)
    ia = np.zeros(1, dtype=np.int32)
    with pkg.api.DescSet([0, 4], a, k) as s, pkg.api.DescSet([0, 4], a) as bare:
        for radius in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(pkg.api.PtzError):
                pkg.api.match_descriptors_guided(s, s, ia, ia, IDENTITY[None], None, radius)
        with pytest.raises(pkg.api.PtzError):
            pkg.api.match_descriptors_guided(s, bare, ia, ia, IDENTITY[None])          # a set without key points
        h = C.c_void_p()
        o = pkg.api.desc_options()
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        assert L.ptz_desc_match_pairs_guided(s.handle, s.handle, 1, p(ia), p(ia), None, None, C.c_double(4.0), C.byref(o), C.byref(h)) == -1  # NULL H
        assert not h.value
        bad = np.array([4], dtype=np.int32)
        with pytest.raises(pkg.api.PtzError):
            pkg.api.match_descriptors_guided(s, s, bad, ia, IDENTITY[None])            # the list of ptz_desc_match_pairs
        with pytest.raises(pkg.api.PtzError):
            pkg.api.match_descriptors_guided(s, s, ia, ia, IDENTITY[None], ratio=-1.0)
        # n_pair = 0 and a non-finite H are no errors
        e = np.zeros(0, dtype=np.int32)
        assert pkg.api.match_descriptors_guided(s, s, e, e, np.zeros((0, 9)))["match_ptr"].tolist() == [0]
        assert pkg.api.match_descriptors_guided(s, s, ia, ia, np.full((1, 9), np.inf))["match_ptr"].tolist() == [0, 0]


def test_device_h_from_the_gate_equals_the_host_pointer_call():
    """H and found as MatchGate.run_device leaves them on the first pass's device_ptrs go into the _device entry point untouched.
    Own process with torch initialised first (as test_gpu_desc_match.py::test_device_pointers_feed_the_gate)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "run_desc_guided_gate.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.count("desc guided gate ok") == 1, r.stdout[-2000:] + r.stderr[-2000:]
