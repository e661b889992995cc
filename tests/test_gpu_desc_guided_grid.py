"""GPU tests of the grid-binned guided matcher (ptz_desc_match_pairs_guided_grid, ptz_desc_match_pairs_guided_grid_device;
api.match_descriptors_guided(..., grid=True)) against the numpy restatement of the guided contract (desc_guided_util.py), which
shares nothing with either kernel: every comparison is array-equal on match_ptr, idx_a, idx_b, dist2, uv_a and uv_b.  The frame and
the cell function used to PLACE key points come from the contract header through the CPU harness (test_cpu_desc_grid.cells)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import desc_guided_util as gu
import desc_match_util as du
from test_cpu_desc_grid import cells, harness
from test_gpu_desc_guided import BEHIND, HS, IDENTITY, NAN_H, OPTIONS, ROT_ZOOM, SHIFT, batch, key_points

pytestmark = pytest.mark.gpu

S = 2048  # kDescGridSlab: positions of the searched side indexed at a time


def test_the_slab_is_the_headers():
    assert harness().h_desc_grid_slab() == S


def run_options(pkg, sa, sb, da, pa, ka, db, pb, kb, ia, ib, H, found, radius, options, what):
    cache = {}
    loose = gu.match_pairs_guided(da, pa, ka, db, pb, kb, ia, ib, H, found, radius, cache=cache, ratio=0.0)
    cut = max(int(np.median(loose["dist2"])), 1) if len(loose["dist2"]) else 1
    for o in options:
        o = dict(o)
        if o.get("max_dist2") == -1:
            o["max_dist2"] = cut
        got = pkg.api.match_descriptors_guided(sa, sb, ia, ib, H, found, radius, grid=True, **o)
        want = gu.match_pairs_guided(da, pa, ka, db, pb, kb, ia, ib, H, found, radius, cache=cache, **o)
        gu.assert_equal(got, want, (what, radius, o))
        if o.get("max_dist2"):
            assert 0 < len(want["idx_a"]) < len(loose["idx_a"])
        if o.get("min_matches"):
            n = np.diff(want["match_ptr"])
            assert (n == 0).any() and (n > 0).any(), "min_matches must empty some pairs and not others"
    return loose


# ------------------------------------------------------------------------------------------------------------ the mixed batch
@pytest.mark.parametrize("D", (1, 64, 128, 130, 512))
def test_mixed_batch_two_sets(pkg, D):
    """the batch of test_gpu_desc_guided.py::test_mixed_batch_two_sets -- key points in a 40-px window: the cell size is the reach"""
    sizes = gu.SIZES + (0, gu.WG_QUERIES - 1)
    da, pa, db, pb = du.mixed_sets(D, D, sizes=sizes)
    ka, kb = key_points(1, len(da)), key_points(2, len(db))
    ia, ib, H, found = batch(len(sizes), len(sizes))
    with pkg.api.DescSet(pa, da, ka) as sa, pkg.api.DescSet(pb, db, kb) as sb:
        loose = run_options(pkg, sa, sb, da, pa, ka, db, pb, kb, ia, ib, H, found, 4.0, OPTIONS, D)
        n = np.diff(loose["match_ptr"])
        assert (n[found != 1] == 0).all() and (n[(found == 1) & np.isnan(H).any(1)] == 0).all() and len(loose["idx_a"]) > 100
        assert 0 < n[(found == 1) & (H == BEHIND).all(1)].sum()
        run_options(pkg, sa, sb, da, pa, ka, db, pb, kb, ia, ib, H, None, 4.0, OPTIONS[:2], D)   # found = NULL: all 1
        run_options(pkg, sa, sb, da, pa, ka, db, pb, kb, ia, ib, H, found, 0.5, OPTIONS[:2], D)
        run_options(pkg, sa, sb, da, pa, ka, db, pb, kb, ia, ib, H, found, 1e9, OPTIONS[:1] + OPTIONS[4:5], D)


# ---------------------------------------------------------------------------------------------------------- the spread regime
def test_spread_key_points(pkg):
    """key points over 1920 x 1080: the cell size comes from the extent.  Pairs (k, k) of two sets with the same image sizes; B's key
    points are A's warped ones on integer pixels plus an offset of {-5 .. 5}^2, permuted (a random pixel where the warp is not ok)."""
    sizes = gu.SIZES + (255, 600, 1000)
    rng = np.random.default_rng(21)
    D = 64
    pa = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    da = du.random_desc(rng, int(pa[-1]), D)
    ka = np.stack([rng.integers(0, 1920, pa[-1]), rng.integers(0, 1080, pa[-1])], 1).astype(np.float32)
    db, kb = np.zeros_like(da), np.zeros_like(ka)
    ia = ib = np.arange(len(sizes), dtype=np.int32)
    H = np.stack([HS[k % len(HS)] for k in range(len(sizes))])
    n_partner = n_adm = 0
    for k, n in enumerate(sizes):
        sl = slice(int(pa[k]), int(pa[k + 1]))
        wx, wy, ok = gu.warp(H[k], ka[sl])
        with np.errstate(all="ignore"):
            b = np.float32(np.rint(np.stack([wx, wy], 1)) + rng.integers(-5, 6, (n, 2)))
        b[~ok] = np.stack([rng.integers(0, 1920, n), rng.integers(0, 1080, n)], 1).astype(np.float32)[~ok]
        perm = rng.permutation(n)
        kb[sl] = b[perm]
        db[sl] = np.clip(da[sl].astype(np.int64) + rng.integers(-6, 7, (n, D)), 0, 255).astype(np.uint8)[perm]
        adm = gu.admissible(H[k], ka[sl], kb[sl], 4.0)
        n_partner += int(ok.sum())
        n_adm += int(adm[perm, np.arange(n)][ok[perm]].sum())  # feature perm[t] of A has its partner at t of B
    print(f"partner pairs {n_partner}, admissible {n_adm} ({n_adm / n_partner:.3f}; 49 of the 121 offsets lie within 4 px)")
    assert 0.25 * n_partner <= n_adm <= 0.75 * n_partner
    with pkg.api.DescSet(pa, da, ka) as sa, pkg.api.DescSet(pa, db, kb) as sb:
        loose = run_options(pkg, sa, sb, da, pa, ka, db, pa, kb, ia, ib, H, None, 4.0, OPTIONS[:5], "spread")
        assert len(loose["idx_a"]) > 0.2 * n_partner
        run_options(pkg, sa, sb, da, pa, ka, db, pa, kb, ia, ib, H, None, 40.0, OPTIONS[:2], "spread")


# -------------------------------------------------------------------------------------------------------------- the slab edge
def test_slab_plus_one(pkg):
    """a searched side of one position more than a slab (and one of a slab exactly), D = 32: the second slab holds one candidate, in
    both directions, alone in a far corner as somebody's only candidate"""
    sizes = (S + 1, S, 17)
    da, pa, db, pb = du.mixed_sets(32, 32, sizes=sizes)
    ka, kb = key_points(3, len(da), 120), key_points(4, len(db), 120)
    ia, ib, H, _ = batch(3, 3)
    H[:] = SHIFT
    H[4] = ROT_ZOOM
    ka[pa[1] - 1] = (500, 500)
    kb[pb[1] - 1] = (503, 496)
    with pkg.api.DescSet(pa, da, ka) as sa, pkg.api.DescSet(pb, db, kb) as sb:
        loose = run_options(pkg, sa, sb, da, pa, ka, db, pb, kb, ia, ib, H, None, 4.0, OPTIONS[:5], "slab")
        last = int(loose["match_ptr"][1]) - 1  # pair 0: feature S of A against feature S of B, each the other's only candidate
        assert loose["idx_a"][last] == S and loose["idx_b"][last] == S


# ---------------------------------------------------------------------------------------------------------- a tie across cells
@pytest.mark.parametrize("copies", (2, 3))
def test_a_tie_across_cells(pkg, copies):
    """copies of one descriptor 3 px left and 3 px right of the predicted point (and, with three, 3 px above it), a cell boundary
    between them by the header's own frame, the HIGHER j in the cell that is walked first: the lowest j wins, and with ratio = 0.8
    the match is rejected because second == best"""
    G = harness().h_desc_grid_g()
    rng = np.random.default_rng(40 + copies)
    a = du.random_desc(rng, 2, 128)
    b = du.random_desc(rng, 8, 128)
    ka = np.array([[64, 24], [200, 200]], dtype=np.float32)  # under the identity the predicted point is the key point
    # the corners fix the frame: G cells of 8 px per axis (reach 4.004 < 8), boundaries at the multiples of 8
    kb = np.array([[0, 0], [8 * G, 8 * G], [67, 24], [150, 90], [64, 21], [10, 200], [90, 30], [61, 24]], dtype=np.float32)
    dup = [7, 2] if copies == 2 else [7, 4, 2]   # (61, 24): cell (7, 3), walked before (67, 24): cell (8, 3); (64, 21): row 2, before both
    low = min(dup)
    for j in dup:
        b[j] = a[0]
    cell, rng_q = cells(kb, ka[:1], 4.0)
    assert cell[7].tolist() == [7, 3] and cell[2].tolist() == [8, 3] and cell[4].tolist() == [8, 2]
    assert rng_q[0].tolist() == [7, 8, 2, 3]
    ia = ib = np.zeros(1, dtype=np.int32)
    with pkg.api.DescSet([0, 2], a, ka) as sa, pkg.api.DescSet([0, 8], b, kb) as sb:
        for o in (dict(ratio=0.0, cross_check=0), dict(ratio=0.0, cross_check=1), dict(ratio=0.8, cross_check=0), dict(ratio=0.8, cross_check=1)):
            got = pkg.api.match_descriptors_guided(sa, sb, ia, ib, IDENTITY[None], None, 4.0, grid=True, **o)
            gu.assert_equal(got, gu.match_pairs_guided(a, [0, 2], ka, b, [0, 8], kb, ia, ib, IDENTITY[None], None, 4.0, **o), o)
            if o["ratio"] == 0.0:
                assert got["idx_a"].tolist() == [0] and got["idx_b"].tolist() == [low] and got["dist2"].tolist() == [0]
            else:
                assert len(got["idx_a"]) == 0
        # and the transposed roles: the duplicates are the QUERIES of direction 1, and A's side holds the tie when the sets swap
        got = pkg.api.match_descriptors_guided(sb, sa, ia, ib, IDENTITY[None], None, 4.0, grid=True, ratio=0.0, cross_check=0)
        gu.assert_equal(got, gu.match_pairs_guided(b, [0, 8], kb, a, [0, 2], ka, ia, ib, IDENTITY[None], None, 4.0, ratio=0.0, cross_check=0), "swapped")


# ------------------------------------------------------------------------------------------- non-finite and far-away input
def test_non_finite_and_far_away_input(pkg):
    """one image pair per input of test_cpu_desc_grid.py's adversarial list, all in one batch, at radius 4, 5 and 40"""
    rng = np.random.default_rng(50)
    A, B = [], []   # per image: key points
    q = np.stack(np.meshgrid(np.arange(0, 200, 7), np.arange(0, 120, 11)), -1).reshape(-1, 2).astype(np.float32)
    offs = [(3, 4), (4, 3), (-3, 4), (3, -4), (0, 5), (5, 0), (0, -5), (-5, 0), (0, 4), (4, 0), (0, -4), (-4, 0)]
    on_radius = np.concatenate([q + np.float32(o) for o in offs])
    for base in (0.0, 1e6, 1e7, -3000.0):  # float spacing a sixteenth of a pixel, a whole pixel; negative coordinates
        A.append(q + np.float32(base)); B.append(on_radius + np.float32(base))
    edge = np.arange(33, dtype=np.float32) * 8     # positions exactly on cell boundaries
    s = np.stack(np.meshgrid(edge, edge), -1).reshape(-1, 2)
    A.append(np.concatenate([s + np.float32((4, 0)), s + np.float32((0, -4)), s + np.float32((-2.5, 3))])); B.append(s)
    box = rng.integers(0, 640, (300, 2)).astype(np.float32)
    far = np.array([[5000, -7000], [-1e6, 1e6], [1e30, 0], [320, 240], [-3, 100], [643, 100], [np.inf, 5], [np.nan, 5]], dtype=np.float32)
    A.append(np.concatenate([far, box[:100] + np.float32((0, 4))])); B.append(box)   # queries far outside the searched box
    bad = np.array([[np.nan, 10], [10, np.nan], [np.inf, 10], [10, -np.inf], [np.nan, np.nan], [1e30, 5], [7, -1e30]], dtype=np.float32)
    A.append(np.concatenate([box[:150] + np.float32((3, 0)), bad])); B.append(np.concatenate([box[:150], bad, box[150:]]))
    A.append(np.array([[77, 77], [77, 81], [73, 77], [80, 81], [81, 81], [1000, 1000]], dtype=np.float32)); B.append(np.full((50, 2), 77, dtype=np.float32))
    pa = np.concatenate([[0], np.cumsum([len(x) for x in A])]).astype(np.int64)
    pb = np.concatenate([[0], np.cumsum([len(x) for x in B])]).astype(np.int64)
    ka, kb = np.concatenate(A), np.concatenate(B)
    da, db = rng.integers(0, 4, (len(ka), 8), dtype=np.uint8), rng.integers(0, 4, (len(kb), 8), dtype=np.uint8)   # few values: ties everywhere
    ia = ib = np.arange(len(A), dtype=np.int32)
    H = np.tile(IDENTITY, (len(A), 1))
    with pkg.api.DescSet(pa, da, ka) as sa, pkg.api.DescSet(pb, db, kb) as sb:
        for radius in (4.0, 5.0, 40.0):
            loose = run_options(pkg, sa, sb, da, pa, ka, db, pb, kb, ia, ib, H, None, radius, OPTIONS[:2] + OPTIONS[4:5], "adversarial")
            assert len(loose["idx_a"]) > 100
        # the same images under the transposed roles: the non-finite points are then queries of direction 0
        run_options(pkg, sb, sa, db, pb, kb, da, pa, ka, ib, ia, H, None, 4.0, OPTIONS[4:5], "adversarial, swapped")


# ------------------------------------------------------------------------------------------------- independence of context
def test_a_pairs_bits_do_not_depend_on_how_it_is_run(pkg):
    sizes = (65, 17, 130, 64, 1)
    da, pa, db, pb = du.mixed_sets(21, 128, sizes=sizes)
    ka, kb = key_points(9, len(da)), key_points(10, len(db))
    ia, ib, H, found = batch(len(sizes), len(sizes))
    o = dict(ratio=1.0, cross_check=1)
    cache = {}
    want = gu.match_pairs_guided(da, pa, ka, db, pb, kb, ia, ib, H, found, 4.0, cache=cache, **o)
    blocks = lambda c: [tuple(c[k][int(c["match_ptr"][p]):int(c["match_ptr"][p + 1])].tolist() for k in gu.KEYS[1:]) for p in range(len(c["match_ptr"]) - 1)]
    wb = blocks(want)
    assert sum(len(x[0]) > 0 for x in wb) >= 5
    run = lambda *a, **k: pkg.api.match_descriptors_guided(*a, grid=True, **k)
    with pkg.api.DescSet(pa, da, ka) as sa, pkg.api.DescSet(pb, db, kb) as sb:
        whole = run(sa, sb, ia, ib, H, found, 4.0, **o)
        gu.assert_equal(whole, want, "whole")
        assert whole["n_chunks"] == 1
        gu.assert_equal(run(sa, sb, ia, ib, H, found, 4.0, **o), whole, "twice")
        r = slice(None, None, -1)
        assert blocks(run(sa, sb, ia[r], ib[r], H[r], found[r], 4.0, **o)) == wb[::-1]
        total = sum(12 * (sizes[x] + sizes[(y + 3) % len(sizes)]) + sizes[x] for x, y in zip(ia, ib))
        ch = run(sa, sb, ia, ib, H, found, 4.0, workspace_bytes=total // 3, **o)
        assert ch["n_chunks"] >= 3
        gu.assert_equal(ch, want, "chunked")
        for p in (0, 3, 7, 13, 24):
            assert blocks(run(sa, sb, ia[p:p + 1], ib[p:p + 1], H[p:p + 1], found[p:p + 1], 4.0, **o)) == wb[p:p + 1], p
        # (B, A) as the transpose under the SAME H and roles: B's features asking A over the same admissible set
        for p in range(len(ia)):
            t = next((v for k, v in cache.items() if k[0] == ia[p] and k[1] == ib[p] and k[2] == H[p].tobytes()), None)
            if t is None or found[p] != 1:
                assert len(wb[p][0]) == 0
                continue
            j, i, d = gu.accept(t[3:] + t[:3], **{**o, "cross_check": True})
            order = np.argsort(i, kind="stable")
            assert (i[order].tolist(), j[order].tolist(), d[order].tolist()) == (list(wb[p][0]), list(wb[p][1]), list(wb[p][2])), p
        # a run after a call that left other data in the workspace: one pair per chunk, so the pair with matches, the same pair with
        # found = 0 and with a NaN H use one slot of the reused workspace one after the other; and again in a second call
        p = int(np.argmax([len(x[0]) for x in wb]))
        i3, j3 = np.repeat(ia[p:p + 1], 3), np.repeat(ib[p:p + 1], 3)
        H3 = np.stack([H[p], H[p], NAN_H])
        f3 = np.array([1, 0, 1], dtype=np.int32)
        st = run(sa, sb, i3, j3, H3, f3, 4.0, workspace_bytes=1, ratio=0.0, cross_check=0)
        assert st["n_chunks"] == 3 and np.diff(st["match_ptr"])[0] > 0 and np.diff(st["match_ptr"])[1:].tolist() == [0, 0]
        again = run(sa, sb, i3[1:2], j3[1:2], H3[1:2], f3[1:2], 4.0, ratio=0.0, cross_check=0)
        assert len(again["idx_a"]) == 0 and again["match_ptr"].tolist() == [0, 0]


def test_argument_errors_on_the_device(pkg):
    """the list of the scan entry points"""
    import ctypes as C
    L = pkg.api.lib()
    a = du.random_desc(np.random.default_rng(0), 4, 8)
    k = key_points(0, 4)
    ia = np.zeros(1, dtype=np.int32)
    g = lambda *x, **kw: pkg.api.match_descriptors_guided(*x, grid=True, **kw)
    with pkg.api.DescSet([0, 4], a, k) as s, pkg.api.DescSet([0, 4], a) as bare:
        for radius in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(pkg.api.PtzError):
                g(s, s, ia, ia, IDENTITY[None], None, radius)
        with pytest.raises(pkg.api.PtzError):
            g(s, bare, ia, ia, IDENTITY[None])          # a set without key points
        h = C.c_void_p()
        o = pkg.api.desc_options()
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        for f in (L.ptz_desc_match_pairs_guided_grid, L.ptz_desc_match_pairs_guided_grid_device):
            assert f(s.handle, s.handle, 1, p(ia), p(ia), None, None, C.c_double(4.0), C.byref(o), C.byref(h)) == -1  # NULL H
            assert not h.value
        with pytest.raises(pkg.api.PtzError):
            g(s, s, np.array([4], dtype=np.int32), ia, IDENTITY[None])
        with pytest.raises(pkg.api.PtzError):
            g(s, s, ia, ia, IDENTITY[None], ratio=-1.0)
        e = np.zeros(0, dtype=np.int32)
        assert g(s, s, e, e, np.zeros((0, 9)))["match_ptr"].tolist() == [0]
        assert g(s, s, ia, ia, np.full((1, 9), np.inf))["match_ptr"].tolist() == [0, 0]
        # a radius whose square is not a finite float admits every pair: the dense matcher's arrays, as the scan kernel gives them
        huge = g(s, s, ia, ia, IDENTITY[None], None, 1e30, ratio=0.0)
        gu.assert_equal(huge, pkg.api.match_descriptors_guided(s, s, ia, ia, IDENTITY[None], None, 1e30, ratio=0.0), "1e30")
        assert len(huge["idx_a"]) == 4


# ---------------------------------------------------------------------------------------------------- equal to the scan kernel
def test_equal_to_the_scan_kernel_on_the_rig():
    """the 20-view rig with repeated descriptors, its 190 pairs, radius 4 and 40, both kernels through the host-array form and the
    device-pointer form.  Own process with torch initialised first (as test_gpu_desc_guided.py's device test)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "run_desc_grid_rig.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.count("desc grid rig ok") == 1, r.stdout[-2000:] + r.stderr[-2000:]
