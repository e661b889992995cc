"""GPU tests of the descriptor matcher (ptz_desc_set, ptz_desc_match_pairs, ptz_debug_desc_dist2) against the numpy restatement
of its contract (desc_match_util.py).  The matcher is integer arithmetic from end to end: every comparison is array-equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

import desc_match_util as du

pytestmark = pytest.mark.gpu

SIZES = du.SIZES


def sets_of(pkg, desc_a, ptr_a, desc_b, ptr_b, kp=False):
    rng = np.random.default_rng(99)
    ka = rng.uniform(0, 1920, (len(desc_a), 2)).astype(np.float32) if kp else None
    kb = rng.uniform(0, 1080, (len(desc_b), 2)).astype(np.float32) if kp else None
    return pkg.api.DescSet(ptr_a, desc_a, ka), pkg.api.DescSet(ptr_b, desc_b, kb), ka, kb


def assert_csr_equal(got, want, what=""):
    for k in ("match_ptr", "idx_a", "idx_b", "dist2"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k][:20], want[k][:20])


# ------------------------------------------------------------------------------------------------------- the distance matrix
@pytest.mark.parametrize("D", du.DIMS)
@pytest.mark.parametrize("kind", ["structured", "random"])
def test_dist2_every_shape(pkg, D, kind):
    """Every (n_a, n_b) of the size list at one D: one image per size in each set.  Asymmetric structured data shows a row <-> column
    swap or a wrong k map; random data with 0 and 255 the bias and the padding."""
    rng = np.random.default_rng(D)
    A, B = [], []
    for n in SIZES:
        if kind == "structured":
            a, _ = du.structured(n, 1, D)
            _, b = du.structured(1, n, D)
        else:
            a, b = du.random_desc(rng, n, D), du.random_desc(rng, n, D)
        A.append(a); B.append(b)
    ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    sa, sb, _, _ = sets_of(pkg, np.concatenate(A), ptr, np.concatenate(B), ptr)
    with sa, sb:
        for x in range(len(SIZES)):
            for y in range(len(SIZES)):
                got = pkg.api.desc_dist2(sa, x, sb, y)
                want = du.dist2(A[x], B[y])
                assert got.dtype == np.int32 and np.array_equal(got, want), (kind, D, SIZES[x], SIZES[y])


def test_dist2_extremes(pkg):
    """all-255 against all-0 at D = 512: the largest d2 there is, 512 * 255^2, through the bias and the int32 range"""
    a = np.full((17, 512), 255, dtype=np.uint8)
    b = np.zeros((65, 512), dtype=np.uint8)
    sa, sb, _, _ = sets_of(pkg, a, [0, 17], b, [0, 65])
    with sa, sb:
        assert np.array_equal(pkg.api.desc_dist2(sa, 0, sb, 0), np.full((17, 65), 512 * 255 * 255, dtype=np.int32))
        assert np.array_equal(pkg.api.desc_dist2(sb, 0, sa, 0), np.full((65, 17), 512 * 255 * 255, dtype=np.int32))
        assert np.array_equal(pkg.api.desc_dist2(sa, 0, sa, 0), np.zeros((17, 17), dtype=np.int32))


# -------------------------------------------------------------------------------------------------------------------- matches
OPTIONS = [dict(ratio=0.8, cross_check=1), dict(ratio=0.0, cross_check=1), dict(ratio=1.0, cross_check=1), dict(ratio=0.8, cross_check=0),
           dict(ratio=0.0, cross_check=0), dict(ratio=1.0, cross_check=0, max_dist2=0), dict(ratio=0.0, cross_check=1, max_dist2=-1),
           dict(ratio=0.8, cross_check=1, min_matches=9), dict(ratio=0.0, cross_check=0, min_matches=20)]


@pytest.fixture(scope="module")
def mixed(pkg):
    """D -> (desc_a, ptr_a, desc_b, ptr_b, pair lists): images of every size of the list, and of 0 features, all against all"""
    out = {}
    for D in du.MATCH_DIMS:
        da, pa, db, pb = du.mixed_sets(D, D)
        n = len(pa) - 1
        ia, ib = np.divmod(np.arange(n * n), n)
        out[D] = (da, pa, db, pb, ia.astype(np.int32), ib.astype(np.int32))
    return out


@pytest.mark.parametrize("D", du.MATCH_DIMS)
def test_matches_two_sets(pkg, mixed, D):
    da, pa, db, pb, ia, ib = mixed[D]
    sa, sb, ka, kb = sets_of(pkg, da, pa, db, pb, kp=True)
    cache = {}
    loose = du.match_pairs(da, pa, db, pb, ia, ib, cache=cache, ratio=0.0)
    cut = int(np.median(loose["dist2"]))  # a max_dist2 that cuts the set
    with sa, sb:
        for o in OPTIONS:
            o = dict(o)
            if o.get("max_dist2") == -1:
                o["max_dist2"] = max(cut, 1)
            got = pkg.api.match_descriptors(sa, sb, ia, ib, **o)
            want = du.match_pairs(da, pa, db, pb, ia, ib, cache=cache, **o)
            assert_csr_equal(got, want, (D, o))
            if o.get("min_matches"):
                n = np.diff(want["match_ptr"])
                assert (n == 0).any() and (n > 0).any(), "min_matches must empty some pairs and not others"
            if o.get("max_dist2"):
                assert 0 < len(want["idx_a"]) < len(loose["idx_a"])
            # gathered pixels: the key points at the indices
            pair_of = np.repeat(np.arange(len(ia)), np.diff(got["match_ptr"]))
            assert np.array_equal(got["uv_a"], ka[pa[ia[pair_of]] + got["idx_a"]])
            assert np.array_equal(got["uv_b"], kb[pb[ib[pair_of]] + got["idx_b"]])


@pytest.mark.parametrize("D", du.MATCH_DIMS)
def test_matches_one_set_and_self_pairs(pkg, mixed, D):
    """set_a == set_b; an image against itself matches every feature with itself at d2 = 0 when ratio = 0 (where rows are distinct:
    not at D = 1, whose rows repeat -- there the restatement alone decides)"""
    da, pa, _, _, _, _ = mixed[D]
    n = len(pa) - 1
    ia, ib = (x.astype(np.int32) for x in np.divmod(np.arange(n * n), n))
    with pkg.api.DescSet(pa, da) as s:
        cache = {}
        for o in (dict(ratio=0.8), dict(ratio=0.0), dict(ratio=0.0, cross_check=0)):
            got = pkg.api.match_descriptors(s, s, ia, ib, **o)
            assert "uv_a" not in got
            assert_csr_equal(got, du.match_pairs(da, pa, da, pa, ia, ib, cache=cache, **o), o)
        got = pkg.api.match_descriptors(s, s, np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32), ratio=0.0)
        assert_csr_equal(got, du.match_pairs(da, pa, da, pa, np.arange(n), np.arange(n), cache=cache, ratio=0.0))
        if D == 1:
            return
        assert np.array_equal(np.diff(got["match_ptr"]), np.diff(pa))
        assert np.array_equal(got["idx_a"], got["idx_b"]) and not got["dist2"].any()
        assert np.array_equal(got["idx_a"], np.concatenate([np.arange(k) for k in np.diff(pa)]))


def test_empty_calls(pkg, mixed):
    da, pa, db, pb, _, _ = mixed[96]
    sa, sb, _, _ = sets_of(pkg, da, pa, db, pb)
    with sa, sb:
        got = pkg.api.match_descriptors(sa, sb, [], [])
        assert got["match_ptr"].tolist() == [0] and len(got["idx_a"]) == 0
        zero = int(np.flatnonzero(np.diff(pa) == 0)[0])
        got = pkg.api.match_descriptors(sa, sb, [zero, 3, zero], [2, int(np.flatnonzero(np.diff(pb) == 0)[0]), zero], ratio=0.0)
        assert got["match_ptr"].tolist() == [0, 0, 0, 0]
    with pkg.api.DescSet([0], np.zeros((0, 128), np.uint8)) as e:
        assert pkg.api.match_descriptors(e, e, [], [])["match_ptr"].tolist() == [0]


def test_more_pairs_than_a_chunk_holds(pkg):
    """2^20 + 3 pairs of one-feature images: the pair list is cut by the pair count as well, and every pair keeps its match"""
    d = np.array([[3, 200, 7, 9]], dtype=np.uint8)
    n = (1 << 20) + 3
    z = np.zeros(n, dtype=np.int32)
    with pkg.api.DescSet([0, 1], d) as s:
        got = pkg.api.match_descriptors(s, s, z, z, ratio=0.0)
    assert got["n_chunks"] == 2 and np.array_equal(got["match_ptr"], np.arange(n + 1))
    assert not got["idx_a"].any() and not got["idx_b"].any() and not got["dist2"].any()


# ----------------------------------------------------------------------------------------------------------------------- ties
def test_ties_in_b_and_in_a(pkg):
    rng = np.random.default_rng(5)
    D = 128
    a = du.random_desc(rng, 40, D)
    b = du.random_desc(rng, 257, D)
    b[3] = a[7]
    b[200] = a[7]          # two identical rows of B in different column tiles and lanes: best 3, second == best
    a[21] = a[20]          # two identical rows of A ...
    b[100] = a[20]         # ... and their common nearest neighbour: the lower i wins the mutual check
    d2 = du.dist2(a, b)
    assert d2[7, 3] == 0 and d2[7, 200] == 0 and d2[20, 100] == 0 and d2[21, 100] == 0
    with pkg.api.DescSet([0, 40], a) as sa, pkg.api.DescSet([0, 257], b) as sb:
        for o in (dict(ratio=0.8), dict(ratio=0.0), dict(ratio=0.0, cross_check=0), dict(ratio=0.8, cross_check=0)):
            got = pkg.api.match_descriptors(sa, sb, [0], [0], **o)
            assert_csr_equal(got, du.match_pairs(a, [0, 40], b, [0, 257], [0], [0], **o), o)
            m = dict(zip(got["idx_a"].tolist(), got["idx_b"].tolist()))
            if o["ratio"] > 0:
                assert 7 not in m  # second == best: the ratio test refuses it
            else:
                assert m[7] == 3
            if not o.get("cross_check", 1):
                assert m[20] == 100 and m[21] == 100
            elif o["ratio"] == 0:
                assert m[20] == 100 and 21 not in m
            else:
                assert 20 not in m and 21 not in m  # B's row 100 has its second at the best: refused on B's side


# --------------------------------------------------------------------------------------------------------------- independence
def test_pairs_are_independent_of_batch_order_and_chunks(pkg, mixed):
    da, pa, db, pb, ia, ib = mixed[128]
    rng = np.random.default_rng(1)
    pick = rng.permutation(len(ia))[:40]
    ia, ib = ia[pick], ib[pick]
    sa, sb, ka, kb = sets_of(pkg, da, pa, db, pb, kp=True)
    with sa, sb:
        full = pkg.api.match_descriptors(sa, sb, ia, ib, min_matches=3)
        assert full["n_chunks"] == 1
        assert_csr_equal(full, du.match_pairs(da, pa, db, pb, ia, ib, min_matches=3))
        per_pair = [{k: full[k][full["match_ptr"][p]:full["match_ptr"][p + 1]] for k in ("idx_a", "idx_b", "dist2", "uv_a", "uv_b")}
                    for p in range(40)]
        # alone
        for p in range(40):
            one = pkg.api.match_descriptors(sa, sb, ia[p:p + 1], ib[p:p + 1], min_matches=3)
            for k, v in per_pair[p].items():
                assert np.array_equal(one[k], v), (p, k)
        # the reversed batch
        rev = pkg.api.match_descriptors(sa, sb, ia[::-1].copy(), ib[::-1].copy(), min_matches=3)
        for p in range(40):
            q = 39 - p
            for k, v in per_pair[p].items():
                assert np.array_equal(rev[k][rev["match_ptr"][q]:rev["match_ptr"][q + 1]], v), (p, k)
        # a workspace bound that forces chunks
        small = pkg.api.match_descriptors(sa, sb, ia, ib, min_matches=3, workspace_bytes=20000)
        assert small["n_chunks"] >= 3
        for k in ("match_ptr", "idx_a", "idx_b", "dist2", "uv_a", "uv_b"):
            assert np.array_equal(small[k], full[k]), k
        # (B, A) is the transposed, re-sorted (A, B)
        tr = pkg.api.match_descriptors(sb, sa, ib, ia, min_matches=3)
        assert np.array_equal(tr["match_ptr"], full["match_ptr"])
        for p in range(40):
            sl = slice(full["match_ptr"][p], full["match_ptr"][p + 1])
            o = np.argsort(full["idx_b"][sl], kind="stable")
            assert np.array_equal(tr["idx_a"][sl], full["idx_b"][sl][o]) and np.array_equal(tr["idx_b"][sl], full["idx_a"][sl][o])
            assert np.array_equal(tr["dist2"][sl], full["dist2"][sl][o])


# ----------------------------------------------------------------------------------------------- device pointers into the gate
def test_device_pointers_feed_the_gate():
    """The resident CSR goes into ptz_match_gate_run_device as it is and gives what the downloaded arrays give through the host.
    Own process with torch initialised first (as test_gpu_match_gate.py::test_device_resident_chain_gate_then_solve)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "run_desc_match_gate.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.count("desc gate ok") == 1, r.stdout[-2000:] + r.stderr[-2000:]
