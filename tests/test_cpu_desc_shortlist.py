"""CPU tests of the reference shortlist's contract: the shared header (ptz-calib_amd/csrc/ptz_desc_shortlist.h) instantiated on the
host by tests/cpu_harness/desc_shortlist_harness.cc against the numpy restatement (desc_shortlist_util.py) -- probes, votes and
lists array-equal -- and the argument errors of the C-ABI that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import desc_match_util as du
import desc_shortlist_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_h = None


def harness():
    global _h
    if _h is None:
        _h = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "libdesc_shortlist_harness.so"))
        _h.h_desc_shortlist.restype = C.c_int32
    return _h


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness_query(refs, q, M, R, min_votes=1, ratio=0.8, max_dist2=0, seed=1, parts=4):
    """(probes, votes, list row, n_short) of one query image against a list of reference images"""
    D = q.shape[1]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int64)
    ref = np.ascontiguousarray(np.concatenate(refs) if len(refs) else np.zeros((0, D)), dtype=np.uint8)
    ref = ref if ref.size else np.zeros((1, D), dtype=np.uint8)
    qq = np.ascontiguousarray(q, dtype=np.uint8) if len(q) else np.zeros((1, D), dtype=np.uint8)
    m = C.c_int32()
    probes = np.zeros(max(min(len(q), M), 1), dtype=np.int32)
    votes = np.zeros(max(len(refs), 1), dtype=np.int32)
    row = np.zeros(R, dtype=np.int32)
    n = harness().h_desc_shortlist(_p(ref), _p(ptr), len(refs), _p(qq), len(q), D, int(M), int(R), int(min_votes), C.c_double(ratio), int(max_dist2),
                                   C.c_uint64(seed), int(parts), C.byref(m), _p(probes), _p(votes), _p(row))
    return probes[:m.value], votes[:len(refs)], row, n


def rig(rng, sizes, D, n_query_feat, noise=6):
    """References of the given sizes and one query image that holds noisy copies of rows of some of them (so that votes are neither
    all 0 nor all m)"""
    refs = [du.random_desc(rng, n, D) for n in sizes]
    q = du.random_desc(rng, n_query_feat, D)
    for r, b in enumerate(refs):
        k = min(len(b), n_query_feat) * (r % 3) // 3
        if k:
            q[rng.permutation(n_query_feat)[:k]] = np.clip(b[rng.permutation(len(b))[:k]].astype(np.int64) + rng.integers(-noise, noise + 1, (k, D)), 0, 255)
    return refs, q


@pytest.mark.parametrize("M", [1, 16, 100, 256])
def test_probes_votes_and_lists_equal_numpy(M):
    """n around M: {0, 1, M - 1, M, M + 1, 3 M + 1}; the probes are strictly increasing features of the image"""
    rng = np.random.default_rng(M)
    for n in sorted({0, 1, max(M - 1, 0), M, M + 1, 3 * M + 1}):
        refs, q = rig(rng, (0, 1, 17, 40, 65, 33), 32, n)
        want_p = su.probes(n, M)
        assert len(want_p) == min(n, M) and (np.diff(want_p) > 0).all() and (len(want_p) == 0 or (want_p[0] == 0 and want_p[-1] < n))
        for o in (dict(ratio=0.8), dict(ratio=0.0), dict(ratio=0.8, max_dist2=32 * 40)):
            want_v = su.votes_of(q, refs, M, **o)
            for R, mv in ((1, 1), (3, 0), (6, 2), (9, 1)):
                got_p, got_v, row, ns = harness_query(refs, q, M, R, min_votes=mv, seed=n + R, parts=1 + (n + R) % 5, **o)
                wrow, wn = su.select(want_v, R, mv)
                assert np.array_equal(got_p, want_p) and np.array_equal(got_v, want_v), (M, n, o)
                assert np.array_equal(row, wrow) and ns == wn, (M, n, o, R, mv)
        if n:
            assert su.votes_of(q, refs, M, ratio=0.8).max() > 0 and su.votes_of(q, refs, M, ratio=0.8)[0] == 0  # an empty reference has no vote


def test_probe_index_is_exact_in_int64():
    """floor(k n / M) where k n does not fit 32 bits: without references the harness reads no row of the query, so the rule can be
    instantiated for the largest image there is"""
    n, M = 2**31 - 1, 2**20
    m = C.c_int32()
    probes = np.zeros(M, dtype=np.int32)
    dummy = np.zeros(4, dtype=np.int32)
    ptr = np.zeros(1, dtype=np.int64)
    q = np.zeros(1, dtype=np.uint8)
    ns = harness().h_desc_shortlist(_p(q), _p(ptr), 0, _p(q), n, 1, M, 2, 1, C.c_double(0.8), 0, C.c_uint64(1), 1, C.byref(m), _p(probes), _p(dummy), _p(dummy))
    want = np.array([k * n // M for k in range(M)], dtype=np.int64)
    assert ns == 0 and m.value == M and np.array_equal(probes, want) and (np.diff(want) > 0).all() and want[-1] < n
    assert dummy[:2].tolist() == [-1, -1]


def test_ties_min_votes_and_order():
    """the same image twice among the references: the lowest index first; min_votes cuts; R > n_ref; ascending whatever the votes"""
    rng = np.random.default_rng(5)
    base = du.random_desc(rng, 50, 64)
    q = np.clip(base.astype(np.int64) + rng.integers(-4, 5, base.shape), 0, 255).astype(np.uint8)
    weak = base.copy(); weak[10:] = du.random_desc(rng, 40, 64)          # 10 rows of the query's scene
    mid = base.copy(); mid[30:] = du.random_desc(rng, 20, 64)            # 30 rows
    refs = [weak, base, du.random_desc(rng, 45, 64), base.copy(), mid]
    v = su.votes_of(q, refs, 256)
    assert v[1] == v[3] == 50 and v[4] >= 30 > v[0] >= 10 > v[2]
    enough = lambda mv: [r for r in (0, 1, 3, 4) if v[r] >= mv]
    for R, mv, want in ((1, 1, [1]), (2, 1, [1, 3]), (3, 1, [1, 3, 4]), (4, 1, [0, 1, 3, 4]), (9, 11, enough(11)), (9, 31, enough(31)), (9, 51, [])):
        _, got_v, row, ns = harness_query(refs, q, 256, R, min_votes=mv)
        wrow, wn = su.select(v, R, mv)
        assert np.array_equal(got_v, v) and np.array_equal(row, wrow) and ns == wn == len(want), (R, mv)
        assert row[:ns].tolist() == sorted(want) and (row[ns:] == -1).all()
    # a reference without votes never ranks, however large R
    _, _, row, ns = harness_query(refs, q, 256, 20, min_votes=0)
    assert ns == int((v >= 1).sum()) and row[:ns].tolist() == [r for r in range(5) if v[r] >= 1]


def test_rank_of_agrees_with_select():
    v = np.array([3, 0, 7, 3, 7, 1])
    assert [su.rank_of(v, r) for r in range(6)] == [2, 6, 0, 3, 1, 4]
    assert su.select(v, 3)[0].tolist() == [0, 2, 4] and su.select(v, 2)[0].tolist() == [2, 4]


# ------------------------------------------------------------------------------------------- C-ABI errors that need no device
def test_abi_argument_errors(pkg):
    L = pkg.api.lib()
    EINVAL = -1
    o = pkg.api.shortlist_options()
    assert (o.max_refs, o.n_probes, o.min_votes, o.reserved_) == (8, 256, 1, 0)
    assert pkg.api.shortlist_options(max_refs=3, n_probes=64, min_votes=2).n_probes == 64
    with pytest.raises(TypeError):
        pkg.api.shortlist_options(probes=3)
    L.ptz_shortlist_options_default(None)
    out = np.zeros(8, dtype=np.int32)
    img = np.zeros(1, dtype=np.int32)
    assert L.ptz_desc_shortlist(None, None, 1, _p(img), None, None, _p(out), _p(out), None, None) == EINVAL
    assert L.ptz_desc_shortlist(None, None, 0, None, None, None, None, None, None, None) == EINVAL
    assert L.ptz_desc_shortlist_device(None, None, 1, None, None, None, None, None, None, None, C.c_int64(0), None) == EINVAL
    L.ptz_desc_shortlist_workspace_bytes.restype = C.c_int64
    assert L.ptz_desc_shortlist_workspace_bytes(None, None, 1, None) == 0
    assert L.ptz_relocalizer_run_shortlisted(None, None, 0, None, None, None, None, None) == EINVAL
    assert L.ptz_relocalizer_pairs(None, None, None, None) == EINVAL
