"""CPU tests of the landmark shortlist's contract: the shared header (ptz-calib_amd/csrc/ptz_landmark_shortlist.h) instantiated on
the host by tests/cpu_harness/landmark_shortlist_harness.cc against the numpy restatement (landmark_shortlist_util.py) -- home
groups, votes, lists and views array-equal -- and the argument errors of the C-ABI that need no device."""
import ctypes as C

import numpy as np
import pytest

import landmark_shortlist_util as lu

LM_SIZES = (0, 1, 17, 257)
HOMES = (1, 5, 23)
QUERY_SIZES = (0, 1, 64, 300)
PROBES = (1, 16, 128, 300)


def _groups_equal(home, n_ref):
    rc, got = lu.harness_groups(home, n_ref)
    want = lu.home_groups(home, n_ref)
    assert rc == 0
    lu.assert_equal(got, want, (len(home), n_ref), keys=("home_ptr", "home_lm"))
    return want


def test_home_groups_with_empty_homes():
    _, home = lu.make_map(257, 23, 8, seed=1, empty=(0, 7, 8, 22))
    g = _groups_equal(home, 23)
    n = np.diff(g["home_ptr"])
    assert n[[0, 7, 8, 22]].tolist() == [0, 0, 0, 0] and (n > 0).sum() == 19 and g["home_ptr"][-1] == 257
    for r in range(23):  # image r: the landmarks of home r, ascending
        assert np.array_equal(g["home_lm"][g["home_ptr"][r]:g["home_ptr"][r + 1]], np.nonzero(home == r)[0])


def test_home_groups_single_home_and_own_homes():
    g = _groups_equal(np.zeros(17, dtype=np.int32), 1)
    assert g["home_ptr"].tolist() == [0, 17] and g["home_lm"].tolist() == list(range(17))
    g = _groups_equal(np.full(17, 3, dtype=np.int32), 5)  # a single home among five
    assert g["home_ptr"].tolist() == [0, 0, 0, 0, 17, 17]
    own = np.random.default_rng(2).permutation(23).astype(np.int32)  # every landmark its own home
    g = _groups_equal(own, 23)
    assert g["home_ptr"].tolist() == list(range(24)) and np.array_equal(own[g["home_lm"]], np.arange(23))
    g = _groups_equal(np.zeros(0, dtype=np.int32), 5)
    assert g["home_ptr"].tolist() == [0] * 6
    assert lu.harness_groups(np.array([0, 5], dtype=np.int32), 5)[0] == -1 and lu.harness_groups(np.array([-1], dtype=np.int32), 5)[0] == -1


@pytest.mark.parametrize("D", [1, 64, 128, 130])
def test_votes_and_lists_equal_numpy(D):
    """maps of {0, 1, 17, 257} landmarks over {1, 5, 23} homes, queries of {0, 1, 64, 300} features, M in {1, 16, 128, 300}"""
    spread = 0
    for n_lm in LM_SIZES:
        for n_ref in HOMES:
            desc, home = lu.make_map(n_lm, n_ref, D, seed=n_lm + n_ref, empty=(1,) if n_ref > 1 else ())
            refs = lu.home_images(desc, home, n_ref)
            for n in QUERY_SIZES:
                q = lu.make_query(desc, n, seed=n + D)
                for M in PROBES:
                    o = dict(ratio=0.8) if (n + M) % 3 else dict(ratio=0.0, max_dist2=D * 40)
                    want_v = lu.su.votes_of(q, refs, M, **o)
                    assert np.array_equal(lu.shortlist(desc, home, n_ref, q, np.array([0, n]), n_probes=M, max_refs=2, **o)["votes"][0], want_v)
                    for R, mv in ((1, 1), (2, 0), (7, 2)):
                        votes, row, ns = lu.harness_shortlist(desc, home, n_ref, q, M, R, min_votes=mv, seed=n + M + R, parts=1 + (n + R) % 4, **o)
                        wrow, wn = lu.su.select(want_v, R, mv)
                        assert np.array_equal(votes, want_v), (D, n_lm, n_ref, n, M, o)
                        assert np.array_equal(row, wrow) and ns == wn, (D, n_lm, n_ref, n, M, R, mv)
                    spread += int(((want_v > 0) & (want_v < min(n, M))).sum())
                    if n_ref > 1:
                        assert want_v[1] == 0  # an empty home has no vote
    assert D == 1 or spread > 20


def _lists(home, n_ref, n_query, seed):
    """the lists of the issue: empty (R slots of -1 is 'all -1'; no query is 'empty'), full, a duplicate home, one home only"""
    rng = np.random.default_rng(seed)
    used = np.unique(home) if len(home) else np.zeros(1, dtype=np.int32)
    R = max(n_ref, 3)
    out = {"all_minus_one": np.full((n_query, R), -1, dtype=np.int32), "full": np.pad(lu.all_homes(home, n_ref, n_query), ((0, 0), (0, R - n_ref)), constant_values=-1),
           "every_index": np.tile(np.pad(np.arange(n_ref, dtype=np.int32), (0, R - n_ref), constant_values=-1), (n_query, 1))}
    dup = np.full((n_query, R), -1, dtype=np.int32)
    dup[:, 0] = dup[:, 2] = used[rng.integers(0, len(used), n_query)]
    dup[:, 1] = used[rng.integers(0, len(used), n_query)]
    out["duplicate"] = dup
    one = np.full((n_query, 1), -1, dtype=np.int32)
    one[:, 0] = used[rng.integers(0, len(used), n_query)]
    out["one_home"] = one
    out["random"] = np.where(rng.random((n_query, 4)) < 0.3, -1, rng.integers(0, n_ref, (n_query, 4))).astype(np.int32)
    return out


@pytest.mark.parametrize("n_ref", [1, 5, 23, 300])
def test_views_equal_numpy(n_ref):
    for n_lm in LM_SIZES + (1025,):
        _, home = lu.make_map(n_lm, n_ref, 1, seed=n_lm, empty=(2,) if n_ref > 2 else ())
        for name, lists in _lists(home, n_ref, 5, n_lm + n_ref).items():
            want = lu.view(home, lists)
            for form in (0, 1):
                rc, got = lu.harness_view(home, n_ref, lists, device_form=form)
                assert rc == 0
                lu.assert_equal(got, want, (n_ref, n_lm, name, form))
            n = np.diff(want["vis_ptr"])
            if name == "all_minus_one":
                assert (n == 0).all()
            if name in ("full", "every_index"):  # the whole map in order
                assert (n == n_lm).all() and np.array_equal(want["vis_lm"], np.tile(np.arange(n_lm, dtype=np.int32), 5))
            if name == "duplicate":  # a home listed twice counts once
                assert all(n[q] == np.isin(home, np.unique(lists[q][lists[q] >= 0])).sum() for q in range(5))
            if name == "one_home":
                assert all(n[q] == (home == lists[q, 0]).sum() for q in range(5))
    # no query at all
    rc, got = lu.harness_view(home, n_ref, np.zeros((0, 3), dtype=np.int32))
    assert rc == 0 and got["vis_ptr"].tolist() == [0] and len(got["vis_lm"]) == 0


def test_an_entry_out_of_range():
    """PTZ_EINVAL in the host form; ignored in the device form"""
    _, home = lu.make_map(257, 5, 1, seed=3)
    for bad in (5, -2, 2**31 - 1, -2**31):
        lists = np.array([[0, bad, 3], [1, -1, -1]], dtype=np.int32)
        assert lu.harness_view(home, 5, lists)[0] == -1
        rc, got = lu.harness_view(home, 5, lists, device_form=True)
        assert rc == 0
        lu.assert_equal(got, lu.view(home, np.array([[0, -1, 3], [1, -1, -1]])), bad)


# ------------------------------------------------------------------------------------------- C-ABI errors that need no device
def test_abi_argument_errors(pkg):
    L = pkg.api.lib()
    EINVAL = -1
    L.ptz_landmark_map_home_set.restype = C.c_void_p
    L.ptz_landmark_shortlist_workspace_bytes.restype = C.c_int64
    assert L.ptz_landmark_map_home_set(None) is None
    assert L.ptz_landmark_map_home_groups(None, None, None) == EINVAL
    assert L.ptz_landmark_shortlist(None, None, 0, None, None, None, None, None, None, None) == EINVAL
    assert L.ptz_landmark_shortlist_device(None, None, 1, None, None, None, None, None, None, None, C.c_int64(0), None) == EINVAL
    assert L.ptz_landmark_shortlist_workspace_bytes(None, None, 1, None) == 0
    h = C.c_void_p(1)
    assert L.ptz_landmark_view_from_homes(None, 0, 1, None, C.c_int64(1 << 20), C.byref(h)) == EINVAL and not h
    h = C.c_void_p(1)
    assert L.ptz_landmark_view_from_homes_device(None, 0, 1, None, C.c_int64(1 << 20), None, C.byref(h)) == EINVAL and not h
    assert L.ptz_landmark_view_from_homes(None, 0, 1, None, C.c_int64(1 << 20), None) == EINVAL
    assert L.ptz_landmark_view_kind(None) == EINVAL
    assert L.ptz_relocalizer_run_landmarks_shortlisted(None, None, None, 0, None, None, None, None, None, None) == EINVAL
    assert (pkg.api.VIEW_PRIOR, pkg.api.VIEW_HOMES) == (0, 1)
