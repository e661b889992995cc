"""GPU tests of the reference shortlist (ptz_desc_shortlist, ptz-calib_amd/csrc/ptz_desc_shortlist.hip): votes, lists and counts are
array-equal to the numpy restatement (desc_shortlist_util.py) over reference images of {0, 1, 15, 16, 17, 63, 64, 65, 129, 257}
features, queries of {0, 1, 31, 32, 33, 127, 128, 129, 300}, probe budgets around the 16-, 32- and 128-probe edges, several k-step
counts, reference sets whose split into groups is ragged, with and without the ratio test and a distance bound; a query's rows do not
depend on the batch; the device-pointer form returns the host form's arrays whatever its workspace held."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import desc_shortlist_util as su

pytestmark = pytest.mark.gpu

REF_SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 129, 257)
QUERY_SIZES = (0, 1, 31, 32, 33, 127, 128, 129, 300)
PROBES = (1, 16, 100, 128, 256, 300)
N_REFS = (1, 2, 5, 23)


def make_sets(seed, D, n_ref=23, noise=6):
    """References of REF_SIZES (cycled, from the largest down so that a set of one image is not empty) and queries of QUERY_SIZES as
    desc_match_util.mixed_sets builds its pairs: random rows, and in every query noisy copies of rows of several references."""
    rng = np.random.default_rng(seed)
    hi = 4 if D == 1 else 256  # (D = 1: few values, so equal distances and ties everywhere)
    sizes = [REF_SIZES[::-1][r % len(REF_SIZES)] for r in range(n_ref)]
    refs = [rng.integers(0, hi, (n, D), dtype=np.uint8) for n in sizes]
    qs = []
    for n in QUERY_SIZES:
        q = rng.integers(0, hi, (n, D), dtype=np.uint8)
        for r in rng.permutation(n_ref)[:6]:
            k = min(len(refs[r]), n) // 3
            if k:
                q[rng.permutation(n)[:k]] = np.clip(refs[r][rng.permutation(len(refs[r]))[:k]].astype(np.int64) + rng.integers(-noise, noise + 1, (k, D)), 0, hi - 1)
        qs.append(q)
    ptr = lambda v: np.concatenate([[0], np.cumsum([len(x) for x in v])]).astype(np.int64)
    return refs, ptr(refs), qs, ptr(qs)


def want_rows(V, R, min_votes):
    rows = [su.select(v, R, min_votes) for v in V]
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], dtype=np.int32)


def assert_equal(got, V, R, min_votes, ctx):
    rows, ns = want_rows(V, R, min_votes)
    assert np.array_equal(got["votes"], V), ctx
    assert np.array_equal(got["shortlist"], rows) and np.array_equal(got["n_short"], ns), ctx


@pytest.mark.parametrize("D", [1, 64, 128, 130, 512])
def test_votes_and_lists_equal_numpy(pkg, D):
    refs, rp, qs, qp = make_sets(D, D)
    qd = np.concatenate(qs)
    api = pkg.api
    spread = 0
    with api.DescSet(qp, qd) as Q:
        for n_ref in N_REFS:
            with api.DescSet(rp[:n_ref + 1], np.concatenate(refs[:n_ref])) as Rs:
                for M in PROBES:
                    for ratio in (0.0, 0.8):
                        V = np.stack([su.votes_of(q, refs[:n_ref], M, ratio=ratio) for q in qs])
                        for R, mv in ((1, 1), (3, 2), (8, 0), (30, 1)):
                            got = api.desc_shortlist(Rs, Q, max_refs=R, n_probes=M, min_votes=mv, ratio=ratio)
                            assert_equal(got, V, R, mv, (D, n_ref, M, ratio, R, mv))
                        if ratio > 0 and M >= 100 and n_ref == 23 and D > 1:
                            m = np.array([min(len(q), M) for q in qs])
                            spread += int(((V > 0) & (V < m[:, None])).sum())
    assert D == 1 or spread > 20  # votes that are neither 0 nor all of the probes


def test_max_dist2_cuts(pkg):
    refs, rp, qs, qp = make_sets(7, 128)
    api = pkg.api
    with api.DescSet(rp, np.concatenate(refs)) as Rs, api.DescSet(qp, np.concatenate(qs)) as Q:
        open_ = np.stack([su.votes_of(q, refs, 256, ratio=0.0) for q in qs])
        bound = 128 * 36  # a near copy's d2 is at most 128 * 6^2; a random row's is far above
        V = np.stack([su.votes_of(q, refs, 256, ratio=0.0, max_dist2=bound) for q in qs])
        assert 0 < V.sum() < open_.sum()
        got = api.desc_shortlist(Rs, Q, max_refs=5, n_probes=256, ratio=0.0, max_dist2=bound)
        assert_equal(got, V, 5, 1, "max_dist2")
        got = api.desc_shortlist(Rs, Q, max_refs=5, n_probes=256, ratio=0.8, max_dist2=bound, cross_check=0, min_matches=50)  # neither enters
        assert_equal(got, np.stack([su.votes_of(q, refs, 256, ratio=0.8, max_dist2=bound) for q in qs]), 5, 1, "ratio and max_dist2")


@pytest.mark.parametrize("n_ref", [2, 5, 23])
def test_a_query_does_not_depend_on_the_batch(pkg, n_ref):
    """alone, reversed, split in two, and repeated 8, 15 and 40 times: with 3 probe tiles per query the references are walked in
    23 / 5 / 3 / 1 groups of a 23-image set (ragged: 23 = 4 x 5 + 3 = 7 x 3 + 2) -- the same rows every time"""
    refs, rp, qs, qp = make_sets(11, 128)
    api = pkg.api
    o = dict(max_refs=4, n_probes=300, min_votes=1)
    with api.DescSet(rp[:n_ref + 1], np.concatenate(refs[:n_ref])) as Rs, api.DescSet(qp, np.concatenate(qs)) as Q:
        V = np.stack([su.votes_of(q, refs[:n_ref], 300) for q in qs])
        full = api.desc_shortlist(Rs, Q, **o)
        assert_equal(full, V, 4, 1, n_ref)
        n = len(qs)
        for img in ([5], list(range(n))[::-1], list(range(n // 2)), list(range(n // 2, n)), list(range(n)) * 8, list(range(n)) * 15, list(range(n)) * 40, []):
            got = api.desc_shortlist(Rs, Q, query_img=np.array(img, dtype=np.int32), **o)
            for key in ("votes", "shortlist", "n_short"):
                assert np.array_equal(got[key], full[key][img]), (n_ref, len(img), key)


def test_device_form_and_stale_workspace():
    """ptz_desc_shortlist_device on a stream, with device outputs, a device image list and a workspace full of stale bytes: the host
    form's arrays.  Own process with torch initialised first (as test_gpu_reloc_assemble.py::test_device_form_on_the_matchers_pointers)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "run_desc_shortlist_device.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.count("desc shortlist device ok") == 3, r.stdout[-2000:] + r.stderr[-2000:]


def test_argument_errors_and_empty_sets(pkg):
    refs, rp, qs, qp = make_sets(17, 64, n_ref=3)
    api = pkg.api
    L = api.lib()
    with api.DescSet(rp, np.concatenate(refs)) as Rs, api.DescSet(qp, np.concatenate(qs)) as Q, \
            api.DescSet(qp, np.concatenate(qs)[:, :32].copy()) as other_D:
        for bad in (dict(max_refs=0), dict(n_probes=0), dict(min_votes=-1), dict(ratio=-0.5), dict(ratio=float("nan")), dict(max_dist2=-1),
                    dict(min_matches=-1), dict(workspace_bytes=0), dict(device_id=1)):
            with pytest.raises(api.PtzError) as e:
                api.desc_shortlist(Rs, Q, **bad)
            assert e.value.code == -1, bad
        for img in ([-1], [len(qs)]):
            with pytest.raises(api.PtzError) as e:
                api.desc_shortlist(Rs, Q, query_img=np.array(img, dtype=np.int32))
            assert e.value.code == -1
        with pytest.raises(api.PtzError):
            api.desc_shortlist(Rs, other_D)
        img = np.zeros(1, dtype=np.int32)
        assert L.ptz_desc_shortlist(Rs.handle, Q.handle, 1, img.ctypes.data_as(C.c_void_p), None, None, None, None, None, None) == -1  # no outputs
        assert L.ptz_desc_shortlist(Rs.handle, Q.handle, 0, None, None, None, None, None, None, None) == 0
        got = api.desc_shortlist(Rs, Q, query_img=np.zeros(0, dtype=np.int32))
        assert got["shortlist"].shape == (0, 8) and got["votes"].shape == (0, 3)
        # NULL options are the defaults
        out, ns = np.zeros((len(qs), 8), dtype=np.int32), np.zeros(len(qs), dtype=np.int32)
        qi = np.arange(len(qs), dtype=np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert L.ptz_desc_shortlist(Rs.handle, Q.handle, len(qs), p(qi), None, None, p(out), p(ns), None, None) == 0
        want = api.desc_shortlist(Rs, Q)
        assert np.array_equal(out, want["shortlist"]) and np.array_equal(ns, want["n_short"])
    # references without any feature, and queries without any
    e = np.zeros((0, 64), dtype=np.uint8)
    with api.DescSet(np.zeros(3, dtype=np.int64), e) as none, api.DescSet(rp, np.concatenate(refs)) as Rs:
        got = api.desc_shortlist(none, Rs)
        assert (got["votes"] == 0).all() and (got["n_short"] == 0).all() and (got["shortlist"] == -1).all()
        got = api.desc_shortlist(Rs, none)
        assert got["votes"].shape == (2, 3) and (got["votes"] == 0).all() and (got["shortlist"] == -1).all()
