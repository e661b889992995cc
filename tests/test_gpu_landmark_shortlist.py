"""GPU tests of the landmark shortlist (ptz-calib_amd/csrc/ptz_landmark_shortlist.hip): the home groups, the votes and lists of the
vote pass over the home set and the views from lists are array-equal to the numpy restatement (landmark_shortlist_util.py) on maps
of {0, 1, 17, 257, 1025} landmarks over {1, 5, 23, 70} homes (257 = 64 x 4 + 1: a wave's four ballots and one lane more; 1025: a
tile of 1024 landmarks and a tile of one lane; 70 homes: three words of the bitmap), queries of {0, 1, 64, 300} features; the
gathered set holds the map's rows; a list of all homes gives the dense matcher's matches; the device-pointer forms equal the host
forms whatever their workspace held.

A MAP WITH CHOSEN HOMES.  A map is only built from tracks, so the tests make one whose landmarks they know: reference r looks
along pan (360 / n_ref) r degrees, every feature sits at the image centre, and landmark l is the single-view track (home[l], next
feature of that image).  Its ray is the optical axis of reference home[l] -- the nearest axis by (1 - cos) of the pan step -- and
its descriptor is the feature's own (the mean of one).  device_map asserts both on the built map."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import landmark_shortlist_util as lu

pytestmark = pytest.mark.gpu

LM_SIZES = (0, 1, 17, 257, 1025)
HOMES = (1, 5, 23, 70)
QUERY_SIZES = (0, 1, 64, 300)
PROBES = (1, 16, 128, 300)


def device_map(pkg, lm_desc, lm_home, n_ref):
    """(refs, map): the LandmarkMap whose landmark l has descriptor lm_desc[l] and home lm_home[l]; close both"""
    cams = np.zeros((n_ref, 15))
    cams[:, 0] = cams[:, 1] = 3000.0
    cams[:, 2], cams[:, 3] = 960.0, 540.0
    cams[:, 5] = [math.radians(360.0 / n_ref * r) for r in range(n_ref)]
    g = lu.home_groups(lm_home, n_ref)
    rank = np.zeros(len(lm_home), dtype=np.int32)
    rank[g["home_lm"]] = np.arange(len(lm_home)) - np.repeat(g["home_ptr"][:-1], np.diff(g["home_ptr"]))
    desc = np.asarray(lm_desc)[g["home_lm"]]
    refs = pkg.api.DescSet(g["home_ptr"], desc, np.tile(np.float32([960.0, 540.0]), (len(desc), 1)))
    m = pkg.api.LandmarkMap(refs, cams, np.arange(len(lm_home) + 1), np.asarray(lm_home, dtype=np.int32), rank)
    a = m.arrays()
    assert m.n_landmarks == len(lm_home) and np.array_equal(a["lm_home"], lm_home) and np.array_equal(a["lm_desc"], lm_desc)
    return refs, m


def query_set(pkg, desc, sizes=QUERY_SIZES, seed=0):
    qs = [lu.make_query(desc, n, seed=seed + n) for n in sizes]
    qp = np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.int64)
    qd = np.concatenate(qs)
    return qs, qp, qd, pkg.api.DescSet(qp, qd, np.zeros((len(qd), 2), dtype=np.float32))


@pytest.mark.parametrize("D", [1, 64, 128, 130])
def test_groups_votes_and_lists_equal_numpy(pkg, D):
    api = pkg.api
    spread = 0
    for n_lm in LM_SIZES[:4]:
        for n_ref in HOMES[:3]:
            desc, home = lu.make_map(n_lm, n_ref, D, seed=n_lm + n_ref, empty=(1,) if n_ref > 1 else ())
            refs, m = device_map(pkg, desc, home, n_ref)
            qs, qp, qd, Q = query_set(pkg, desc, seed=D)
            try:
                lu.assert_equal(m.home_groups(), lu.home_groups(home, n_ref), (D, n_lm, n_ref), keys=("home_ptr", "home_lm"))
                hs = m.home_set()
                assert hs.n_img == n_ref and hs.handle.value == m.home_set().handle.value  # built once
                images = lu.home_images(desc, home, n_ref)
                for M in PROBES:
                    o = dict(ratio=0.8) if M != 16 else dict(ratio=0.0, max_dist2=D * 40)
                    V = np.stack([lu.su.votes_of(q, images, M, **o) for q in qs])
                    for R, mv in ((1, 1), (2, 0), (7, 2)):
                        got = api.landmark_shortlist(m, Q, max_refs=R, n_probes=M, min_votes=mv, **o)
                        rows = [lu.su.select(v, R, mv) for v in V]
                        assert np.array_equal(got["votes"], V), (D, n_lm, n_ref, M)
                        assert np.array_equal(got["shortlist"], np.stack([r[0] for r in rows])), (D, n_lm, n_ref, M, R, mv)
                        assert np.array_equal(got["n_short"], [r[1] for r in rows]), (D, n_lm, n_ref, M, R, mv)
                    spread += int(((V > 0) & (V < np.minimum([len(q) for q in qs], M)[:, None])).sum())
                # the same call on the home set by its own name
                assert np.array_equal(api.desc_shortlist(hs, Q, max_refs=2)["votes"], api.landmark_shortlist(m, Q, max_refs=2)["votes"])
            finally:
                Q.close(); m.close(); refs.close()
    assert D == 1 or spread > 20


def _hand_lists(home, n_ref, n_query, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for R in (1, 2, 7):
        out[f"random{R}"] = np.where(rng.random((n_query, R)) < 0.3, -1, rng.integers(0, n_ref, (n_query, R))).astype(np.int32)
    out["home0"] = np.zeros((n_query, 1), dtype=np.int32)
    out["last_home"] = np.full((n_query, 2), n_ref - 1, dtype=np.int32)  # (and a duplicate)
    out["last_home"][:, 0] = -1
    out["all_minus_one"] = np.full((n_query, 7), -1, dtype=np.int32)
    out["full"] = lu.all_homes(home, n_ref, n_query)
    dup = out["random7"].copy()
    dup[:, 6] = dup[:, 0]
    out["duplicate"] = dup
    return out


@pytest.mark.parametrize("n_ref", HOMES)
def test_views_equal_numpy(pkg, n_ref):
    api = pkg.api
    nq = 9
    for n_lm in LM_SIZES:
        desc, home = lu.make_map(n_lm, n_ref, 64, seed=n_lm, empty=(2,) if n_ref > 2 else ())
        refs, m = device_map(pkg, desc, home, n_ref)
        try:
            for name, lists in _hand_lists(home, n_ref, nq, n_lm + n_ref).items():
                want = lu.view(home, lists)
                with api.landmark_view_from_homes(m, lists) as v:
                    got = v.arrays()
                    assert v.kind == api.VIEW_HOMES and v.n_visible == len(want["vis_lm"]) and v.device_ms > 0
                lu.assert_equal(got, want, (n_ref, n_lm, name))
                assert got["vis_uv"].shape == (len(want["vis_lm"]), 2) and not got["vis_uv"].any()
                if name == "full":
                    assert np.array_equal(got["vis_lm"], np.tile(np.arange(n_lm, dtype=np.int32), nq))
                # a query alone, reversed, and a split batch: its rows do not depend on its neighbours
                for qsel in ([4], list(range(nq))[::-1], list(range(4)), list(range(4, nq)), []):
                    with api.landmark_view_from_homes(m, lists[qsel].reshape(len(qsel), lists.shape[1])) as v:
                        lu.assert_equal(v.arrays(), lu.view(home, lists[qsel].reshape(len(qsel), lists.shape[1])), (n_ref, n_lm, name, qsel))
        finally:
            m.close(); refs.close()


def test_the_gathered_set_holds_the_maps_rows_and_a_full_list_gives_the_dense_matches(pkg):
    """ptz_debug_desc_dist2 of (view q, query q) is that of (map, query q) restricted to vis_lm; with a hand-made list of all homes
    match_descriptors on (view q, query q) lifted through vis_lm is array-equal to match_descriptors on (map, query q)"""
    api = pkg.api
    n_ref, n_lm = 23, 1025
    desc, home = lu.make_map(n_lm, n_ref, 130, seed=9, empty=(0, 22))
    refs, m = device_map(pkg, desc, home, n_ref)
    qs, qp, qd, Q = query_set(pkg, desc, sizes=(300, 64, 0, 1, 257), seed=3)
    nq = len(qs)
    whole = api._ViewDescSet(m.desc_set().handle, 130, 0, np.array([0, n_lm], dtype=np.int64))
    try:
        sl = api.landmark_shortlist(m, Q, max_refs=3, n_probes=128)
        assert sl["n_short"].max() == 3 and sl["n_short"][2] == 0  # a query without features lists nothing
        full = lu.all_homes(home, n_ref, nq)
        for lists in (sl["shortlist"], full):
            want = lu.view(home, lists)
            with api.landmark_view_from_homes(m, lists) as v:
                view, vs = v.arrays(), v.desc_set()
                lu.assert_equal(view, want, "view")
                for q in range(nq):
                    rows = view["vis_lm"][view["vis_ptr"][q]:view["vis_ptr"][q + 1]]
                    assert np.array_equal(api.desc_dist2(vs, q, Q, q), api.desc_dist2(whole, 0, Q, q)[rows]), q
                t = api.match_descriptors(vs, Q, np.arange(nq), np.arange(nq))
            if lists is full:
                dense = api.match_descriptors(m.desc_set(), Q, np.zeros(nq, dtype=np.int32), np.arange(nq))
                assert np.array_equal(t["match_ptr"], dense["match_ptr"]) and np.array_equal(lu.lift(view, t), dense["idx_a"])
                for key in ("idx_b", "dist2", "uv_a", "uv_b"):
                    assert np.array_equal(t[key], dense[key]), key
                assert dense["match_ptr"][-1] > 50
            else:  # the numpy matcher on the restated view
                wt = lu.su.du.match_pairs(desc[want["vis_lm"]], want["vis_ptr"], qd, qp, np.arange(nq), np.arange(nq))
                for key in ("match_ptr", "idx_a", "idx_b", "dist2"):
                    assert np.array_equal(t[key], wt[key]), key
    finally:
        Q.close(); m.close(); refs.close()


def test_whole_map_property_on_the_24_query_scene(pkg):
    """The scene of test_gpu_relocalizer_landmarks.py: with a hand-made list of all homes, the matches of (view q, query q) lifted
    through vis_lm are those of (map, query q), for every one of the 24 queries"""
    api = pkg.api
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt.copy()
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=24, n_feat=600, visible_share=0.5, noise_px=0.5, seed=0)
    rf, qf = pkg.synth_reloc.make_reloc_descriptors(sc, D=128, noise=12, n_distractors=50, seed=0)
    tp, ti, tf, _ = pkg.synth_reloc.scene_tracks(sc, 50)
    with api.DescSet(*rf) as refs, api.DescSet(*qf) as tests, api.LandmarkMap(refs, rig, tp, ti, tf) as m:
        home = m.arrays()["lm_home"]
        lu.assert_equal(m.home_groups(), lu.home_groups(home, 20), "groups", keys=("home_ptr", "home_lm"))
        ia = np.arange(24, dtype=np.int32)
        dense = api.match_descriptors(m.desc_set(), tests, np.zeros(24, dtype=np.int32), ia, min_matches=8)
        with api.landmark_view_from_homes(m, lu.all_homes(home, 20, 24)) as v:
            view = v.arrays()
            t = api.match_descriptors(v.desc_set(), tests, ia, ia, min_matches=8)
        assert np.array_equal(view["vis_lm"], np.tile(np.arange(m.n_landmarks, dtype=np.int32), 24))
        assert np.array_equal(t["match_ptr"], dense["match_ptr"]) and np.array_equal(lu.lift(view, t), dense["idx_a"])
        for key in ("idx_b", "dist2", "uv_b"):
            assert np.array_equal(t[key], dense[key]), key
        assert np.diff(dense["match_ptr"]).min() >= 100


def test_device_forms_and_stale_workspace():
    """ptz_landmark_shortlist_device with device outputs and a workspace poisoned with 0xFF, then ptz_landmark_view_from_homes_device
    on its device lists: the host forms' arrays.  Own process with torch initialised first (as
    test_gpu_desc_shortlist.py::test_device_form_and_stale_workspace)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "run_landmark_shortlist_device.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.count("landmark shortlist device ok") == 3, r.stdout[-2000:] + r.stderr[-2000:]


def test_argument_errors_and_limits(pkg):
    api = pkg.api
    desc, home = lu.make_map(257, 5, 64, seed=1)
    refs, m = device_map(pkg, desc, home, 5)
    try:
        def code(fn):
            with pytest.raises(api.PtzError) as e:
                fn()
            return e.value.code

        for bad in (5, -2):  # an entry that is neither -1 nor a home: PTZ_EINVAL in the host form
            assert code(lambda: api.landmark_view_from_homes(m, np.array([[0, bad]], dtype=np.int32))) == -1
        assert code(lambda: api.landmark_view_from_homes(m, np.array([[0, 1]], dtype=np.int32), max_view_bytes=0)) == -1
        assert code(lambda: api.landmark_view_from_homes(m, np.array([[0, 1, 2, 3, 4]], dtype=np.int32), max_view_bytes=1 << 10)) == -5  # PTZ_ELIMIT
        with pytest.raises(ValueError):
            api.landmark_view_from_homes(m, np.zeros((2, 0), dtype=np.int32))
        with api.landmark_view_from_homes(m, np.zeros((0, 3), dtype=np.int32)) as v:  # no query: an empty view
            assert v.n_visible == 0 and v.arrays()["vis_ptr"].tolist() == [0]
        with api.DescSet(np.array([0, 3]), np.zeros((3, 32), np.uint8)) as other_D:
            assert code(lambda: api.landmark_shortlist(m, other_D)) == -1
        for o in (dict(max_refs=0), dict(n_probes=0), dict(min_votes=-1), dict(ratio=-1.0)):
            with api.DescSet(np.array([0, 3]), np.zeros((3, 64), np.uint8)) as q:
                assert code(lambda: api.landmark_shortlist(m, q, **o)) == -1, o
    finally:
        m.close(); refs.close()
