"""GPU tests of the landmark map (ptz-calib_amd/csrc/ptz_landmark.hip): the device build and the device assembly, array-equal to
the host instantiation of the shared header (tests/cpu_harness/landmark_harness.cc) and to the numpy restatement
(landmark_util.py) on the cases of test_cpu_landmark.py; a query's bits alone, reversed and in a split batch; the device-pointer
form with a stale workspace on the matcher's own buffers and on the same cases, with the two rules only that form has (a landmark
index out of range, a malformed range); the argument errors.
The rotation matrices are an input of the contract: harness and restatement get the library's own (api.reloc_ref_rotations).
One CPU case has no device twin: opposite rays that cancel EXACTLY need hand-made rotation matrices, and the map build makes its
own from the cameras (Rodrigues of a half turn leaves sin(pi) = 1.2e-16 behind).  The device's non-finite ray is a reference whose
focal length is not a number instead."""
import os
import subprocess
import sys

import numpy as np
import pytest

import landmark_util as lu

pytestmark = pytest.mark.gpu

N_FEAT = 80
COUNTS = [0, 1, 63, 64, 65, 1025, 7, 0]


def _case(pkg, ft, D, seed=0):
    cams = lu.make_rig(ft & 1, seed=seed)
    fp, desc, kp = lu.make_features(len(cams), D, N_FEAT, seed=seed + 1)
    tp, ti, tf, names = lu.make_tracks(len(cams), N_FEAT, seed=seed + 2)
    return cams, pkg.api.reloc_ref_rotations(cams), (fp, desc, kp), (tp, ti, tf), names


def _device_map(pkg, cams, feats, tracks, ft, min_views=1):
    with pkg.api.DescSet(*feats) as refs, pkg.api.LandmarkMap(refs, cams, *tracks, factor_type=ft, min_views=min_views) as m:
        out = m.arrays()
        assert m.n_landmarks == len(out["lm_track"]) and m.build_ms > 0
    return out


@pytest.mark.parametrize("ft", [0, 1])
@pytest.mark.parametrize("D", [1, 64, 128, 130, 512])
def test_device_build_equals_harness_and_numpy(pkg, ft, D):
    cams, R, feats, tracks, names = _case(pkg, ft, D)
    got = _device_map(pkg, cams, feats, tracks, ft)
    args = dict(feat_ptr=feats[0], desc=feats[1], kp=feats[2], ref_cams=cams, trk_ptr=tracks[0], trk_img=tracks[1], trk_feat=tracks[2],
                factor_type=ft, ref_R=R)
    lu.assert_equal(got, lu.harness_build(**args), lu.MAP_KEYS, ("harness", ft, D))
    lu.assert_equal(got, lu.build(**args), lu.MAP_KEYS, ("numpy", ft, D))
    at = {names[t]: i for i, t in enumerate(got["lm_track"].tolist()) if names[t] != "bulk"}
    assert [int(got["lm_views"][at[f"len{n}"]]) for n in (1, 2, 3, 63, 64, 65)] == [1, 2, 3, 63, 64, 65]
    assert "all_invalid" not in at and "empty" not in at and ("only_outside_with_dist" in at) == (ft == 0)
    assert got["lm_home"][at["home_tie_twin_first"]] == 12 and got["lm_home"][at["home_tie_twin_last"]] == 3


@pytest.mark.parametrize("ft", [0, 1])
def test_min_views_and_a_ray_that_is_not_finite(pkg, ft):
    """min_views = 2 drops the tracks one view short; a reference with fx = NaN makes the rays of its views, and every L they enter,
    not finite: those tracks are no landmarks, on the device as on the host."""
    cams, R, feats, tracks, names = _case(pkg, ft, 64, seed=3)
    cams[1, 0] = np.nan
    got = _device_map(pkg, cams, feats, tracks, ft, min_views=2)
    args = dict(feat_ptr=feats[0], desc=feats[1], kp=feats[2], ref_cams=cams, trk_ptr=tracks[0], trk_img=tracks[1], trk_feat=tracks[2],
                factor_type=ft, min_views=2, ref_R=R)
    lu.assert_equal(got, lu.harness_build(**args), lu.MAP_KEYS, ("harness", ft))
    lu.assert_equal(got, lu.build(**args), lu.MAP_KEYS, ("numpy", ft))
    kept = {names[t] for t in got["lm_track"].tolist()}
    assert not kept & {"single", "one_valid_of_two", "len1"} and "bulk" in kept
    assert (got["lm_views"] >= 2).all() and np.isfinite(got["lm_ray"]).all()
    tp, ti, tf = tracks
    in_1 = (ti == 1) & (tf >= 0) & (tf < N_FEAT)  # a view of reference 1 whose feature exists: its ray is not finite
    uses_1 = {t for t in range(len(names)) if in_1[tp[t]:tp[t + 1]].any()}
    assert len(uses_1) >= 5 and not uses_1 & set(got["lm_track"].tolist())


@pytest.fixture(scope="module")
def maps(pkg):
    out = {}
    for ft in (0, 1):
        cams, R, feats, tracks, names = _case(pkg, ft, 64, seed=5 + ft)
        refs = pkg.api.DescSet(*feats)
        m = pkg.api.LandmarkMap(refs, cams, *tracks, factor_type=ft)
        lm = m.arrays()
        out[ft] = (cams, R, m, lm, lu.make_queries(lm, names, COUNTS, seed=9 + ft), refs)
    yield out
    for v in out.values():
        v[2].close()
        v[5].close()


def _device_asm(pkg, m, csr, R):
    out = pkg.api.landmark_assemble(m, csr["match_ptr"], csr["idx_a"], csr["uv_b"], csr["query_wh"], ref_R=R)
    out.pop("device_ms")
    return out


@pytest.mark.parametrize("ft", [0, 1])
def test_device_assembly_equals_harness_and_numpy(pkg, maps, ft):
    cams, R, m, lm, csr, _ = maps[ft]
    got = _device_asm(pkg, m, csr, R)
    lu.assert_equal(got, lu.harness_assemble(lm, ref_cams=cams, ref_R=R, **csr), lu.ASM_KEYS, ("harness", ft))
    lu.assert_equal(got, lu.assemble(lm, ref_cams=cams, ref_R=R, **csr), lu.ASM_KEYS, ("numpy", ft))
    nq = len(csr["match_ptr"]) - 1
    assert got["anchor_ref"][0] == -1 and got["anchor_ref"][nq - 2] == got["anchor_ref"][nq - 1] == np.unique(lm["lm_home"])[0]
    assert 0 < len(got["src"]) < len(csr["idx_a"])


@pytest.mark.parametrize("ft", [0, 1])
def test_a_querys_bits_alone_reversed_and_split(pkg, maps, ft):
    cams, R, m, lm, csr, _ = maps[ft]
    full = _device_asm(pkg, m, csr, R)
    nq = len(csr["match_ptr"]) - 1
    for qs in [[5], [2], [nq - 3], list(range(nq))[::-1], list(range(0, 4)), list(range(4, nq))]:
        sub, idx = lu.slice_queries(csr, qs)
        part = _device_asm(pkg, m, sub, R)
        for k, q in enumerate(qs):
            a, b = lu.per_query(part, k), lu.per_query(full, q)
            assert np.array_equal(idx[a["src"]], b["src"]), (qs, q)
            for key in ("anchor_ref", "uv_ref", "uv_cur", "cam_ref", "cam_init"):
                assert np.array_equal(a[key], b[key]), (qs, q, key)


def test_argument_errors(pkg, maps):
    api = pkg.api
    cams, R, m, lm, csr, refs = maps[0]
    tp, ti, tf = np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([0], dtype=np.int32)

    def code(fn):
        with pytest.raises(api.PtzError) as e:
            fn()
        return e.value.code

    assert code(lambda: api.LandmarkMap(refs, cams[:5], tp, ti, tf)) == -1              # not the set's image count
    assert code(lambda: api.LandmarkMap(refs, cams, np.array([1, 1]), ti, tf)) == -1    # offsets do not start at 0
    assert code(lambda: api.LandmarkMap(refs, cams, np.array([0, 2, 1]), ti, tf)) == -1  # decreasing
    assert code(lambda: api.LandmarkMap(refs, cams, tp, ti, tf, min_views=0)) == -1
    assert code(lambda: api.LandmarkMap(refs, cams, tp, ti, tf, factor_type=9)) == -4
    with api.DescSet(np.array([0, 2] + [2] * (len(cams) - 1)), np.zeros((2, 64), np.uint8)) as no_kp:
        assert code(lambda: api.LandmarkMap(no_kp, cams, tp, ti, tf)) == -1             # features without key points
    bad = dict(csr, idx_a=np.where(np.arange(len(csr["idx_a"])) == 3, len(lm["lm_home"]), csr["idx_a"]).astype(np.int32))
    assert code(lambda: _device_asm(pkg, m, bad, R)) == -1                              # a landmark index out of range
    assert code(lambda: _device_asm(pkg, m, dict(csr, match_ptr=csr["match_ptr"] + 1), R)) == -1
    assert code(lambda: _device_asm(pkg, m, dict(csr, query_wh=csr["query_wh"] * 0), R)) == -1
    with api.LandmarkMap(refs, cams, np.array([0], dtype=np.int64), ti[:0], tf[:0]) as empty:  # no tracks: an empty map is a map
        assert empty.n_landmarks == 0 and len(empty.arrays()["lm_track"]) == 0


def _helper(mode):
    return subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "run_landmark_assemble_device.py"), mode], capture_output=True,
                          text=True, timeout=600)


def test_device_form_on_the_matchers_pointers():
    """ptz_landmark_assemble_device on ptz_desc_matches_device_ptrs of the (map, query) pairs, on a stream, the workspace and the
    outputs filled with a stale pattern first: the host form's arrays on the downloaded table.  Own process with torch initialised
    first (as test_gpu_reloc_assemble.py::test_device_form_on_the_matchers_pointers)."""
    r = _helper("matcher")
    assert r.returncode == 0 and r.stdout.count("landmark assemble device ok") == 2, r.stdout[-2000:] + r.stderr[-2000:]


def test_device_form_on_the_cases():
    """The device-pointer form, stale workspace and outputs, on the cases the host form is held to above (queries of 0, 1, 63, 64,
    65, 1025 matches, no anchor, the hand-made query of a landmark behind and one far away, the ties), F and FDist, array-equal to
    the harness and the restatement; and the two rules only this form has: a landmark index out of range neither votes nor is
    kept, a malformed range is an empty one.  Own process, as above."""
    r = _helper("cases")
    assert r.returncode == 0 and r.stdout.count("landmark assemble device cases ok") == 2, r.stdout[-2000:] + r.stderr[-2000:]
