"""CPU tests of the landmark map's contract: the shared header (ptz-calib_amd/csrc/ptz_landmark.h) instantiated on the host by
tests/cpu_harness/landmark_harness.cc against the numpy restatement (landmark_util.py), array-equal on every output with no ulp
bound; the argument errors of the C-ABI that need no device; and the tracks of the synthetic scene (synth_reloc.scene_tracks)."""
import ctypes as C

import numpy as np
import pytest

import landmark_util as lu
import reloc_assemble_util as ru

N_FEAT = 80
COUNTS = [0, 1, 63, 64, 65, 1025, 7, 0]


def _case(ft, D, min_views=1, seed=0):
    cams = lu.make_rig(ft & 1, seed=seed)
    R = ru.harness_rotations(cams)
    fp, desc, kp = lu.make_features(len(cams), D, N_FEAT, seed=seed + 1)
    tp, ti, tf, names = lu.make_tracks(len(cams), N_FEAT, seed=seed + 2)
    args = dict(feat_ptr=fp, desc=desc, kp=kp, ref_cams=cams, trk_ptr=tp, trk_img=ti, trk_feat=tf, factor_type=ft, min_views=min_views, ref_R=R)
    return cams, R, args, names


def _build_both(args, what):
    got, want = lu.harness_build(**args), lu.build(**args)
    lu.assert_equal(got, want, lu.MAP_KEYS, what)
    return got


@pytest.mark.parametrize("ft", [0, 1])
@pytest.mark.parametrize("D", [1, 64, 128, 130, 512])
def test_build_harness_equals_numpy(ft, D):
    """Tracks of 1, 2, 3, 63, 64 and 65 views, byte sums on a half, means of 0 and 255, invalid views of every kind, the home tie,
    for F and FDist and every D: track list, rays, homes, view counts and descriptors, array-equal."""
    cams, R, args, names = _case(ft, D)
    lm = _build_both(args, (ft, D))
    at = {names[t]: i for i, t in enumerate(lm["lm_track"].tolist()) if names[t] != "bulk"}
    assert [int(lm["lm_views"][at[f"len{n}"]]) for n in (1, 2, 3, 63, 64, 65)] == [1, 2, 3, 63, 64, 65]
    assert "all_invalid" not in at and "empty" not in at
    assert (lm["lm_desc"][at["half_up"]] == 1).all() and (lm["lm_desc"][at["half_up_254_255"]] == 255).all()
    assert (lm["lm_desc"][at["three_halves"]] == 1).all()
    assert (lm["lm_desc"][at["mean0"]] == 0).all() and (lm["lm_desc"][at["mean255"]] == 255).all()
    assert lm["lm_views"][at["bad_image_inside"]] == 2 and lm["lm_views"][at["bad_feature_inside"]] == 2
    assert lm["lm_home"][at["home_tie_twin_first"]] == 12 and lm["lm_home"][at["home_tie_twin_last"]] == 3
    if ft == 0:
        assert lm["lm_views"][at["outside_with_dist"]] == 2 and "only_outside_with_dist" in at
    else:
        assert lm["lm_views"][at["outside_with_dist"]] == 1 and "only_outside_with_dist" not in at
    assert np.abs(np.linalg.norm(lm["lm_ray"], axis=1) - 1).max() < 1e-15


@pytest.mark.parametrize("ft", [0, 1])
def test_min_views_drops_tracks_one_short(ft):
    cams, R, args, names = _case(ft, 64, min_views=2)
    lm = _build_both(args, ("min_views", ft))
    got = {names[t] for t in lm["lm_track"].tolist()}
    assert "one_valid_of_two" not in got and "single" not in got and "len1" not in got and "len2" in got
    assert (lm["lm_views"] >= 2).all()
    one = lu.harness_build(**dict(args, min_views=1))
    assert {"one_valid_of_two", "single", "len1"} <= {names[t] for t in one["lm_track"].tolist()}


def test_opposite_rays_give_no_landmark():
    """Two references looking in exactly opposite directions (their rotation matrices are an input: diag(1, 1, 1) and
    diag(-1, 1, -1)), a pixel at each principal point: the rays sum to (0, 0, 0), L = 0 / 0 is not finite, no landmark.  A third
    track of one of the two views alone is one."""
    cams = np.zeros((2, 15))
    cams[:, 0] = cams[:, 1] = 2000.0
    cams[:, 2], cams[:, 3] = 960.0, 540.0
    R = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1], [-1, 0, 0, 0, 1, 0, 0, 0, -1]], dtype=np.float64)
    fp = np.array([0, 1, 2], dtype=np.int64)
    desc = np.array([[10, 20], [30, 41]], dtype=np.uint8)
    kp = np.array([[960, 540], [960, 540]], dtype=np.float32)
    args = dict(feat_ptr=fp, desc=desc, kp=kp, ref_cams=cams, trk_ptr=np.array([0, 2, 3, 5]), trk_img=np.array([0, 1, 1, 1, 0]),
                trk_feat=np.zeros(5, dtype=np.int32), ref_R=R)
    lm = _build_both(args, "opposite")
    assert lm["lm_track"].tolist() == [1] and lm["lm_ray"].tolist() == [[0.0, 0.0, -1.0]] and lm["lm_desc"].tolist() == [[30, 41]]


@pytest.fixture(scope="module")
def maps():
    out = {}
    for ft in (0, 1):
        cams, R, args, names = _case(ft, 64, seed=5 + ft)
        lm = lu.harness_build(**args)
        out[ft] = (cams, R, lm, lu.make_queries(lm, names, COUNTS, seed=9 + ft), names)
    return out


def _asm_both(lm, csr, cams, R, what):
    got, want = lu.harness_assemble(lm, ref_cams=cams, ref_R=R, **csr), lu.assemble(lm, ref_cams=cams, ref_R=R, **csr)
    lu.assert_equal(got, want, lu.ASM_KEYS, what)
    return got


@pytest.mark.parametrize("ft", [0, 1])
def test_assemble_harness_equals_numpy(maps, ft):
    """Queries of 0, 1, 63, 64, 65 and 1025 matches, an anchor tie in both orders, a landmark behind the anchor and one 75 degrees
    away: anchors, cameras, kept sets, out_src and the transferred pixels, array-equal."""
    cams, R, lm, csr, names = maps[ft]
    out = _asm_both(lm, csr, cams, R, ft)
    nq = len(csr["match_ptr"]) - 1
    assert out["anchor_ref"][0] == -1 and out["anchor_ref"][7] == -1 and out["match_ptr"][1] == 0
    assert np.array_equal(out["cam_init"][0, 4:], cams[0, 4:]) and out["cam_ref"][0, 2] == lu.S
    assert out["anchor_ref"][nq - 2] == out["anchor_ref"][nq - 1] == np.unique(lm["lm_home"])[0]  # the tie: the lowest reference, either order
    # the landmarks behind and far away are matched by the large query and dropped by the transfer
    big = slice(int(csr["match_ptr"][5]), int(csr["match_ptr"][6]))
    drop = [i for i, t in enumerate(lm["lm_track"].tolist()) if names[t] in ("behind", "far")]
    assert len(drop) == 2 and np.isin(csr["idx_a"][big], drop).any()
    kept = out["src"][int(out["match_ptr"][5]):int(out["match_ptr"][6])]
    assert not np.isin(csr["idx_a"][kept], drop).any() and 0 < len(kept) < 1025
    assert (out["uv_ref"] >= 0).all() and (out["uv_ref"] < 2 * lu.S).all()
    # the hand-made query: [behind, far, some of reference 4's own]; each rule drops its own landmark and only that
    h = nq - 3
    lo = int(csr["match_ptr"][h])
    a = int(out["anchor_ref"][h])
    assert csr["idx_a"][lo:lo + 2].tolist() == drop and a == 4
    assert out["src"][int(out["match_ptr"][h]):int(out["match_ptr"][h + 1])].tolist() == list(range(lo + 2, int(csr["match_ptr"][h + 1])))
    m = lm["lm_ray"][drop] @ R[a].reshape(3, 3).T
    assert m[0, 2] <= 0                                            # behind the anchor: m_z > 0 fails
    px, keep = lu.transfer(R[a], cams[a, 0], lm["lm_ray"][drop])
    assert m[1, 2] > 0 and not keep[1] and not ((px[1] >= 0) & (px[1] < 2 * lu.S)).all()  # in front, its pixel outside [0, 2S)


@pytest.mark.parametrize("ft", [0, 1])
def test_a_querys_bits_alone_reversed_and_split(maps, ft):
    cams, R, lm, csr, _ = maps[ft]
    full = _asm_both(lm, csr, cams, R, ft)
    nq = len(csr["match_ptr"]) - 1
    for qs in [[5], [2], [nq - 3], list(range(nq))[::-1], list(range(0, 4)), list(range(4, nq))]:
        sub, idx = lu.slice_queries(csr, qs)
        part = _asm_both(lm, sub, cams, R, (ft, qs))
        for k, q in enumerate(qs):
            a, b = lu.per_query(part, k), lu.per_query(full, q)
            assert np.array_equal(idx[a["src"]], b["src"]), (qs, q)
            for key in ("anchor_ref", "uv_ref", "uv_cur", "cam_ref", "cam_init"):
                assert np.array_equal(a[key], b[key]), (qs, q, key)


def test_scene_tracks_are_the_scenes_rays(pkg):
    """synth_reloc.scene_tracks: every reference feature in exactly one track, a track's features all of one world ray, its views in
    ascending image order; the indices are those of the descriptor sets, whose distractors belong to no track."""
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=3, n_feat=60, seed=2)
    tp, ti, tf, rays = pkg.synth_reloc.scene_tracks(sc, n_distractors=50)
    assert tp[0] == 0 and tp[-1] == len(sc.ref_track) and (np.diff(tp) >= 1).all() and (np.diff(rays) > 0).all()
    row = sc.ref_ptr[ti] + tf
    assert sorted(row.tolist()) == list(range(len(sc.ref_track)))
    assert np.array_equal(sc.ref_track[row], np.repeat(rays, np.diff(tp)))
    for t in range(len(rays)):
        assert (np.diff(ti[tp[t]:tp[t + 1]]) > 0).all()
    (rp, rd, rk), _ = pkg.synth_reloc.make_reloc_descriptors(sc, D=32, n_distractors=50, seed=1)
    assert np.array_equal(rk[rp[ti] + tf], sc.ref_kp[row])


def test_argument_errors_need_no_device(pkg):
    """PTZ_EINVAL before any device work: NULL arguments of the map's entry points."""
    L = pkg.api.lib()
    h = C.c_void_p()
    cams = np.zeros((1, 15))
    ptr = np.zeros(1, dtype=np.int64)
    assert L.ptz_landmark_map_create(None, cams.ctypes.data_as(C.c_void_p), 1, 0, ptr.ctypes.data_as(C.c_void_p), None, None, 0, 1, 0, C.byref(h)) == -1
    assert L.ptz_landmark_map_create(None, None, 1, 0, None, None, None, 0, 1, 0, None) == -1
    assert L.ptz_landmark_assemble(None, 0, ptr.ctypes.data_as(C.c_void_p), *([None] * 5), 0, *([None] * 8)) == -1
    assert L.ptz_landmark_assemble_device(None, 0, C.c_int64(0), *([None] * 6), 0, *([None] * 8), C.c_int64(0), None) == -1
    assert L.ptz_relocalizer_run_landmarks(None, None, None, 0, None, None, None) == -1
    L.ptz_landmark_assemble_workspace_bytes.restype = C.c_int64
    assert L.ptz_landmark_assemble_workspace_bytes(-1, C.c_int64(0)) == 0 and L.ptz_landmark_assemble_workspace_bytes(3, C.c_int64(100)) % 256 == 0
    assert L.ptz_landmark_map_n_landmarks(None) == 0 and L.ptz_landmark_map_download(None, None, None, None, None, None) == -1
