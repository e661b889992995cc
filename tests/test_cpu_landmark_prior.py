"""CPU tests of the landmark view's contract: the shared header (ptz-calib_amd/csrc/ptz_landmark_prior.h) instantiated on the host by
tests/cpu_harness/landmark_prior_harness.cc against the numpy restatement (landmark_prior_util.py), array-equal on vis_ptr, vis_lm
and vis_uv with no ulp bound; the true camera as a prior against the scene's own query pixels; and the argument errors of the
C-ABI that need no device."""
import ctypes as C

import numpy as np
import pytest

import landmark_prior_util as lp
import landmark_util as lu
import reloc_assemble_util as ru

N_LM, N_QUERY = 700, 7


def _both(rays, cams, wh, ft, radius_px=40.0, what=""):
    R = ru.harness_rotations(cams) if len(cams) else np.zeros((0, 9))
    got = lp.harness_visible(rays, cams, wh, ft, radius_px, prior_R=R)
    want = lp.visible(rays, cams, wh, ft, radius_px, prior_R=R)
    lp.assert_equal(got, want, what)
    return got


@pytest.mark.parametrize("ft", [0, 1, 2, 3])
@pytest.mark.parametrize("radius_px", [40.0, 7.5])
def test_harness_equals_numpy(ft, radius_px):
    """F / FDist / Fxfy / FxfyDist priors with a distortion (which must not enter) and fy != fx (which enters for the last two):
    rays a quarter pixel inside and outside each of the four margins of query 0, one on its axis, one behind it, rays with NaN,
    infinite, huge and zero components, a query that looks the other way and one that sees nothing."""
    rays, cams, wh = lp.make_case(N_LM, N_QUERY, ft, seed=3 + ft, radius_px=radius_px)
    v = _both(rays, cams, wh, ft, radius_px, (ft, radius_px))
    q0 = lp.per_query(v, 0)["vis_lm"].tolist()
    assert [l in q0 for l in range(10)] == [True, False, True, False, True, False, True, False, True, False], q0[:10]
    n = np.diff(v["vis_ptr"])
    assert n[N_QUERY // 2] == 0 and n[0] > 10 and n[-1] > 0, n
    for q in range(N_QUERY):
        assert (np.diff(lp.per_query(v, q)["vis_lm"]) > 0).all()  # ascending landmark index
    # the nasty rays (indices 10 .. 22): only the finite ones in front are ever seen
    nasty = rays[10:23]
    bad = ~np.isfinite(nasty).all(axis=1)
    assert not np.isin(v["vis_lm"], 10 + np.nonzero(bad)[0]).any()
    uv = lp.per_query(v, 0)["vis_uv"]
    assert (uv[:, 0] >= -radius_px).all() and (uv[:, 0] < wh[0, 0] + radius_px).all() and (uv[:, 1] >= -radius_px).all() and (uv[:, 1] < wh[0, 1] + radius_px).all()


def test_fy_enters_for_two_focal_types_only():
    rays, cams, wh = lp.make_case(N_LM, 3, 0, seed=11)
    R = ru.harness_rotations(cams)
    one, two = lp.harness_visible(rays, cams, wh, 0, prior_R=R), lp.harness_visible(rays, cams, wh, 2, prior_R=R)
    lp.assert_equal(one, lp.harness_visible(rays, cams, wh, 1, prior_R=R), "F = FDist")
    lp.assert_equal(two, lp.harness_visible(rays, cams, wh, 3, prior_R=R), "Fxfy = FxfyDist")
    a, b = lp.per_query(one, 0), lp.per_query(two, 0)  # a landmark both see: the same u, another v
    _, ia, ib = np.intersect1d(a["vis_lm"], b["vis_lm"], return_indices=True)
    assert len(ia) > 10 and np.array_equal(a["vis_uv"][ia, 0], b["vis_uv"][ib, 0]) and (a["vis_uv"][ia, 1] != b["vis_uv"][ib, 1]).mean() > 0.9
    same = cams.copy()
    same[:, 10:] = 0.0  # the prior's distortion does not enter
    lp.assert_equal(one, lp.harness_visible(rays, same, wh, 0, prior_R=R), "distortion")


@pytest.mark.parametrize("ft", [0, 3])
def test_a_querys_bits_alone_reversed_and_split(ft):
    rays, cams, wh = lp.make_case(N_LM, N_QUERY, ft, seed=20 + ft)
    full = _both(rays, cams, wh, ft, what=ft)
    for qs in [[0], [N_QUERY // 2], [N_QUERY - 1], list(range(N_QUERY))[::-1], list(range(0, 3)), list(range(3, N_QUERY))]:
        part = _both(rays, cams[qs], wh[qs], ft, what=(ft, qs))
        for k, q in enumerate(qs):
            a, b = lp.per_query(part, k), lp.per_query(full, q)
            assert np.array_equal(a["vis_lm"], b["vis_lm"]) and np.array_equal(a["vis_uv"].view(np.uint32), b["vis_uv"].view(np.uint32)), (qs, q)


def test_empty_inputs_and_capacity():
    rays, cams, wh = lp.make_case(N_LM, 4, 0, seed=1)
    none = _both(rays[:0], cams, wh, 0, what="no landmarks")
    assert none["vis_ptr"].tolist() == [0] * 5 and len(none["vis_lm"]) == 0
    noq = _both(rays, cams[:0], wh[:0], 0, what="no queries")
    assert noq["vis_ptr"].tolist() == [0]
    full = lp.harness_visible(rays, cams, wh, 0)
    cut = lp.harness_visible(rays, cams, wh, 0, capacity=17)
    assert np.array_equal(cut["vis_ptr"], full["vis_ptr"]) and np.array_equal(cut["vis_lm"], full["vis_lm"][:17]) and len(cut["vis_uv"]) == 17


def test_true_camera_predicts_the_scenes_query_pixels(pkg):
    """The map of a synthetic scene (F: no distortion anywhere), the queries' TRUE cameras as priors: a landmark whose world ray a
    query observes is predicted where the query saw it.  Both pixels carry Gaussian noise of 0.5 px per axis -- the query's own and,
    through the ray, the references' (averaged over a track's views, so at most 0.5) -- hence a difference of sigma <= 0.71 px per
    axis: the median distance is bounded by 1.5 px and the largest, over some thousand pairs, by 5 px (seven sigma)."""
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=6, n_feat=200, noise_px=0.5, seed=4)
    tp, ti, tf, trk_ray = pkg.synth_reloc.scene_tracks(sc)
    lm = lu.build(sc.ref_ptr, np.zeros((len(sc.ref_kp), 1), dtype=np.uint8), sc.ref_kp, rig, tp, ti, tf)
    v = _both(lm["lm_ray"], sc.cam_gt, sc.query_wh, 0, what="scene")
    ray_of_lm = trk_ray[lm["lm_track"]]
    dist, seen = [], 0
    for q in range(sc.n_query):
        sl = slice(int(sc.query_ptr_feat[q]), int(sc.query_ptr_feat[q + 1]))
        pq = lp.per_query(v, q)
        at = {int(r): i for i, r in enumerate(ray_of_lm[pq["vis_lm"]].tolist())}
        for track, kp in zip(sc.query_track[sl].tolist(), sc.query_kp[sl]):
            if track in set(ray_of_lm.tolist()):
                assert track in at, (q, track)  # a landmark the query observes is in its view
                dist.append(float(np.linalg.norm(pq["vis_uv"][at[track]].astype(np.float64) - kp)))
        seen += len(pq["vis_lm"])
    dist = np.asarray(dist)
    print(f"true-camera prediction: {len(dist)} pairs, median {np.median(dist):.3f} px, max {dist.max():.3f} px; {seen} visible of {len(ray_of_lm)} landmarks x 6")
    assert len(dist) > 500 and np.median(dist) < 1.5 and dist.max() < 5.0, (len(dist), np.median(dist), dist.max())


def test_argument_errors_need_no_device(pkg):
    """PTZ_EINVAL / PTZ_EUNSUPPORTED before any device work: what can be said without a map (which needs a device) -- NULL handles,
    and every check of the device form, whose pointers are not read before they are validated (host addresses stand in)."""
    L = pkg.api.lib()
    h = C.c_void_p()
    cams, R, wh = np.ones((1, 15)), np.zeros((1, 9)), np.full((1, 2), 100, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    o = pkg.api.landmark_prior_options()
    assert o.radius_px == 40.0 and o.max_view_bytes == 2 << 30
    with pytest.raises(TypeError):
        pkg.api.landmark_prior_options(radius=3)
    assert L.ptz_landmark_visible(None, 1, p(cams), p(R), p(wh), 0, C.byref(o), C.byref(h)) == -1 and not h
    assert L.ptz_landmark_visible(None, 0, None, None, None, 0, None, None) == -1
    L.ptz_landmark_view_n_visible.restype = C.c_int64
    L.ptz_landmark_view_device_ms.restype = C.c_double
    L.ptz_landmark_view_desc_set.restype = C.c_void_p
    assert L.ptz_landmark_view_n_visible(None) == 0 and L.ptz_landmark_view_device_ms(None) == 0.0 and not L.ptz_landmark_view_desc_set(None)
    assert L.ptz_landmark_view_download(None, None, None, None) == -1 and L.ptz_landmark_view_device_ptrs(None, None, None, None) == -1
    L.ptz_landmark_view_destroy.restype = None
    L.ptz_landmark_view_destroy(None)
    assert L.ptz_relocalizer_run_landmarks_tracked(None, None, None, 0, None, None, None, None, None, None) == -1
    assert L.ptz_relocalizer_view(None, None, None, None, None) == -1
    L.ptz_landmark_visible_workspace_bytes.restype = C.c_int64
    assert L.ptz_landmark_visible_workspace_bytes(-1, 0) == 0 and L.ptz_landmark_visible_workspace_bytes(0, -1) == 0
    ws = L.ptz_landmark_visible_workspace_bytes(2049, 257)
    assert ws % 256 == 0 and ws >= 4 * 257 * 3 + 4 * 257
    assert L.ptz_landmark_visible_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1) == 0  # more (query, tile) workgroups than a launch has
    rays, ptr, buf = np.zeros((4, 3)), np.zeros(2, dtype=np.int64), np.zeros(4096, dtype=np.uint8)
    lm, uv = np.zeros(8, dtype=np.int32), np.zeros((8, 2), dtype=np.float32)
    al = (buf.ctypes.data + 255) & ~255

    def dev(n_lm=4, ray=rays, n_query=1, pc=cams, pr=R, qwh=wh, ft=0, radius=40.0, vptr=ptr, vlm=lm, vuv=uv, cap=8, w=al, wb=2048):
        g = lambda a: None if a is None else p(a)
        return L.ptz_landmark_visible_device(n_lm, g(ray), n_query, g(pc), g(pr), g(qwh), ft, C.c_double(radius), g(vptr), g(vlm), g(vuv),
                                             C.c_int64(cap), C.c_void_p(w) if w else None, C.c_int64(wb), None)

    for bad in (dict(n_lm=-1), dict(n_query=-1), dict(cap=-1), dict(vptr=None), dict(w=0), dict(ray=None), dict(pc=None), dict(pr=None),
                dict(qwh=None), dict(vlm=None), dict(vuv=None), dict(radius=0.0), dict(radius=-3.0), dict(radius=float("nan")),
                dict(radius=float("inf")), dict(w=al + 8), dict(wb=0)):
        assert dev(**bad) == -1, bad
    assert dev(ft=4) == -4 and dev(ft=-1) == -4
    assert dev(n_lm=2 ** 31 - 1, n_query=2 ** 31 - 1) == -5
    with pytest.raises(ValueError):
        pkg.api.Relocalizer.run(None, None, np.zeros((1, 2)), landmark_prior=dict(cams=cams))  # landmark_prior without landmarks
