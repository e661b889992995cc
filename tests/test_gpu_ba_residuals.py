"""GPU tests of the residual report of a bundle-adjustment batch (ptz_ba_batch_residuals, ptz-calib_amd/csrc/ptz_ba_resid.hip) and
of the selection on it (ptz_ba_batch_trim_select): parity with the CPU oracle's residuals evaluated at the same state, the
per-ray / per-view / per-problem figures against a numpy restatement, a view batch against its packed problem, bit-equality
across batch position and runs, no side effects on the batch, and the error codes."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import ba_cov_georef_util as gu
import ba_trim_util as tu

pytestmark = pytest.mark.gpu

ABS_PX = 1e-9  # |err_px - oracle|: the residual is a handful of FP64 operations on values of about 2e3 (rounding ~1e-12 px)
REL = 1e-9     # the reduced figures, relative

# (scene id, views, obs per view, factor type, annotated)
RIGS = [(5, 6, 40, 0, False), (5, 6, 40, 1, False), (5, 6, 40, 2, False), (5, 20, 100, 0, False), (6, 6, 40, 0, True)]


@functools.lru_cache(maxsize=None)
def _solved(sid, nv, no, ft, annotated):
    """(scene, cam, ray, tlw, report, oracle err [n_obs], oracle err3d [n_obs3d]): the report of a one-problem batch after its solve,
    the oracle's residuals at the state the batch returns"""
    pkg, o = tu.pkg(), tu.orc()
    sc = pkg.synth.make_scene(sid, nv, no, factor_type=ft)
    if annotated:
        # synth.add_annotations yields next to no points on a 6-view rig (its views do not see that ground plane): the annotations
        # come from the generator the georeferenced-covariance tests use, six points on each of four views
        sc = gu.annotate(sc, [0, 2, 3, 5], 6, 0.5)[0]
    b = pkg.api.BaBatch([sc])
    b.set_state()
    b.solve()
    cams, rays = b.get_state()
    tlw = b.last_tlw[0].copy()
    rep = b.residuals()[0]
    b.close()
    res = o.ba_residuals(sc, cams[0], rays[0], tlw=tlw, obs3d=sc.obs3d if annotated else None)
    err = tu.err_norm(res)
    return sc, cams[0].copy(), rays[0].copy(), tlw, rep, err[:sc.n_obs], err[sc.n_obs:]


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), 1e-300)))


@pytest.mark.parametrize("rig", RIGS, ids=lambda r: "scene%d-%dx%d-type%d%s" % (r[0], r[1], r[2], r[3], "-annot" if r[4] else ""))
def test_errors_equal_the_oracle_residuals(rig):
    sc, cam, ray, tlw, rep, err, err3 = _solved(*rig)
    d = float(np.abs(rep["err_px"] - err).max())
    d3 = float(np.abs(rep["err3d_px"] - err3).max()) if rig[4] else 0.0
    print(f"{rig}: max |err_px - oracle| {d:.2e} px over {sc.n_obs} observations (rms {rep['rms']:.3f}), err3d {d3:.2e} px over {len(err3)}")
    assert len(rep["err_px"]) == sc.n_obs and d <= ABS_PX
    if rig[4]:
        assert len(err3) > 0 and len(rep["err3d_px"]) == len(err3) and d3 <= ABS_PX
        # a problem without annotations beside it: its rms3d is NaN, the annotated one's figures do not move
        plain = copy.copy(sc)
        plain.obs3d = None
        b2 = tu.pkg().api.BaBatch([plain, sc])
        b2.set_state(cams=[cam, cam], rays=[ray, ray], tlws=[tlw, tlw])
        r2 = b2.residuals()
        b2.close()
        assert np.isnan(r2[0]["rms3d"]) and len(r2[0]["err3d_px"]) == 0
        assert (r2[1]["err3d_px"] == rep["err3d_px"]).all() and r2[1]["rms3d"] == rep["rms3d"] and (r2[1]["err_px"] == rep["err_px"]).all()
    else:
        assert len(rep["err3d_px"]) == 0 and np.isnan(rep["rms3d"])  # like ComputeErrors
    # ... and before any solve: the state last set
    b = tu.pkg().api.BaBatch([sc])
    b.set_state()
    e0 = b.residuals(only=["err_px"])[0]["err_px"]
    b.close()
    ref0 = tu.err_norm(tu.orc().ba_residuals(sc, sc.cam_init, sc.ray_init, tlw=sc.tlw_init, obs3d=sc.obs3d if rig[4] else None))[:sc.n_obs]
    d0 = float(np.abs(e0 - ref0).max())
    print(f"  initial state: max diff {d0:.2e} px (errors up to {ref0.max():.1f} px)")
    assert d0 <= ABS_PX


@pytest.mark.parametrize("rig", RIGS, ids=lambda r: "scene%d-%dx%d-type%d%s" % (r[0], r[1], r[2], r[3], "-annot" if r[4] else ""))
def test_ray_view_and_problem_figures(rig):
    sc, cam, ray, tlw, rep, err, err3 = _solved(*rig)
    _, _, med, ray_max, ray_worst = tu.select_restated(sc.obs_ray, sc.n_ray, err, 4.0, 3.0)
    assert _rel(rep["ray_max"], ray_max) <= REL
    start = np.searchsorted(sc.obs_ray, np.arange(sc.n_ray + 1))
    clear = np.array([np.diff(np.sort(err[start[r]:start[r + 1]])[-2:]).sum() > 1e-9 if start[r + 1] - start[r] > 1 else True for r in range(sc.n_ray)])
    assert clear.sum() > 0.9 * sc.n_ray and (rep["ray_worst"][clear] == ray_worst[clear]).all()
    assert (rep["ray_max"] == rep["err_px"][rep["ray_worst"]]).all()  # the report is consistent with itself bit for bit
    cnt = np.bincount(sc.obs_cam, minlength=sc.n_cam)
    vrms = np.sqrt(np.bincount(sc.obs_cam, weights=err * err, minlength=sc.n_cam) / cnt)
    vmax = np.array([err[sc.obs_cam == c].max() for c in range(sc.n_cam)])
    assert (rep["view_count"] == cnt).all()
    figs = dict(view_rms=_rel(rep["view_rms"], vrms), view_max=_rel(rep["view_max"], vmax), rms=_rel(rep["rms"], np.sqrt(np.mean(err * err))),
                median=_rel(rep["median"], med))
    if rig[4]:
        figs["rms3d"] = _rel(rep["rms3d"], np.sqrt(np.mean(err3 * err3)))
    print(f"{rig}: relative differences {figs}")
    assert max(figs.values()) <= REL
    # the median is an element of the report's own errors: the exact lower median, bit for bit
    assert rep["median"] == np.sort(rep["err_px"])[(sc.n_obs - 1) // 2]


def test_selection_on_the_device_equals_the_header_on_the_host():
    api = tu.pkg().api
    for case in (tu.CONTAMINATED[0], tu.CONTAMINATED[4], tu.CLEAN + (0.0,)):
        sc = tu.contaminated_scene(*case)[0] if case[4] > 0 else tu.clean_scene(*case[:4])
        b = api.BaBatch([sc])
        b.set_state()
        b.solve()
        rep = b.residuals()[0]
        for trim_px, k_sigma in ((4.0, 3.0), (4.0, 0.0), (0.5, 3.0), (1.0, 12.0)):
            rej, thr, nrej, _ = b.trim_select(trim_px, k_sigma)
            ref = tu.select_host(sc.obs_ray, sc.n_ray, rep["err_px"], trim_px, k_sigma)
            assert (rej[0] == ref[0]).all() and thr[0] == ref[1] and nrej[0] == int(ref[0].sum())
        if case[4] > 0:
            assert nrej[0] > 0
        b.close()


def test_view_batch_gives_the_bits_of_its_packed_problem():
    pkg, o = tu.pkg(), tu.orc()
    sc = pkg.synth.make_scene(7, 12, 60)
    images = [1, 2, 4, 5, 6, 9, 10]
    vp = pkg.api.view_problem(sc, images)
    counts = np.bincount(vp.obs_ray, minlength=vp.n_ray)
    assert (vp.ray_weight > counts).any() and (counts == 1).any()  # weights above the counts; rays with a single candidate observation
    cam, ray = o.ba_solve(vp, jacobian_mode=o.JAC_ANALYTIC)[:2]
    rig = pkg.api.Rig.from_scene(sc)
    vb = pkg.api.ViewBatch([rig], [images], factor_type=0)
    vb.set_state(cams=[cam], rays=[ray])
    pb = pkg.api.BaBatch([vp])
    pb.set_state(cams=[cam], rays=[ray])
    rv = vb.residuals(n_obs=[vp.n_obs], n_ray=[vp.n_ray])[0]
    rp = pb.residuals()[0]
    ref = tu.err_norm(o.ba_residuals(vp, cam, ray))
    assert np.abs(rp["err_px"] - ref).max() <= ABS_PX
    for k in ("err_px", "ray_max", "ray_worst", "view_rms", "view_max", "view_count"):
        assert (rv[k] == rp[k]).all(), k
    assert rv["rms"] == rp["rms"] and rv["median"] == rp["median"]
    sv = vb.trim_select(0.5, 3.0, n_obs=[vp.n_obs], n_ray=[vp.n_ray])
    sp = pb.trim_select(0.5, 3.0)
    assert (sv[0][0] == sp[0][0]).all() and sv[1][0] == sp[1][0] and sv[2][0] == sp[2][0] and sp[2][0] > 0
    # ... and after a solve of both
    vb.solve(); pb.solve()
    rv, rp = vb.residuals(n_obs=[vp.n_obs], n_ray=[vp.n_ray])[0], pb.residuals()[0]
    for k in ("err_px", "ray_max", "ray_worst", "view_rms", "view_max", "view_count"):
        assert (rv[k] == rp[k]).all(), k
    assert rv["rms"] == rp["rms"] and rv["median"] == rp["median"]
    vb.close(); pb.close(); rig.close()


def _same(a, b):
    for k in ("err_px", "ray_max", "ray_worst", "view_rms", "view_max", "view_count"):
        if not (a[k] == b[k]).all():
            return False
    return a["rms"] == b["rms"] and a["median"] == b["median"]


def test_bits_do_not_depend_on_batch_position_or_run():
    api = tu.pkg().api
    sc, cam, ray = _solved(*RIGS[3])[:3]
    a, ca, ra = _solved(*RIGS[0])[:3]
    c = tu.contaminated_scene(*tu.CONTAMINATED[3])[0]
    solo = api.BaBatch([sc])
    solo.set_state(cams=[cam], rays=[ray])
    r1 = solo.residuals()[0]
    r2 = solo.residuals()[0]
    s1 = solo.trim_select(0.5, 3.0)
    three = api.BaBatch([a, sc, c])
    three.set_state(cams=[ca, cam, c.cam_init], rays=[ra, ray, c.ray_init])
    r3 = three.residuals()
    s3 = three.trim_select(0.5, 3.0)
    assert _same(r1, r2) and _same(r1, r3[1])
    assert (s1[0][0] == s3[0][1]).all() and s1[1][0] == s3[1][1] and s1[2][0] == s3[2][1]
    assert len(r3[0]["err_px"]) == a.n_obs and len(r3[2]["err_px"]) == c.n_obs and len(r3[2]["ray_max"]) == c.n_ray
    solo.close(); three.close()


def test_the_report_does_not_disturb_the_batch():
    api = tu.pkg().api
    sc = tu.contaminated_scene(*tu.CONTAMINATED[0])[0]
    plain = api.BaBatch([sc])
    plain.set_state()
    s0 = plain.solve()
    c0, r0 = plain.get_state()
    b = api.BaBatch([sc])
    b.set_state()
    b.residuals()
    b.trim_select()
    s1 = b.solve()
    c1, r1 = b.get_state()
    assert s0 == s1 and (c0[0] == c1[0]).all() and (r0[0] == r1[0]).all()
    b.residuals()
    b.trim_select(4.0, 0.0)
    s2 = b.solve()  # (a solve starts from the state last set)
    c2, r2 = b.get_state()
    assert s0 == s2 and (c0[0] == c2[0]).all() and (r0[0] == r2[0]).all()
    plain.close(); b.close()


def test_null_outputs_and_error_codes():
    api = tu.pkg().api
    sc, cam, ray, _, rep = _solved(*RIGS[0])[:5]
    lib = api.lib()
    b = api.BaBatch([sc])
    none = [None] * 10
    # no state yet
    rms = np.zeros(1)
    assert lib.ptz_ba_batch_residuals(b.handle, *none[:6], tu._p(rms), *none[7:], None) == tu.EINVAL
    assert lib.ptz_ba_batch_trim_select(b.handle, C.c_double(4.0), C.c_double(3.0), None, tu._p(rms), None, None) == tu.EINVAL
    b.set_state(cams=[cam], rays=[ray])
    # all outputs NULL
    assert lib.ptz_ba_batch_residuals(b.handle, *none, None) == tu.EINVAL
    assert lib.ptz_ba_batch_trim_select(b.handle, C.c_double(4.0), C.c_double(3.0), None, None, None, None) == tu.EINVAL
    for tp, ks in ((0.0, 3.0), (-1.0, 3.0), (float("nan"), 3.0), (float("inf"), 3.0), (4.0, -0.5), (4.0, float("nan"))):
        assert lib.ptz_ba_batch_trim_select(b.handle, C.c_double(tp), C.c_double(ks), None, tu._p(rms), None, None) == tu.EINVAL
    # every output alone: the others are skipped, the one asked for has the bits of the full report
    for k in ("err_px", "ray_max", "ray_worst", "view_rms", "view_max", "view_count", "rms", "median", "rms3d"):
        one = b.residuals(only=[k])[0]
        assert all(one[j] is None for j in one if j not in (k, "device_ms")), k
        assert np.array_equal(np.asarray(one[k]), np.asarray(rep[k]), equal_nan=True), k
    b.close()
    # PTZRayDistDisp and shared intrinsics
    d = copy.copy(sc)
    d.factor_type = api.BA_PTZRayDistDisp
    bd = api.BaBatch([d])
    bd.set_state()
    with pytest.raises(api.PtzError) as ei:
        bd.residuals()
    assert ei.value.code == tu.EUNSUPPORTED
    with pytest.raises(api.PtzError) as ei:
        bd.trim_select()
    assert ei.value.code == tu.EUNSUPPORTED
    bd.close()
    s = copy.copy(sc)
    s.ic_of_cam = np.zeros(sc.n_cam, dtype=np.int32)
    bs = api.BaBatch([s])
    bs.set_state()
    with pytest.raises(api.PtzError) as ei:
        bs.residuals()
    assert ei.value.code == tu.EUNSUPPORTED
    bs.close()
