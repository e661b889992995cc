"""GPU tests of the covariance of georeferenced cameras and of the rig's projection centre (ptz_ba_batch_covariance_georef, the
georef kernels of ptz-calib_amd/csrc/ptz_ba_cov.hip) through the C-ABI: parity with the independent restatement of
ba_cov_georef_util.py and with the host harness, batches with a problem that has no annotations, bit-equality across batch
position / order / grouping, gauge independence, no side effects on the batch, the statistics of 400 noisy solves on the device,
the C++ class and the tool."""
import copy
import json
import os
import subprocess

import numpy as np
import pytest

import ba_cov_georef_util as gu
import host_util as hu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-6     # against the restatement: |C_ij - Cref_ij| <= BOUND sqrt(Cref_ii Cref_jj); the sigmas to 1e-9 relative
HARNESS = 1e-10  # against the same algebra on the host
BAND = 4 / np.sqrt(2 * gu.STAT_N)

# the base shape, and a 12 x 60 scene with four annotated views and a non-zero gauge
SHAPES = [(gu.BASE, gu.BASE_CAMS, 0), (gu.BASE, gu.BASE_CAMS, 3), ((7, 12, 60), (1, 4, 7, 10), 5)]


def _scene(shape, cams, ft):
    return gu.solved_scene(*shape, ft, cams)


@pytest.mark.parametrize("factor_type", [0, 1])
@pytest.mark.parametrize("shape,cams,gauge", SHAPES)
def test_parity_with_the_restatement_and_the_harness(pkg, shape, cams, gauge, factor_type):
    sc, cam, ray, tlw = _scene(shape, cams, factor_type)
    st, ref, ref_c, s0, cond = gu.restated(*shape, factor_type, gauge, cams)
    cov, cen, sig, stt = pkg.api.ba_covariance_georef(sc, cam, ray, tlw, gauge_cam=gauge)
    assert st == gu.OK and stt == pkg.api.COV_OK
    d, dc = gu.scaled_diff(cov, ref), gu.scaled_diff(cen[None], ref_c[None])
    hst, hcov, hcen, hs0 = gu.harness_run(sc, cam, ray, tlw, gauge)
    dh, dhc = gu.scaled_diff(cov, hcov), gu.scaled_diff(cen[None], hcen[None])
    print(f"type {factor_type} {shape} anchor {gauge}: restatement {d:.2e} / {dc:.2e}, harness {dh:.2e} / {dhc:.2e}, "
          f"sigma0 rel {np.abs(sig / s0 - 1).max():.1e}, cond {cond:.1e}")
    assert d <= BOUND and dc <= BOUND
    assert hst == gu.OK and dh <= HARNESS and dhc <= HARNESS
    assert (np.abs(sig / s0 - 1) <= 1e-9).all()
    assert (cov == cov.transpose(0, 2, 1)).all() and (cen == cen.T).all()
    assert (np.einsum("cii->ci", cov) > 0).all()  # the anchor's rows are not zero
    # given sigmas: the estimates are returned either way
    _, ref2, refc2, _, _ = gu.restate(sc, cam, ray, tlw, gauge, 0.5, 1.5, check=False)
    cov2, cen2, sig2, st2 = pkg.api.ba_covariance_georef(sc, cam, ray, tlw, gauge_cam=gauge, pixel_sigma=0.5, annotation_sigma=1.5)
    assert st2 == pkg.api.COV_OK and (sig2 == sig).all()
    assert gu.scaled_diff(cov2, ref2) <= BOUND and gu.scaled_diff(cen2[None], refc2[None]) <= BOUND


@pytest.mark.parametrize("factor_type", [0, 1])
def test_gauge_independence_on_the_device(pkg, factor_type):
    sc, cam, ray, tlw = _scene(gu.BASE, gu.BASE_CAMS, factor_type)
    c0, e0, s0, st0 = pkg.api.ba_covariance_georef(sc, cam, ray, tlw, gauge_cam=0)
    c3, e3, s3, st3 = pkg.api.ba_covariance_georef(sc, cam, ray, tlw, gauge_cam=3)
    assert st0 == 0 and st3 == 0
    d, dc = gu.scaled_diff(c3, c0), gu.scaled_diff(e3[None], e0[None])
    print(f"type {factor_type}: gauge 0 against gauge 3 on the device: {d:.2e}, centre {dc:.2e}")
    assert d <= 1e-7 and dc <= 1e-7 and (s0 == s3).all()


def _max_mb(value):
    class Ctx:
        def __enter__(self):
            self.old = os.environ.get("PTZ_BA_COV_MAX_MB")
            os.environ["PTZ_BA_COV_MAX_MB"] = value

        def __exit__(self, *a):
            if self.old is None:
                del os.environ["PTZ_BA_COV_MAX_MB"]
            else:
                os.environ["PTZ_BA_COV_MAX_MB"] = self.old
    return Ctx()


def test_batch_position_order_and_grouping_do_not_change_the_bits(pkg):
    """the base shape, a 12 x 60 scene and a scene without annotations: the third is DOF and untouched; every problem's bits are
    those of the one-shot call alone, in the batch, in reversed order and with every problem a group of its own"""
    a, ca, ra, ta = _scene(gu.BASE, gu.BASE_CAMS, 0)
    b, cb, rb, tb = _scene((7, 12, 60), (1, 4, 7, 10), 0)
    c = copy.copy(pkg.synth.make_scene(2, 6, 40)); c.obs3d = None
    cc, rc, tc = c.cam_init, c.ray_init, np.zeros(6)
    solo = [pkg.api.ba_covariance_georef(s, x, r, t, gauge_cam=g) for s, x, r, t, g in ((a, ca, ra, ta, 2), (b, cb, rb, tb, 5))]
    assert solo[0][3] == 0 and solo[1][3] == 0
    fill = -7.25

    def run(order, env=None):
        scs = [(a, ca, ra, ta, 2), (b, cb, rb, tb, 5), (c, cc, rc, tc, 0)]
        scs = [scs[i] for i in order]
        bt = pkg.api.BaBatch([s[0] for s in scs]); bt.set_state(cams=[s[1] for s in scs], rays=[s[2] for s in scs], tlws=[s[3] for s in scs])
        n = sum(s[0].n_cam for s in scs)
        kw = dict(gauge_cam=[s[4] for s in scs], cov=np.full((n, 4, 4), fill), cov_centre=np.full((3, 3, 3), fill), sigma0=np.full((3, 2), fill))
        if env:
            with _max_mb(env):
                out = bt.covariance_georef(**kw)
        else:
            out = bt.covariance_georef(**kw)
        # the 2D-2D call keeps refusing an annotated batch
        with pytest.raises(pkg.api.PtzError) as refused:
            bt.covariance()
        assert refused.value.code == -4  # PTZ_EUNSUPPORTED
        bt.close()
        covs, cens, sig, st, _ = out
        return {i: (covs[k], cens[k], sig[k], st[k]) for k, i in enumerate(order)}

    for order, env in (((0, 1, 2), None), ((2, 1, 0), None), ((0, 1, 2), "1")):
        got = run(order, env)
        for i in (0, 1):
            assert got[i][3] == 0
            assert (got[i][0] == solo[i][0]).all() and (got[i][1] == solo[i][1]).all() and (got[i][2] == solo[i][2]).all(), (order, env, i)
        assert got[2][3] == pkg.api.COV_DOF
        assert (got[2][0] == fill).all() and (got[2][1] == fill).all() and (got[2][2] == fill).all()


def test_singular_and_dof_leave_the_outputs_untouched(pkg):
    sc, cam, ray, tlw = _scene(gu.BASE, gu.BASE_CAMS, 0)
    fill = -7.25
    three = copy.copy(sc); three.obs3d = {k: v[:3] for k, v in sc.obs3d.items()}
    behind = copy.copy(sc); behind.obs3d = dict(sc.obs3d, xyz=sc.obs3d["xyz"].copy())
    behind.obs3d["xyz"][5] = 2 * gu.centre_of(tlw) - sc.obs3d["xyz"][5]
    for s, want in ((three, pkg.api.COV_DOF), (behind, pkg.api.COV_SINGULAR)):
        cov, cen, sig, st = pkg.api.ba_covariance_georef(s, cam, ray, tlw, cov=np.full((6, 4, 4), fill), cov_centre=np.full((3, 3), fill))
        assert st == want and (cov == fill).all() and (cen == fill).all() and (sig == 0).all()


def test_a_solve_after_the_call_is_the_solve_without_it(pkg):
    scs = [gu.solved_scene(*gu.BASE, 0)[0], gu.solved_scene(7, 12, 60, 0, (1, 4, 7, 10))[0]]
    a = pkg.api.BaBatch(scs); a.set_state(); sa = a.solve(); ca, ra = a.get_state(); ta = a.last_tlw
    b = pkg.api.BaBatch(scs); b.set_state()
    *_, st0, _ = b.covariance_georef()       # at the state last set, before any solve
    sb = b.solve()
    cov1, cen1, s1, st1, _ = b.covariance_georef()   # at the minimum-cost point
    cb, rb = b.get_state(); tb = b.last_tlw
    sb2 = b.solve(); cb2, rb2 = b.get_state(); tb2 = b.last_tlw
    assert list(st0) == [0, 0] and list(st1) == [0, 0]
    assert sa == sb == sb2 and (ta == tb).all() and (ta == tb2).all()
    for i in range(2):
        assert (ca[i] == cb[i]).all() and (ra[i] == rb[i]).all() and (ca[i] == cb2[i]).all() and (ra[i] == rb2[i]).all()
        one, cone, sone, _ = pkg.api.ba_covariance_georef(scs[i], cb[i], rb[i], tb[i])  # one-shot call = batch call, bit for bit
        assert (cov1[i] == one).all() and (cen1[i] == cone).all() and (s1[i] == sone).all()
    a.close(); b.close()


def test_device_covariance_predicts_the_scatter_of_noisy_solves(pkg):
    """The 400 noisy copies of the CPU test as ONE batch through ptz_ba_batch_solve and ptz_ba_batch_covariance_georef, given
    sigmas for the covariance: every ratio observed / predicted lies in 1 +- 4 / sqrt(2 N) = [0.86, 1.14], and so do the means of
    the two estimated levels over the truth (s_a: 0.96 with the restatement, test_cpu_ba_covariance_georef.py)."""
    copies = gu.noisy_copies(0)
    b = pkg.api.BaBatch(copies, function_tolerance=1e-14, parameter_tolerance=1e-12, max_num_iterations=200); b.set_state()
    summ = b.solve()
    assert all(s["termination_type"] == 0 for s in summ)
    cams, _ = b.get_state()
    covs, cens, sig, st, ms = b.covariance_georef(pixel_sigma=gu.SIGMA_F, annotation_sigma=gu.SIGMA_A)
    assert (st == 0).all()
    ratios = gu.stat_ratios(cams, b.last_tlw, covs, cens)
    ratios["s_f"] = sig[:, 0].mean() / gu.SIGMA_F
    ratios["s_a"] = sig[:, 1].mean() / gu.SIGMA_A
    print({k: round(float(v), 3) for k, v in ratios.items()}, f"device {ms:.3f} ms")
    assert len(ratios) == 6 + 6 * 3 + 3 + 2
    for k, v in ratios.items():
        assert 1 - BAND <= v <= 1 + BAND, (k, v)
    b.close()


def _class_solve_world_cov(pkg, sc, cand, ftype, annotations=None):
    """PTZRayOptimizer::Solve, WorldCovariance, WorldStdDevs, WorldCentre and Covariance through the host library's test entry"""
    from ctypes import POINTER, byref, c_double, c_float, c_int32, c_int64
    lib = hu.lib()
    kps, plist = hu.scene_to_features_matches(sc)
    _p = hu._p
    n_img = len(kps)
    kp_ptr = np.concatenate([[0], np.cumsum([len(k) for k in kps])]).astype(np.int64)
    kp_xy = np.ascontiguousarray(np.concatenate([np.asarray(k, dtype=np.float32).reshape(-1, 2) for k in kps]), dtype=np.float32)
    src = np.array([p[0] for p in plist], dtype=np.int64); dst = np.array([p[1] for p in plist], dtype=np.int64)
    mptr = np.concatenate([[0], np.cumsum([len(p[2]) for p in plist])]).astype(np.int64)
    q = np.array([m[0] for p in plist for m in p[2]], dtype=np.int32); t = np.array([m[1] for p in plist for m in p[2]], dtype=np.int32)
    cam = np.array(sc.cam_init, dtype=np.float64, order="C").copy()
    cand = np.array(list(cand), dtype=np.int64)
    ann_ptr = ann_uv = ann_xyz = None
    if annotations is not None:
        acam = np.asarray(annotations["cam"])
        ann_ptr = np.searchsorted(acam, np.arange(n_img + 1)).astype(np.int64)
        ann_uv = np.ascontiguousarray(annotations["uv"], dtype=np.float32); ann_xyz = np.ascontiguousarray(annotations["xyz"], dtype=np.float64)
    nc = len(cand)
    o = dict(cov=np.zeros(25 * nc), cen=np.zeros(9), sd=np.zeros(5 * nc), sc=np.zeros(3), s0=np.zeros(2), centre=np.zeros(3), tlw=np.zeros(6))
    before = c_int32(-1); plain = c_int32(-1); n_obs = c_int32(); n_ray = c_int32(); n_o3 = c_int32()
    puv = POINTER(c_float)(); pcam = POINTER(c_int32)(); pray = POINTER(c_int32)(); pw = POINTER(c_double)()
    pc15 = POINTER(c_double)(); pr3 = POINTER(c_double)(); pci = POINTER(c_int64)()
    o3uv = POINTER(c_float)(); o3xyz = POINTER(c_double)(); o3cam = POINTER(c_int32)()
    code = lib.ptzh_ptzray_solve_world_cov(n_img, _p(kp_ptr), _p(kp_xy), len(plist), _p(src), _p(dst), _p(mptr), _p(q), _p(t), _p(cam), _p(ann_ptr),
                                           _p(ann_uv), _p(ann_xyz), _p(cand), nc, 200, ftype, _p(o["cov"]), _p(o["cen"]), _p(o["sd"]), _p(o["sc"]),
                                           _p(o["s0"]), _p(o["centre"]), _p(o["tlw"]), byref(before), byref(plain), byref(n_obs), byref(n_ray),
                                           byref(puv), byref(pcam), byref(pray), byref(pw), byref(pc15), byref(pr3), byref(pci), byref(n_o3),
                                           byref(o3uv), byref(o3xyz), byref(o3cam))
    no, nr, n3 = n_obs.value, n_ray.value, n_o3.value
    packed = copy.copy(sc)
    packed.n_cam, packed.n_ray, packed.factor_type = nc, nr, ftype
    packed.obs_uv = np.ctypeslib.as_array(puv, (no, 2)).copy(); packed.obs_cam = np.ctypeslib.as_array(pcam, (no,)).copy()
    packed.obs_ray = np.ctypeslib.as_array(pray, (no,)).copy(); packed.ray_weight = np.ctypeslib.as_array(pw, (nr,)).copy()
    packed.obs3d = None if n3 == 0 else dict(uv=np.ctypeslib.as_array(o3uv, (n3, 2)).copy(), xyz=np.ctypeslib.as_array(o3xyz, (n3, 3)).copy(),
                                             cam=np.ctypeslib.as_array(o3cam, (n3,)).copy())
    pcams = np.ctypeslib.as_array(pc15, (nc, 15)).copy(); prays = np.ctypeslib.as_array(pr3, (nr, 3)).copy()
    for x in (puv, pcam, pray, pw, pc15, pr3, pci, o3uv, o3xyz, o3cam):
        lib.ptzh_free(x)
    return code, before.value, plain.value, o, packed, pcams, prays


def test_class_world_covariance_equals_the_batch_call(pkg):
    ann = pkg.synth.add_annotations(pkg.synth.make_scene(1, 20, 100, factor_type=1))
    code, before, plain, o, packed, pcams, prays = _class_solve_world_cov(pkg, ann, range(20), 1, annotations=ann.obs3d)
    assert code == 7 and before == 0 and plain == 0  # Covariance() keeps refusing the annotated problem
    nf = 5
    want, wcen, ws0, st = pkg.api.ba_covariance_georef(packed, pcams, prays, o["tlw"])
    assert st == 0
    assert (o["cov"].reshape(20, nf, nf) == want).all() and (o["cen"].reshape(3, 3) == wcen).all() and (o["s0"] == ws0).all()
    assert (o["sd"].reshape(20, nf) == np.sqrt(np.einsum("cii->ci", want))).all() and (o["sc"] == np.sqrt(np.diag(wcen))).all()
    assert np.abs(o["centre"] - gu.centre_of(o["tlw"])).max() <= 1e-12 * np.abs(o["centre"]).max()
    # a 2D-2D problem: false, before and after the solve
    plain_sc = pkg.synth.make_scene(3, 12, 60)
    code, before, plain, *_ = _class_solve_world_cov(pkg, plain_sc, range(12), 0)
    assert code == 1 and before == 0 and plain == 1


def _run_tool(name, *args):
    exe = os.path.join(ROOT, "ptz-calib_amd", "bin", name)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def rig_files(pkg, tmp_path_factory):
    sc = pkg.synth.add_annotations(pkg.synth.make_scene(1, 20, 100))
    assert sorted(set(sc.obs3d["cam"])) == [0, 12, 15]
    tb = pkg.synth.make_match_table(sc)
    d = tmp_path_factory.mktemp("rig")
    return sc, tb, pkg.dataset_io.write_rig(str(d), sc, tb, annotations=sc.obs3d), d


def test_run_ptz_ba_uncertainty_georeferenced(pkg, rig_files):
    sc, tb, paths, d = rig_files
    out_a, out_b = str(d / "out_a"), str(d / "out_b")
    args = ["-i", paths["images"], "-f", paths["features"], "-a", paths["annotation"]]
    ra = _run_tool("run_ptz_ba", *args, "--output=" + out_a)
    rb = _run_tool("run_ptz_ba", *args, "--output=" + out_b, "--uncertainty")
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr, rb.stderr)
    assert open(os.path.join(out_a, "rig0.json"), "rb").read() == open(os.path.join(out_b, "rig0.json"), "rb").read()
    assert not os.path.exists(os.path.join(out_a, "rig0_uncertainty.json"))
    text = open(os.path.join(out_b, "rig0_uncertainty.json")).read()
    u = json.loads(text)
    # the old keys as before: the same text up to where the new key begins
    assert list(u.keys()) == ["sigma0", "anchor", "images", "georeferenced"]
    assert list(u["images"].keys()) == list(paths["names"]) and 0.3 < u["sigma0"] < 0.8
    g = u["georeferenced"]
    assert list(g.keys()) == ["sigma0_features", "sigma0_annotations", "centre", "sigma_centre", "images"]
    assert list(g["images"].keys()) == list(paths["names"])
    assert (np.array(g["sigma_centre"]) > 0).all() and len(g["centre"]) == 3
    for rec in g["images"].values():
        assert rec["sigma_f"] > 0 and (np.array(rec["sigma_rot_deg"]) > 0).all() and "sigma_k1" not in rec
    # the values are the API's on the same problem: the class from the initial guess reaches the tool's minimum to the solver's
    # tolerances, and its state through the library gives the class's own bits (test above)
    code, _, _, o, packed, pcams, prays = _class_solve_world_cov(pkg, sc, range(20), 0, annotations=sc.obs3d)
    assert code == 7
    cov, cen, s0, st = pkg.api.ba_covariance_georef(packed, pcams, prays, o["tlw"])
    assert st == 0
    sd = np.sqrt(np.einsum("cii->ci", cov))
    got = np.array([[rec["sigma_f"]] + list(np.radians(rec["sigma_rot_deg"])) for rec in g["images"].values()])
    assert (np.abs(got / sd - 1) <= 1e-3).all()
    assert (np.abs(np.array(g["sigma_centre"]) / np.sqrt(np.diag(cen)) - 1) <= 1e-3).all()
    assert abs(g["sigma0_features"] / s0[0] - 1) <= 1e-3 and abs(g["sigma0_annotations"] / s0[1] - 1) <= 1e-3
    cw = gu.centre_of(o["tlw"])  # (a value like the others: to 1e-3 of its size -- two solves meet at the solver's tolerance, not at a bit)
    assert np.abs(np.array(g["centre"]) - cw).max() <= 1e-3 * np.linalg.norm(cw)


def test_run_ptz_ba_uncertainty_with_dist_and_without_annotations(pkg, rig_files):
    sc, tb, paths, d = rig_files
    out_c, out_d = str(d / "out_c"), str(d / "out_d")
    rc = _run_tool("run_ptz_ba", "-i", paths["images"], "-f", paths["features"], "-a", paths["annotation"], "--output=" + out_c, "--uncertainty", "--dist")
    assert rc.returncode == 0, rc.stderr
    g = json.load(open(os.path.join(out_c, "rig0_uncertainty.json")))["georeferenced"]
    assert all(rec["sigma_k1"] > 0 for rec in g["images"].values()) and list(g["images"].keys()) == list(paths["names"])
    # without -a there is no georeferencing stage: the side file of the PTZ-IBA stage alone
    _run_tool("run_ptz_ba", "-i", paths["images"], "-f", paths["features"], "--output=" + out_d, "--uncertainty")
    u = json.load(open(os.path.join(out_d, "rig0_uncertainty.json")))
    assert "georeferenced" not in u and list(u.keys()) == ["sigma0", "anchor", "images"]
