"""CPU tests of the product's host side: the C-ABI library loads and exports every declared symbol, argument
validation happens before any device work, there is NO CPU fallback (compute entry points fail loudly without
a GPU), the device math agrees with the oracle when instantiated on the host, evaluator / generator / sharding."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------ C-ABI
def test_library_exports_every_declared_symbol(pkg):
    hdr = open(os.path.join(ROOT, "include", "ptz_calib_amd.h")).read()
    names = set(re.findall(r"\b(ptz_[a-z0-9_]+)\s*\(", hdr))
    names -= {"ptz_ba_problem", "ptz_lm_options", "ptz_lm_summary"}
    assert names == set(pkg.api.EXPORTS), names ^ set(pkg.api.EXPORTS)
    lib = pkg.api.lib()
    for n in names:
        assert getattr(lib, n) is not None
    assert "gfx950" in pkg.api.version()


def test_library_does_not_link_the_oracle(pkg):
    import subprocess
    out = subprocess.run(["ldd", pkg.api.LIB_PATH], capture_output=True, text=True).stdout
    assert "ptz_oracle" not in out and "factor_harness" not in out
    syms = subprocess.run(["nm", "-D", pkg.api.LIB_PATH], capture_output=True, text=True).stdout
    assert " orc_" not in syms


def test_options_defaults_are_ceres_114(pkg):
    o = pkg.api.default_options()
    assert (o.max_num_iterations, o.max_num_consecutive_invalid_steps, o.jacobi_scaling) == (200, 5, 1)
    assert (o.initial_trust_region_radius, o.max_trust_region_radius, o.min_trust_region_radius) == (1e4, 1e16, 1e-32)
    assert (o.min_relative_decrease, o.min_lm_diagonal, o.max_lm_diagonal) == (1e-3, 1e-6, 1e32)
    assert (o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance) == (1e-6, 1e-10, 1e-8)


def test_validation_precedes_device_and_no_cpu_fallback(pkg, scene_c1):
    import copy
    api = pkg.api
    # malformed problems are rejected with PTZ_EINVAL whether or not a GPU exists
    bad = copy.copy(scene_c1); bad.obs_ray = scene_c1.obs_ray[::-1].copy()  # not sorted by track
    with pytest.raises(api.PtzError) as e:
        api.BaBatch([bad])
    assert e.value.code == -1
    dd = copy.copy(scene_c1); dd.factor_type = 4  # not a PTZRayOptimizer::FACTOR_TYPE
    with pytest.raises(api.PtzError) as e:
        api.BaBatch([dd])
    assert e.value.code == -4  # PTZ_EUNSUPPORTED
    assert api.lib().ptz_ba_cam_block_dim(0) == 4 and api.lib().ptz_ba_cam_block_dim(1) == 5
    assert api.lib().ptz_ba_cam_block_dim(2) == 6 and api.lib().ptz_ba_cam_block_dim(api.BA_PTZRayDistDisp) == 8
    if api.device_count() == 0:
        # no GPU: the product path must fail loudly, never compute on the CPU
        with pytest.raises(api.PtzError) as e:
            api.ba_solve(scene_c1)
        assert e.value.code == -2  # PTZ_ENODEVICE
        with pytest.raises(api.PtzError) as e:
            api.chol_solve_batch(np.eye(4)[None], np.ones((1, 4)))
        assert e.value.code == -2
        rb = pkg.synth.make_reloc_batch(2, 16)
        with pytest.raises(api.PtzError) as e:
            api.krt_solve_batch(rb)
        assert e.value.code == -2
        with pytest.raises(api.PtzError) as e:
            api.ba_solve_sharded([scene_c1, scene_c1], [0, 1])
        assert e.value.code == -2
        with pytest.raises(api.PtzError) as e:
            api.mfma_f64_peak()
        assert e.value.code == -2
        with pytest.raises(api.PtzError) as e:
            api.hbm_bandwidth()
        assert e.value.code == -2


def test_product_package_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "ptz-calib_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cc", ".cpp")) or f == "Makefile":
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle_py" not in txt and "ptz_oracle" not in txt and "libptz_oracle" not in txt, f


# ------------------------------------------------------------------------------------------------ device math on the host
@pytest.fixture(scope="module")
def harness():
    so = os.path.join(ROOT, "tests", "cpu_harness", "libfactor_harness.so")
    srcs = [os.path.join(ROOT, "tests", "cpu_harness", "factor_harness.cc"), os.path.join(ROOT, "ptz-calib_amd", "csrc", "ptz_factor.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
        import subprocess
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                               os.path.join(ROOT, "tests", "cpu_harness", "factor_harness.cc")])
    return C.CDLL(so)


@pytest.mark.parametrize("ftype", [0, 1])
def test_device_math_matches_oracle(pkg, orc, harness, ftype):
    sc = pkg.synth.make_scene(1, 20, 100, factor_type=ftype)
    cam = sc.cam_init.copy()
    if ftype:
        cam[:, 10] = 0.01
    ray = sc.ray_init * (1.3 if ftype == 0 else 1.0)
    lin = orc.ba_linearize(sc, cam, ray, jacobian_mode=orc.JAC_ANALYTIC)
    nc = 4 if ftype == 0 else 5
    sel = [0, 2, 3, 4] if ftype == 0 else [0, 2, 3, 4, 5]
    W = np.zeros((sc.n_obs, nc, 3)); cost = 0.0
    resd = orc.ba_residuals(sc, cam, ray)
    for a in range(sc.n_obs):
        res = np.zeros(2); Jc = np.zeros((2, nc)); Jr = np.zeros((2, 3)); r2 = np.zeros(2)
        harness.h_ba_linearize(ftype, _p(cam[sc.obs_cam[a]].copy()), _p(ray[sc.obs_ray[a]].copy()), _p(sc.obs_uv[a].copy()), _p(res), _p(Jc), _p(Jr))
        harness.h_ba_residual(ftype, _p(cam[sc.obs_cam[a]].copy()), _p(ray[sc.obs_ray[a]].copy()), _p(sc.obs_uv[a].copy()), _p(r2))
        assert np.array_equal(res, r2) and np.array_equal(res, resd[a])  # bit-identical residual arithmetic
        w = sc.ray_weight[sc.obs_ray[a]]
        W[a] = w * Jc.T @ Jr
        cost += 0.5 * w * res @ res
    assert abs(cost - lin["cost"]) / lin["cost"] < 1e-14
    assert np.abs(W - lin["W"][:, sel, :]).max() / np.abs(W).max() < 1e-13


@pytest.mark.parametrize("ftype", [0, 1, 2])
def test_device_step_direction_equals_jacobian_times_step(harness, ftype):
    """ba_step_dir (the evaluation kernel's one-cross-product form): residual and ray Jacobian identical to ba_linearize,
    camera-side directional derivative equal to Jc v."""
    rng = np.random.default_rng(5 + ftype)
    nc = [4, 5, 6][ftype]
    for _ in range(50):
        cam = np.zeros(15); cam[0] = rng.uniform(1500, 3500); cam[1] = cam[0] * (1.03 if ftype == 2 else 1.0)
        cam[2], cam[3] = 960, 540
        cam[4:7] = rng.normal(0, 0.4, 3)
        if ftype:
            cam[10] = rng.uniform(-0.05, 0.05)
        R = np.zeros(9); Jl = np.zeros(9)
        harness.h_rodrigues(_p(cam[4:7].copy()), _p(R), _p(Jl))
        ray = R.reshape(3, 3).T @ np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), 1.0]) * rng.uniform(0.7, 1.4)
        uv = np.array([rng.uniform(100, 1800), rng.uniform(100, 1000)], dtype=np.float32)
        v = rng.normal(0, 1, nc) * np.array([10.0] * (nc - 3) + [1e-3] * 3)
        res = np.zeros(2); Jc = np.zeros((2, nc)); Jr = np.zeros((2, 3))
        harness.h_ba_linearize(ftype, _p(cam), _p(ray), _p(uv), _p(res), _p(Jc), _p(Jr))
        res2 = np.zeros(2); pd = np.zeros(2); Jr2 = np.zeros((2, 3))
        harness.h_ba_step_dir(ftype, _p(cam), _p(ray), _p(uv), _p(v), _p(res2), _p(pd), _p(Jr2))
        assert np.array_equal(res, res2) and np.array_equal(Jr, Jr2)
        assert np.allclose(pd, Jc @ v, rtol=1e-12, atol=1e-12 * np.abs(Jc @ v).max())


def test_device_displacement_math_matches_oracle(pkg, orc, harness):
    """PTZRayDistDisp (ptzray_optimizer.cc:195-259) device math on the host: residuals bit-identical to the oracle's functor,
    W = Jc^T Jr rows equal to the oracle's closed-form linearisation (columns [f, k1, r, d0, d1, d2]; the oracle also carries
    the reference's always-zero fy column), step direction = Jc v."""
    sc = pkg.synth.make_scene(2, 20, 100, factor_type=3)
    cam = sc.cam_init.copy(); cam[:, 10] = 0.02
    ray = sc.ray_init * 1.2
    d = np.array([0.05, 2e-5, -1e-9])
    lin = orc.ba_linearize(sc, cam, ray, jacobian_mode=orc.JAC_ANALYTIC, disp=d)
    resd = orc.ba_residuals(sc, cam, ray, disp=d)
    sel = [0, 2, 3, 4, 5, 6, 7, 8]
    W = np.zeros((sc.n_obs, 8, 3)); cost = 0.0
    rng = np.random.default_rng(3)
    for a in range(sc.n_obs):
        res = np.zeros(2); Jc = np.zeros((2, 8)); Jr = np.zeros((2, 3)); r2 = np.zeros(2)
        c, x, uv = cam[sc.obs_cam[a]].copy(), ray[sc.obs_ray[a]].copy(), sc.obs_uv[a].copy()
        harness.h_ba_linearize_disp(_p(c), _p(d), _p(x), _p(uv), _p(res), _p(Jc), _p(Jr))
        harness.h_ba_residual_disp(_p(c), _p(d), _p(x), _p(uv), _p(r2))
        assert np.array_equal(res, r2) and np.array_equal(res, resd[a])
        w = sc.ray_weight[sc.obs_ray[a]]
        W[a] = w * Jc.T @ Jr
        cost += 0.5 * w * res @ res
        if a % 17 == 0:
            v = rng.normal(0, 1, 8) * np.array([10.0, 1e-2, 1e-3, 1e-3, 1e-3, 1e-2, 1e-5, 1e-9])
            res3 = np.zeros(2); pd = np.zeros(2); Jr3 = np.zeros((2, 3))
            harness.h_ba_step_dir_disp(_p(c), _p(d), _p(x), _p(uv), _p(v), _p(res3), _p(pd), _p(Jr3))
            assert np.array_equal(res, res3) and np.array_equal(Jr, Jr3)
            assert np.allclose(pd, Jc @ v, rtol=1e-12, atol=1e-12 * np.abs(Jc @ v).max())
    assert abs(cost - lin["cost"]) / lin["cost"] < 1e-14
    assert not lin["W"][:, 1, :].any()  # fy: not read by the 2D-2D functor
    for k in range(8):  # per column: the displacement columns differ by twelve orders of magnitude
        assert np.abs(W[:, k] - lin["W"][:, sel[k], :]).max() / np.abs(W[:, k]).max() < 1e-12, k


def test_device_displacement_2d3d_math_matches_oracle(pkg, orc, harness):
    """Reproj2d3dDispFactor (ptzray_optimizer.cc:334-396): residual equal to the oracle's functor; Jacobian against central
    differences of that functor."""
    rng = np.random.default_rng(11)
    for _ in range(30):
        cam = np.zeros(15); cam[0] = rng.uniform(1500, 3500); cam[1] = cam[0] * rng.uniform(0.97, 1.03); cam[2], cam[3] = 960, 540
        cam[4:7] = rng.normal(0, 0.3, 3); cam[7:10] = rng.normal(0, 1, 3); cam[10] = rng.uniform(-0.05, 0.05)
        tlw = np.concatenate([rng.normal(0, 0.2, 3), rng.normal(0, 2, 3)])
        R = np.zeros(9); Jl = np.zeros(9)
        harness.h_rodrigues(_p(cam[4:7].copy()), _p(R), _p(Jl))
        Rl = np.zeros(9); harness.h_rodrigues(_p(tlw[:3].copy()), _p(Rl), _p(Jl))
        Pc = np.array([rng.uniform(-8, 8), rng.uniform(-5, 5), rng.uniform(40, 80)])
        xyz = Rl.reshape(3, 3).T @ (R.reshape(3, 3).T @ Pc - tlw[3:])
        uv = np.array([rng.uniform(100, 1800), rng.uniform(100, 1000)], dtype=np.float32)
        d = np.array([rng.normal(0, 0.5), rng.normal(0, 1e-4), rng.normal(0, 1e-8)])
        res = np.zeros(2); Jc = np.zeros((2, 9)); Jt = np.zeros((2, 6))
        harness.h_reproj2d3d_disp(_p(cam), _p(d), _p(tlw), _p(xyz), _p(uv), _p(res), _p(Jc), _p(Jt))

        def f(c, dd, t):
            intr = np.concatenate([c[:4], c[10:15]]); out = np.zeros(2)
            orc.lib().orc_res_reproj2d3d_disp(_p(intr), _p(np.ascontiguousarray(dd)), _p(np.ascontiguousarray(c[4:10])), _p(np.ascontiguousarray(t)), _p(uv), _p(xyz), _p(out))
            return out.copy()
        assert np.allclose(res, f(cam, d, tlw), rtol=0, atol=1e-9)
        # central differences in the ambient parameters; rotations through the left Jacobian are checked by the solve tests,
        # here: fx, fy, k1 and the displacement block, and the T_l_w translation
        for col, (idx, h) in enumerate([(0, 1e-2), (1, 1e-2), (10, 1e-3)]):  # (the residual is linear in fy and k1)
            cp, cm = cam.copy(), cam.copy(); cp[idx] += h; cm[idx] -= h
            num = (f(cp, d, tlw) - f(cm, d, tlw)) / (2 * h)
            assert np.allclose(Jc[:, col], num, rtol=1e-6, atol=1e-7 * max(1.0, np.abs(num).max())), (col, Jc[:, col], num)
        for k, h in enumerate([1e-4, 1e-7, 1e-11]):
            dp, dm = d.copy(), d.copy(); dp[k] += h; dm[k] -= h
            num = (f(cam, dp, tlw) - f(cam, dm, tlw)) / (2 * h)
            assert np.allclose(Jc[:, 6 + k], num, rtol=1e-5, atol=1e-6 * np.abs(num).max()), (k, Jc[:, 6 + k], num)
        for k in range(3):
            tp, tm = tlw.copy(), tlw.copy(); tp[3 + k] += 1e-5; tm[3 + k] -= 1e-5
            num = (f(cam, d, tp) - f(cam, d, tm)) / 2e-5
            assert np.allclose(Jt[:, 3 + k], num, rtol=1e-6, atol=1e-6)


def test_device_math_behind_camera_branch(harness):
    cam = np.zeros(15); cam[0] = cam[1] = 2000; cam[2], cam[3] = 960, 540
    res = np.zeros(2); Jc = np.ones((2, 5)); Jr = np.ones((2, 3))
    harness.h_ba_linearize(1, _p(cam), _p(np.array([0.0, 0.0, -1.0])), _p(np.zeros(2, np.float32)), _p(res), _p(Jc), _p(Jr))
    assert np.array_equal(res, [1e6, 1e6]) and not Jc.any() and not Jr.any()  # ptzray_optimizer.cc:97-102


def _krt_reference_residual(orc, ktype, x, k1, d1, uv1, uv2):
    """F / FDist: the oracle's functors.  Fxfy / FxfyDist (krt_optimizer.cc:52-71, 141-192): written out here -- the same
    projection with fy = x[1] instead of fx."""
    out = np.zeros(2)
    if ktype == 0:
        orc.lib().orc_res_2d2d(_p(x), _p(k1), _p(uv1), _p(uv2), _p(out))
        return out
    if ktype == 1:
        orc.lib().orc_res_2d2d_dist(_p(x), _p(k1), _p(d1), _p(uv1), _p(uv2), _p(out))
        return out
    u, v = float(uv1[0]), float(uv1[1])
    if ktype == 3:
        und = np.zeros(2, dtype=np.float32)
        orc.lib().orc_undistort_point(_p(k1), _p(d1), _p(uv1), _p(und))
        if und[0] < 0 or und[0] >= 2 * k1[2] or und[1] < 0 or und[1] >= 2 * k1[3]:
            return out
        u, v = float(und[0]), float(und[1])
    X = np.array([(u - k1[2]) / k1[0], (v - k1[3]) / k1[1], 1.0])
    P = orc.rodrigues(x[4:7]) @ (X / np.linalg.norm(X))
    if ktype == 2:
        return np.array([uv2[0] - (x[0] * P[0] + x[2] * P[2]) / P[2], uv2[1] - (x[1] * P[1] + x[3] * P[2]) / P[2]])
    px, py = P[0] / P[2], P[1] / P[2]
    r2 = px * px + py * py
    rad = 1 + x[10] * r2 + x[11] * r2 ** 2 + x[12] * r2 ** 3
    xd = px * rad + 2 * x[13] * px * py + x[14] * (r2 + 2 * px * px)
    yd = py * rad + 2 * x[14] * px * py + x[13] * (r2 + 2 * py * py)
    return np.array([uv2[0] - (x[0] * xd + x[2]), uv2[1] - (x[1] * yd + x[3])])


@pytest.mark.parametrize("ktype", [0, 1, 2, 3])
def test_device_krt_math_matches_oracle(pkg, orc, harness, ktype):
    rb = pkg.synth.make_reloc_batch(4, 32, seed_id=ktype, factor_type=ktype)
    idx = {0: [0, 4, 5, 6], 1: [0, 4, 5, 6, 10], 2: [0, 1, 4, 5, 6], 3: [0, 1, 4, 5, 6, 10]}[ktype]  # krt_optimizer.cc:321-340
    nf = len(idx)
    for q in range(rb.n_query):
        loc = orc.krt_world_to_local(rb.cam_ref[q], rb.cam_init[q])
        loc[4:7] += [0.01, -0.02, 0.005]
        if ktype & 1:
            loc[10] = 0.01
        if ktype & 2:
            loc[1] = loc[0] * 1.03
        k1 = rb.cam_ref[q, :4].copy(); d1 = rb.cam_ref[q, 10:15].copy()
        for m in range(rb.match_ptr[q], rb.match_ptr[q + 1]):
            res = np.zeros(2); J = np.zeros((2, nf))
            uv1 = rb.uv_ref[m].copy(); uv2 = rb.uv_cur[m].copy()
            harness.h_krt_eval(ktype, _p(loc), _p(k1), _p(d1), _p(uv1), _p(uv2), _p(res), _p(J))
            assert np.allclose(res, _krt_reference_residual(orc, ktype, loc, k1, d1, uv1, uv2), rtol=0, atol=1e-9)
            # Jacobian against central differences of the reference functor
            for c, k in enumerate(idx):
                h = max(1.5e-8, abs(loc[k]) * 1e-6)
                xp = loc.copy(); xp[k] += h
                xm = loc.copy(); xm[k] -= h
                num = (_krt_reference_residual(orc, ktype, xp, k1, d1, uv1, uv2) - _krt_reference_residual(orc, ktype, xm, k1, d1, uv1, uv2)) / (2 * h)
                assert np.allclose(J[:, c], num, rtol=1e-5, atol=1e-4 * max(1.0, np.abs(num).max()))


@pytest.mark.parametrize("ktype", [0, 1, 2, 3])
def test_device_krt_2d3d_math_matches_oracle(pkg, orc, harness, ktype):
    """Factor2d3dDist / Factor2d3dFxfyDist (krt_optimizer.cc:200-249): device residual = the oracle's cv::projectPoints
    restatement (all five distortion coefficients set, so the (k1,k2,p1,p2,k3) reading is exercised, and a non-zero
    local translation), Jacobian = central differences of the oracle functor."""
    rb = pkg.synth.add_reloc_points(pkg.synth.make_reloc_batch(3, 16, seed_id=ktype, factor_type=ktype), n_pt=8)
    idx = {0: [0, 4, 5, 6], 1: [0, 4, 5, 6, 10], 2: [0, 1, 4, 5, 6], 3: [0, 1, 4, 5, 6, 10]}[ktype]
    nf = len(idx)
    for q in range(rb.n_query):
        ref = rb.cam_ref[q].copy(); ref[7:10] = [0.4, -0.2, 0.3]
        cur = rb.cam_init[q].copy(); cur[7:10] = [0.1, 0.25, -0.3]
        loc = orc.krt_world_to_local(ref, cur)
        loc[4:7] += [0.01, -0.02, 0.005]
        loc[10:15] = [0.02, -0.01, 0.003, -0.002, 0.004]
        if ktype & 2:
            loc[1] = loc[0] * 1.03
        Xl = orc.krt_point_to_local(ref, rb.pts3d[rb.point_ptr[q]:rb.point_ptr[q + 1]])
        for i in range(len(Xl)):
            uv = rb.pts2d[rb.point_ptr[q] + i].copy()
            res = np.zeros(2); J = np.zeros((2, nf))
            harness.h_krt_eval_2d3d(ktype, _p(loc), _p(Xl[i]), _p(uv), _p(res), _p(J))
            f = lambda x: orc.res_2d3d_krt(x, ktype & 2, uv, Xl[i])
            assert np.allclose(res, f(loc), rtol=0, atol=1e-9)
            for c, k in enumerate(idx):
                h = max(1.5e-8, abs(loc[k]) * 1e-6)
                xp = loc.copy(); xp[k] += h
                xm = loc.copy(); xm[k] -= h
                num = (f(xp) - f(xm)) / (2 * h)
                assert np.allclose(J[:, c], num, rtol=1e-5, atol=1e-4 * max(1.0, np.abs(num).max()))


def test_oracle_krt_2d3d_known_answers(pkg, orc):
    """Zero residual at the exact projection; the stored distortion (d0..d4) is read as (k1,k2,p1,p2,k3) by
    cv::projectPoints, not as the (k1,k2,k3,p1,p2) of the reference's own functors; F/FDist use fy := fx; the solve
    with both constraint kinds recovers the ground truth and counts both kinds of residuals."""
    cam = np.zeros(15); cam[0] = 2100; cam[1] = 1900; cam[2], cam[3] = 960, 540
    cam[4:7] = [0.02, -0.4, 0.01]; cam[7:10] = [0.3, -0.1, 0.2]; cam[10:15] = [0.03, -0.01, 0.002, -0.001, 0.005]
    X = np.array([1.5, -0.7, 20.0])
    R = orc.rodrigues(cam[4:7])
    P = R @ X + cam[7:10]
    x, y = P[0] / P[2], P[1] / P[2]
    r2 = x * x + y * y
    k1, k2, p1, p2, k3 = cam[10:15]
    cd = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    uv = np.array([xd * cam[0] + cam[2], yd * cam[1] + cam[3]])
    r_fxfy = orc.res_2d3d_krt(cam, 1, uv.astype(np.float32), X)
    assert np.abs(r_fxfy - (uv.astype(np.float32) - uv)).max() < 1e-9
    r_f = orc.res_2d3d_krt(cam, 0, uv.astype(np.float32), X)  # fy := fx
    assert abs(r_f[1] - (float(np.float32(uv[1])) - (yd * cam[0] + cam[3]))) < 1e-9
    # the solve
    for ftype in (0, 3):
        rb = pkg.synth.add_reloc_points(pkg.synth.make_reloc_batch(2, 64, seed_id=11 + ftype, factor_type=ftype), n_pt=10)
        for q in range(rb.n_query):
            s = slice(rb.match_ptr[q], rb.match_ptr[q + 1]); ps = slice(rb.point_ptr[q], rb.point_ptr[q + 1])
            loc0 = orc.krt_world_to_local(rb.cam_ref[q], rb.cam_init[q])
            Xl = orc.krt_point_to_local(rb.cam_ref[q], rb.pts3d[ps])
            la, sa, _ = orc.krt_solve(rb.uv_ref[s], rb.uv_cur[s], rb.cam_ref[q], loc0, factor_type=ftype, pts2d=rb.pts2d[ps],
                                      pts3d_local=Xl, jacobian_mode=orc.JAC_ANALYTIC)
            ln, sn, _ = orc.krt_solve(rb.uv_ref[s], rb.uv_cur[s], rb.cam_ref[q], loc0, factor_type=ftype, pts2d=rb.pts2d[ps],
                                      pts3d_local=Xl, jacobian_mode=orc.JAC_NUMERIC)
            assert sa["num_residuals"] == sn["num_residuals"] == 2 * (64 + 10)
            assert sa["termination_type"] == sn["termination_type"] == 0 and sa["num_iterations"] == sn["num_iterations"]
            assert np.abs(la - ln).max() < 1e-6 * max(1.0, np.abs(ln).max())
            w = orc.krt_local_to_world(rb.cam_ref[q], ln, ftype)
            assert abs(w[0] - rb.cam_gt[q, 0]) / rb.cam_gt[q, 0] < 0.02


def test_device_so3_and_inv3(orc, harness):
    rng = np.random.default_rng(9)
    for _ in range(20):
        r = rng.standard_normal(3) * rng.choice([1e-9, 1e-3, 0.3, 1.2])
        R = np.zeros(9); Jl = np.zeros(9)
        harness.h_rodrigues(_p(r), _p(R), _p(Jl))
        assert np.array_equal(R.reshape(3, 3), orc.rodrigues(r))  # same formula, same arithmetic
        _, dR = orc.rodrigues_jac(r)
        X = rng.standard_normal(3)
        P = R.reshape(3, 3) @ X
        for k in range(3):
            assert np.allclose(np.cross(Jl.reshape(3, 3)[:, k], P), dR[k] @ X, atol=1e-9)
        A = rng.standard_normal((3, 3)); A = A @ A.T + 0.1 * np.eye(3)
        a6 = np.array([A[0, 0], A[1, 0], A[1, 1], A[2, 0], A[2, 1], A[2, 2]]); o6 = np.zeros(6)
        assert harness.h_inv3(_p(a6), _p(o6)) == 1
        Ai = np.linalg.inv(A)
        assert np.allclose(o6, [Ai[0, 0], Ai[1, 0], Ai[1, 1], Ai[2, 0], Ai[2, 1], Ai[2, 2]], rtol=1e-10)
    assert harness.h_inv3(_p(np.array([1.0, 2.0, 1.0, 0, 0, 1.0])), _p(np.zeros(6))) == 0  # not SPD


# ------------------------------------------------------------------------------------------------ evaluator (eval_synthetic.py)
def test_eval_metrics_against_reference_vectors(pkg):
    doc = json.load(open(os.path.join(GOLD, "eval_synthetic_vectors.json")))
    em = pkg.evalmetrics
    for c in doc["ape_cases"]:
        assert em.calc_focal_error(c["pred_f"], c["gt_f"]) == c["focal_error"]
        t, r = em.calc_ape(c["pred_R"], c["pred_t"], c["gt_R"], c["gt_t"])
        assert abs(t - c["ape_trans"]) < 1e-10 * max(1.0, c["ape_trans"])
        assert abs(r - c["ape_rot_deg"]) < 1e-7
    for c in doc["mean_median_cases"]:
        m, md = em.cal_mean_median(c["data"])
        assert abs(m - c["mean"]) < 1e-15 and abs(md - c["median"]) < 1e-15


# ------------------------------------------------------------------------------------------------ generator
def test_splitmix64_known_values(pkg):
    g = pkg.synth.SplitMix64(0)
    # reference outputs of SplitMix64 seeded with 0 (Vigna's splitmix64.c)
    assert [int(v) for v in g.u64(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_scene_generator_is_deterministic(pkg):
    a = pkg.synth.make_scene(0, 20, 100)
    b = pkg.synth.make_scene(0, 20, 100)
    for k in ("obs_uv", "obs_cam", "obs_ray", "ray_weight", "cam_init", "cam_gt", "ray_init"):
        assert np.array_equal(getattr(a, k), getattr(b, k))
    assert a.obs_uv.dtype == np.float32 and a.obs_cam.dtype == np.int32
    assert np.all(np.diff(a.obs_ray) >= 0) and np.bincount(a.obs_ray).min() >= 4  # Filter(4)
    assert np.array_equal(a.ray_weight, np.bincount(a.obs_ray))
    h = hashlib.sha256(a.obs_uv.tobytes() + a.obs_cam.tobytes() + a.obs_ray.tobytes()).hexdigest()
    assert h == json.load(open(os.path.join(GOLD, "lm_trajectories.json")))["ba"][0].get("scene_sha256", h)
    assert np.all(a.cam_init[:, 0] == 2304.0)  # 1.2 * max(w, h), ptz_incremental_optimizer.cc:324


def test_c2_scene_shape(pkg):
    sc = pkg.synth.make_scene(0, 200, 500)
    per_view = np.bincount(sc.obs_cam, minlength=200)
    assert 95_000 < sc.n_obs < 105_000 and per_view.min() > 350 and per_view.max() < 650
    assert sc.meta["track_len_mean"] >= 4


# ------------------------------------------------------------------------------------------------ sharding
def test_shard_range_and_greedy(pkg):
    sh = pkg.sharding
    for n in (0, 1, 7, 8, 1000):
        for w in (1, 2, 3, 8):
            parts = [list(sh.shard_range(n, r, w)) for r in range(w)]
            assert sorted(sum(parts, [])) == list(range(n))
            assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1
    parts = sh.greedy_partition([10, 9, 1, 1, 1, 8], 2)
    assert sorted(sum(parts, [])) == list(range(6))
    loads = [sum([10, 9, 1, 1, 1, 8][i] for i in p) for p in parts]
    assert max(loads) <= (4 / 3) * 15  # LPT bound: <= 4/3 of the optimal makespan (15)


def _gloo_worker(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import __graft_entry__ as ge
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = ge.load_package()
    ids = list(range(5))

    def make(s):
        return pkg.synth.make_scene(s, 12, 40)

    def fake_solve(scenes):  # stands in for BaBatch.solve on a GPU rank: deterministic function of the scene
        cams = [sc.cam_init * (1.0 + 1e-3 * sc.seed % 7) for sc in scenes]
        summ = [dict(termination_type=0, num_iterations=sc.n_obs % 11, final_cost=float(sc.n_ray)) for sc in scenes]
        return cams, summ

    out = pkg.sharding.solve_scenes_sharded(ids, make, fake_solve, dist=dist, cam_width=12)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_solve_gathers_on_every_rank_gloo(pkg):
    """world_size-2 gloo run of the sharding/gather path (the N>1 path of bench.py without GPUs)."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=90) for _ in range(2))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert np.array_equal(res[0], res[1])
    # single-process result is identical
    def make(s):
        return pkg.synth.make_scene(s, 12, 40)
    def fake_solve(scenes):
        cams = [sc.cam_init * (1.0 + 1e-3 * sc.seed % 7) for sc in scenes]
        summ = [dict(termination_type=0, num_iterations=sc.n_obs % 11, final_cost=float(sc.n_ray)) for sc in scenes]
        return cams, summ
    single = pkg.sharding.solve_scenes_sharded(list(range(5)), make, fake_solve, dist=None, cam_width=12)
    assert np.array_equal(single, res[0])


def _closure_chain(mask, perm):
    """Tile-level symbolic factorisation of the permuted mask: returns (closed mask, trsm tiles)."""
    nt = len(mask)
    m = np.zeros((nt, nt), dtype=bool)
    for a in range(nt):
        for e in range(a + 1):
            if mask[a, e]:
                pa, pe = perm[a], perm[e]
                m[max(pa, pe), min(pa, pe)] = True
    for k in range(nt):
        for x in range(k + 1, nt):
            if m[x, k]:
                for y in range(k + 1, x + 1):
                    if m[y, k]:
                        m[x, y] = True
    return m


def _levels(closed, width=4):
    """Earliest step of every block column of a filled structure, at most `width` columns per step (level_schedule)."""
    nt = len(closed)
    level = np.zeros(nt, dtype=int)
    used = np.zeros(nt + 1, dtype=int)
    for t in range(nt):
        lv = 0
        for k in range(t):
            if closed[t, k]:
                lv = max(lv, level[k] + 1)
        while used[lv] >= width:
            lv += 1
        level[t] = lv
        used[lv] += 1
    return level


def _band_mask(nt, band, wrap, tail=1):
    m = np.zeros((nt, nt), dtype=np.uint8)
    free = nt - tail
    for a in range(nt):
        for e in range(a + 1):
            d = a - e
            if d <= band or (wrap and a < free and free - d <= band) or a >= free:
                m[a, e] = 1
    return m


def test_tile_order_planner(pkg):
    """plan_dissection (host logic of ptz_ba_batch_create; no GPU needed): on ring and band tile graphs it returns a
    permutation whose two lanes do not couple -- before and after the fill of the factorisation -- keeps the dense tail in
    place and shortens the chain max(lane) + separator + tail by at least two; graphs that do not fall apart keep the
    natural order."""
    plan = pkg.api.plan_tile_order
    for nt, band, wrap in [(13, 2, True), (13, 2, False), (20, 3, True), (38, 2, True), (9, 1, False), (14, 2, True)]:
        mask = _band_mask(nt, band, wrap)
        planned, perm, (la, lb) = plan(mask, nt - 1)
        assert planned, (nt, band, wrap)
        assert sorted(perm.tolist()) == list(range(nt)) and perm[nt - 1] == nt - 1
        assert la >= lb >= 1
        steps = la + (nt - la - lb)
        assert steps <= nt - 2, (nt, steps)
        closed = _closure_chain(mask.astype(bool), perm)
        # lane A = positions [0, la), lane B = [la, la + lb): no tile couples them, also after fill
        assert not closed[la:la + lb, :la].any()
        # the steps the library reads off the filled structure: columns of one step do not couple, every column comes after
        # the columns it depends on, and the chain is shorter than the lanes-then-separator count whenever a lane was halved again
        level = _levels(closed)
        for a in range(nt):
            for e in range(a):
                if closed[a, e]:
                    assert level[e] < level[a]
        assert level.max() + 1 <= steps
    # the C2 ring: 12 free tiles, band of two, wrap-around -> two lanes of four, each halved again (ends first, middle after),
    # separator of four, tail: 3 + 4 + 1 = 8 steps instead of 13
    mask = _band_mask(13, 2, True)
    planned, perm, lanes = plan(mask, 12)
    assert planned and lanes == (4, 4)
    assert _levels(_closure_chain(mask.astype(bool), perm)).max() + 1 == 8
    # a dense graph, a tiny one, and one whose free part is too short: natural order
    for mask, fd in [(np.tril(np.ones((10, 10), dtype=np.uint8)), 9), (_band_mask(5, 1, False), 4), (_band_mask(13, 6, True), 12)]:
        planned, perm, lanes = plan(mask, fd)
        assert not planned and perm.tolist() == list(range(len(mask))) and lanes == (0, 0)
    # the library's own schedule for the C2 ring: 8 steps, every column once, a column after the columns it depends on, columns
    # of a step without coupling
    planned, perm, lanes = plan(_band_mask(13, 2, True), 12)
    sched = plan.last_schedule
    closed = _closure_chain(_band_mask(13, 2, True).astype(bool), perm)
    assert len(sched) == 8 and sorted(c for c in sched.reshape(-1) if c >= 0) == list(range(13))
    step_of = {int(c): st for st, row in enumerate(sched) for c in row if c >= 0}
    for a in range(13):
        for e in range(a):
            if closed[a, e]:
                assert step_of[e] < step_of[a]
    # more independent pieces than a step has slots (six disconnected three-tile chains): the surplus moves to later steps
    nt = 19
    mask = np.zeros((nt, nt), dtype=np.uint8)
    for t in range(nt):
        mask[t, t] = 1
    for c in range(6):
        mask[3 * c + 1, 3 * c] = mask[3 * c + 2, 3 * c + 1] = 1
    mask[18, :] = 1
    # (no separator needed: the planner sees components only after removing one, so give it a trivial one: tile 0 as prefix)
    planned, perm, lanes = plan(mask, 18)
    if planned:
        sched = plan.last_schedule
        closed = _closure_chain(mask.astype(bool), perm)
        assert sorted(c for c in sched.reshape(-1) if c >= 0) == list(range(nt))
        assert all((row >= 0).sum() <= 4 for row in sched)
        step_of = {int(c): st for st, row in enumerate(sched) for c in row if c >= 0}
        for a in range(nt):
            for e in range(a):
                if closed[a, e]:
                    assert step_of[e] < step_of[a]
        assert len(sched) < nt - 4
    # a tail of several dense tiles (T_l_w block straddling) stays last and in order
    mask = _band_mask(16, 2, True, tail=3)
    planned, perm, (la, lb) = plan(mask, 13)
    assert planned and perm[13:].tolist() == [13, 14, 15]


@pytest.mark.parametrize("ftype", [0, 1, 2, 3])
def test_device_pair_side_equals_linearize(harness, ftype):
    """ba_pair_side -- the factored Jacobians from which k_schur's phase 2 rebuilds the other camera's product row instead of
    gathering it -- against ba_linearize: G with its rotation columns taken through Jl equals Jc, -MR / |X| equals Jr."""
    rng = np.random.default_rng(40 + ftype)
    nc = [4, 5, 6, 8][ftype]
    for it in range(200):
        cam = np.zeros(15); cam[0] = rng.uniform(1500, 3500); cam[1] = cam[0] * (1.03 if ftype == 2 else 1.0)
        cam[2], cam[3] = 960, 540
        cam[4:7] = rng.normal(0, 0.8, 3)
        if ftype:
            cam[10:15] = rng.uniform(-0.05, 0.05, 5) * np.array([1, 0.1, 0.01, 0.01, 0.01])
        d = np.array([0.05, 2e-5, -1e-9]) * rng.uniform(0.5, 1.5) if ftype == 3 else np.zeros(3)
        R = np.zeros(9); Jl = np.zeros(9)
        harness.h_rodrigues(_p(cam[4:7].copy()), _p(R), _p(Jl))
        ray = R.reshape(3, 3).T @ np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), 1.0]) * rng.uniform(0.7, 1.4)
        if ftype == 1 and it % 20 == 0:
            ray = -ray  # behind the camera: zero Jacobians on both paths
        uv = np.array([rng.uniform(100, 1800), rng.uniform(100, 1000)], dtype=np.float32)
        res = np.zeros(2); Jc = np.zeros((2, nc)); Jr = np.zeros((2, 3))
        if ftype == 3:
            harness.h_ba_linearize_disp(_p(cam), _p(d), _p(ray), _p(uv), _p(res), _p(Jc), _p(Jr))
        else:
            harness.h_ba_linearize(ftype, _p(cam), _p(ray), _p(uv), _p(res), _p(Jc), _p(Jr))
        Jc2 = np.zeros((2, nc)); Jr2 = np.zeros((2, 3))
        ok = harness.h_ba_pair_side(ftype, _p(cam), _p(d), _p(ray), _p(Jc2), _p(Jr2))
        if ftype == 1 and it % 20 == 0:
            assert ok == 0 and not Jc.any() and not Jr.any() and not Jc2.any() and not Jr2.any()
            continue
        assert ok == 1
        for k in range(nc):  # per column: the displacement columns are twelve orders of magnitude apart
            assert np.abs(Jc2[:, k] - Jc[:, k]).max() <= 1e-12 * np.abs(Jc[:, k]).max(), (k, Jc, Jc2)
        assert np.abs(Jr2 - Jr).max() <= 1e-12 * np.abs(Jr).max()


def test_scene_generator_reproduces_the_committed_hashes(pkg):
    """synth.make_scene is a deterministic function of its arguments, and the committed fixtures (minima, trajectories) and
    bench.py's workloads are made of its scenes: the generator may get faster (round 3 evaluates only the (view, ray) pairs
    that can be visible), it may not move a bit.  tests/golden/scene_hashes.json was written by the dense round-2 generator
    (tests/golden/gen_scene_hashes.py)."""
    import hashlib
    import json

    def scene_hash(sc):
        h = hashlib.sha256()
        for a in (sc.obs_uv, sc.obs_cam, sc.obs_ray, sc.ray_weight, sc.cam_gt, sc.cam_init, sc.ray_gt, sc.ray_init):
            h.update(a.tobytes())
        h.update(repr((sc.n_cam, sc.n_ray, sc.n_obs)).encode())
        return h.hexdigest()

    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "scene_hashes.json")))
    assert len(cases) >= 15
    for c in cases:
        if c["args"]["n_views"] * c["args"]["obs_per_view"] > 60000 and c["args"]["scene_id"] not in (0, 999):
            continue  # (two of the three C2-sized scenes are enough for the CPU suite's time budget)
        sc = pkg.synth.make_scene(**c["args"])
        assert (sc.n_ray, sc.n_obs) == (c["n_ray"], c["n_obs"]), c["args"]
        assert scene_hash(sc) == c["sha256"], c["args"]


def test_scene_cache_round_trip(pkg, tmp_path):
    """make_scenes(cache_dir=...): scenes written as .npz (no pickle) come back identical, including the ones with shared
    intrinsics; a second call generates nothing."""
    import dataclasses
    for kw in ({}, {"factor_type": 1, "n_intrinsics_groups": 3}):
        a = pkg.synth.make_scenes(range(3), 20, 100, workers=2, cache_dir=str(tmp_path), **kw)
        n_files = len(os.listdir(tmp_path))
        b = pkg.synth.make_scenes(range(3), 20, 100, workers=2, cache_dir=str(tmp_path), **kw)
        assert len(os.listdir(tmp_path)) == n_files
        fresh = [pkg.synth.make_scene(i, 20, 100, **kw) for i in range(3)]
        for x, y, z in zip(a, b, fresh):
            for f in dataclasses.fields(x):
                u, v, w = getattr(x, f.name), getattr(y, f.name), getattr(z, f.name)
                if isinstance(u, np.ndarray):
                    assert np.array_equal(u, v) and np.array_equal(u, w) and u.dtype == v.dtype == w.dtype, f.name
                else:
                    assert u == v == w, f.name
    assert len(os.listdir(tmp_path)) == 6


def test_batch_structure_is_pinned_and_thread_independent(pkg):
    """The host-side structure of a batch (internal ray order, camera-major lists, camera-pair entry lists, k_schur's runs) fixes
    the order of every sum on the device.  Its hash (ptz_debug_host_structure, no GPU needed) must equal the committed one --
    written after the round-3 builder had been compared with round 2's on these scenes, tests/golden/gen_structure_hashes.py --
    and must not depend on the number of builder threads."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_structure_hashes", os.path.join(ROOT, "tests", "golden", "gen_structure_hashes.py"))
    gsh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gsh)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "structure_hashes.json")))
    assert gsh.all_hashes(pkg) == want
    scenes = [pkg.synth.make_scene(**c) for c in gsh.CASES if c.get("factor_type", 0) == 0] + [gsh.shuffled_tracks(pkg)]
    assert len({gsh.structure_hash(pkg, scenes, t) for t in (1, 2, 5, 8)}) == 1


def test_worldcup14_layout_writer(pkg, tmp_path):
    """dataset_io.write_worldcup14_layout: the directory tree the reference's run_ptzba_worldcup14.sh / run_reloc_worldcup14.sh read
    (offline/<MATCH>, offline_matches/<MATCH>, online/<TEST>, online_matches/<TEST> under the reference's names), every test sequence
    matched against images of the match it is relocalised against."""
    import json
    import os
    root = str(tmp_path / "worldcup14")
    info = pkg.dataset_io.write_worldcup14_layout(root, views=(8, 10, 8, 6), obs_per_view=50, n_online=2)
    assert set(info["matches"]) == {"GER_ARG", "GER_POR", "NED_ARG", "USA_GER"} and len(info["tests"]) == 7
    for tag, n in info["matches"].items():
        assert os.path.exists(os.path.join(root, "offline", tag, tag + ".json"))
        assert os.path.exists(os.path.join(root, "offline_matches", tag, "pairs_matches.txt"))
        cams = json.load(open(os.path.join(root, "offline", tag, tag + ".json")))["cameras"]
        assert len(cams) == n and all(c["res"] == [1280, 720] for c in cams.values())
    for ref, test in pkg.dataset_io.WORLDCUP14_TESTS:
        lines = open(os.path.join(root, "online_matches", test, "pairs_matches.txt")).read().split()
        ref_images = set(os.listdir(os.path.join(root, "offline", ref)))
        assert any(tok in ref_images for tok in lines), (ref, test)  # the pairs name images of the reference match
        assert len([f for f in os.listdir(os.path.join(root, "online", test)) if f.endswith(".png")]) == info["tests"][test]


def test_bench_floor_model_of_the_one_rig_iteration_adds_up():
    """bench.py prints, beside the measured microseconds per LM iteration of the C2 rig, the floor of the present structure term by
    term ("so the remaining gap is arithmetic, not prose"): the terms are all there, positive, and the total
    is their sum; the north star's 100 us is below it, which the note says."""
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location("bench_for_floor_model", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    argv = sys.argv
    sys.argv = ["bench.py"]
    try:
        spec.loader.exec_module(bench)
    finally:
        sys.argv = argv
    m = bench.c2_floor_model()
    terms = {k: v for k, v in m.items() if k not in ("total_us", "note", "measured_on")}
    assert "MI355X" in m["measured_on"]  # (the constants are one part's at one clock)
    assert {"chain_pivots", "chain_hand_overs", "back_substitution", "k_eval", "k_schur_f"} <= set(terms)
    assert all(isinstance(v, float) and v > 0 for v in terms.values())
    assert abs(sum(terms.values()) - m["total_us"]) < 0.5 and m["total_us"] > 100.0 and "100 us" in m["note"]


def test_chain_kernel_inline_asm_keeps_wait_states_and_fence_free_hand_overs(tmp_path):
    """the pivot sweep of the diagonal tile (ptz_chol.hip dpp_sweep) is inline asm, which the compiler's hazard
    recogniser does not look into -- a DPP read of a VGPR needs two wait states behind the VALU write of it.  The device code is
    compiled to assembly (cross-compiles without a GPU) and every DPP instruction's source is checked against the two
    instructions before it (tools/check_dpp_hazards.py)."""
    import importlib.util
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path / "chol.s")
    src = os.path.join(ROOT, "ptz-calib_amd", "csrc", "ptz_chol.hip")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--offload-device-only", "-S", src, "-o", out],
                          stderr=subprocess.DEVNULL)
    spec = importlib.util.spec_from_file_location("check_dpp_hazards", os.path.join(ROOT, "tools", "check_dpp_hazards.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n_dpp, bad = mod.scan(out)
    assert n_dpp >= 512, n_dpp   # chol_chain_kernel and chol_col_step_kernel carry the sweep: 16 broadcasts + 240 multiply-adds each
    assert not bad, bad[:5]
    # Round 6: the chain kernel's hand-overs carry no fence -- every handed-over byte is stored write-through (sc1), drained, and read
    # with sc1 loads (ptz_chol.hip ld_sc1 / st_sc1).  What the compiler made of it: no L2 write-back and no L1 invalidate in the kernel,
    # and its plain vector loads are the launch's own inputs only (structure words, bytes, and the workgroup's own C tile: sixteen
    # 8-byte loads) -- a plain load of handed-over bytes added later would read this compute unit's stale L1 copy.
    text = open(out).read()
    name = "_ZN3ptz12_GLOBAL__N_117chol_chain_kernelENS_9CholBatchE"
    begin = text.index("\n" + name + ":")
    body = text[begin:text.index("s_endpgm", begin)]
    assert "buffer_inv" not in body and "buffer_wbl2" not in body, name
    plain = [l.split()[0] for l in body.splitlines() if ("global_load" in l or "flat_load" in l or "buffer_load" in l) and " sc1" not in l]
    assert sum(op == "global_load_dwordx2" for op in plain) == 16, plain        # the workgroup's own C tile (accumulator layout)
    assert all(op in ("global_load_dwordx2", "global_load_dword", "global_load_ubyte", "global_load_ushort", "global_load_sshort") for op in plain), plain
    assert body.count(" sc1") > 100
    # and the checker sees a violation when there is one
    hz = tmp_path / "hazard.s"
    hz.write_text("x:\n\tv_mul_f64 v[2:3], v[2:3], v[4:5]\n\tv_mul_f64 v[8:9], v[2:3], v[4:5]\n"
                  "\tv_fmac_f64_dpp v[6:7], v[2:3], -v[8:9] row_newbcast:3 row_mask:0xf bank_mask:0xf\n")
    assert len(mod.scan(str(hz))[1]) == 1


def test_scene_generator_c_inner_loops_reproduce_the_numpy_form(pkg):
    """Round 6: the generator's two inner loops (candidate pairs, projection + visibility) also exist in C (host/synth_kernels.c,
    -ffp-contract=off) -- 0.37 -> 0.16 s per 200 x 500 scene.  Every array of a scene must have the bits of the numpy form, over the
    shapes the tests and the benchmark use (ring and sector rigs, distortion, shared intrinsics, the dense-window case of tiny rigs)."""
    if pkg.synth._synth_lib() is None:
        pytest.skip("libptzsynth.so not built")
    cfgs = [dict(scene_id=0, n_views=200, obs_per_view=500), dict(scene_id=7, n_views=20, obs_per_view=100),
            dict(scene_id=3, n_views=60, obs_per_view=300, factor_type=1, width=1280, height=720, pan_range_deg=120.0),
            dict(scene_id=11, n_views=40, obs_per_view=150, factor_type=2), dict(scene_id=9, n_views=70, obs_per_view=250, n_intrinsics_groups=3),
            dict(scene_id=21, n_views=2, obs_per_view=40)]
    fields = ("obs_uv", "obs_cam", "obs_ray", "ray_weight", "cam_gt", "cam_init", "ray_gt", "ray_init")
    with_c = [pkg.synth.make_scene(**c) for c in cfgs]
    saved = pkg.synth._SYNTH_LIB
    pkg.synth._SYNTH_LIB = None  # the numpy form
    try:
        plain = [pkg.synth.make_scene(**c) for c in cfgs]
    finally:
        pkg.synth._SYNTH_LIB = saved
    for a, b in zip(with_c, plain):
        assert a.n_ray == b.n_ray
        for f in fields:
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
