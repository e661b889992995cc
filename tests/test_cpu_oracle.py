"""CPU tests of the oracle (the checker): golden vectors, known answers, internal consistency.
These run without a GPU."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------- tracks: bit-exact against the reference's union-find
def _load_tracks():
    return json.load(open(os.path.join(GOLD, "tracks_reference.json")))["cases"]


@pytest.mark.parametrize("name", sorted(_load_tracks().keys()))
def test_tracks_match_reference_golden(orc, name):
    case = _load_tracks()[name]
    pairs = [(i, j, [tuple(m) for m in ms]) for i, j, ms in case["pairs"]]
    got = orc.tracks_build(pairs, case["min_track_length"])
    want = {int(t): {int(i): f for i, f in v.items()} for t, v in case["tracks"].items()}
    assert got == want  # track ids (union-find roots), membership and ordering are bit-exact


def test_tracks_against_live_reference_build(orc):
    """20 seeded random graphs against the reference's track builder: its outputs stored in tests/golden/ (gen_tracks_random.py),
    and, where oracle/_ref exists (built from the reference tree's own headers), the live build as well."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_tracks_random", os.path.join(GOLD, "gen_tracks_random.py"))
    gtr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gtr)
    cases = json.load(open(os.path.join(GOLD, "tracks_reference_random.json")))["cases"]
    graphs = gtr.graphs()
    assert len(cases) == len(graphs) == 20
    live = orc.ref_tracks_available()
    for (pairs, ml), case in zip(graphs, cases):
        assert gtr.graph_hash(pairs, ml) == case["graph_sha256"] and ml == case["min_track_length"]
        want = {int(t): {int(i): f for i, f in v.items()} for t, v in case["tracks"].items()}
        assert orc.tracks_build(pairs, ml) == want
        if live:
            assert orc.ref_tracks_build(pairs, ml) == want


def test_tracks_empty_input(orc):
    assert orc.tracks_build([(0, 1, [])], 4) == {}


# ---------------------------------------------------------------- Rodrigues (types.cc:41,68 -> cv::Rodrigues)
def test_rodrigues_known_values(orc):
    assert np.array_equal(orc.rodrigues([0, 0, 0]), np.eye(3))
    assert np.array_equal(orc.rodrigues([1e-17, 0, 0]), np.eye(3))  # theta < DBL_EPSILON -> exactly I
    R = orc.rodrigues([0, 0, math.pi / 2])
    assert np.allclose(R, [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    R = orc.rodrigues([1e-9, 0, 0])  # OpenCV's formula with c1 = 1 - cos(theta) (no series branch)
    assert abs(R[2, 1] - 1e-9) < 1e-24 and R[0, 0] == 1.0
    R = orc.rodrigues([math.pi, 0, 0])
    assert np.allclose(R, np.diag([1, -1, -1]), atol=1e-15)


def test_rodrigues_roundtrip_and_jacobian(orc):
    rng = np.random.default_rng(3)
    for _ in range(50):
        r = rng.standard_normal(3)
        r *= rng.uniform(0.01, 3.0) / np.linalg.norm(r)  # angle in (0, pi): the inverse returns the principal value
        R, dR = orc.rodrigues_jac(r)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14)
        assert np.allclose(orc.rodrigues_inv(R), r, atol=1e-12)
        for k in range(3):
            h = 1e-6
            e = np.zeros(3); e[k] = h
            num = (orc.rodrigues(r + e) - orc.rodrigues(r - e)) / (2 * h)
            assert np.allclose(dR[k], num, atol=1e-9)
    _, dR0 = orc.rodrigues_jac([0, 0, 0])  # theta -> 0 branch: [e_k]_x
    assert np.allclose(dR0[0], [[0, 0, 0], [0, 0, -1], [0, 1, 0]])


# ---------------------------------------------------------------- residual known answers
def _cam(f=2000.0, rvec=(0.1, -0.2, 0.05), k1=0.0):
    c = np.zeros(15)
    c[0] = c[1] = f; c[2], c[3] = 960, 540; c[4:7] = rvec; c[10] = k1
    return c


def _res(orc, name, *args):
    out = np.zeros(2)
    getattr(orc.lib(), name)(*[_p(np.ascontiguousarray(a)) for a in args], _p(out))
    return out


def _blocks(cam):
    intr = np.array([cam[0], cam[1], cam[2], cam[3], *cam[10:15]])
    extr = cam[4:10].copy()
    return intr, extr


def test_f1_zero_residual_at_exact_projection(orc):
    cam = _cam()
    intr, extr = _blocks(cam)
    R = orc.rodrigues(cam[4:7])
    X = np.array([0.1, -0.05, 1.0]); X /= np.linalg.norm(X)
    P = R @ X
    uv = np.array([cam[0] * P[0] / P[2] + 960, cam[0] * P[1] / P[2] + 540], dtype=np.float32)
    r = _res(orc, "orc_res_ptzray", intr, extr, X * 3.7, uv)  # ray scale is irrelevant (normalised, :45-46)
    assert np.abs(r).max() < 2e-4  # float32 rounding of the pixel
    intr2 = intr.copy(); intr2[1] = 999.0  # "fy" is ignored by PTZRayFactor (:24-25)
    assert np.array_equal(r, _res(orc, "orc_res_ptzray", intr2, extr, X * 3.7, uv))


def test_f2_penalty_branch_and_distortion(orc):
    cam = _cam(k1=0.03)
    intr, extr = _blocks(cam)
    R = orc.rodrigues(cam[4:7])
    behind = R.T @ np.array([0.0, 0.0, -1.0])
    r = _res(orc, "orc_res_ptzray_dist", intr, extr, behind, np.zeros(2, dtype=np.float32))
    assert np.array_equal(r, [1e6, 1e6])  # ptzray_optimizer.cc:97-102
    X = R.T @ np.array([0.2, 0.1, 1.0])
    x, y = 0.2, 0.1
    rad = 1 + 0.03 * (x * x + y * y)
    uv = np.array([2000 * x * rad + 960, 2000 * y * rad + 540], dtype=np.float32)
    assert np.abs(_res(orc, "orc_res_ptzray_dist", intr, extr, X, uv)).max() < 2e-4
    assert np.abs(_res(orc, "orc_res_ptzray_dist", intr, extr, 2.5 * X, uv)).max() < 2e-4  # scale invariant after /z


def test_f3_ignores_extrinsic_translation_and_reads_fy(orc):
    cam = _cam()
    intr, extr = _blocks(cam)
    tlw = np.array([0.02, -0.01, 0.03, 1.0, 2.0, 30.0])
    xyz = np.array([0.5, -0.3, 2.0]); uv = np.array([1000, 500], dtype=np.float32)
    out = np.zeros(2)
    def f3(i, e):
        orc.lib().orc_res_reproj2d3d(_p(i), _p(e), _p(tlw), _p(uv), _p(xyz), _p(out)); return out.copy()
    r0 = f3(intr, extr)
    e2 = extr.copy(); e2[3:] = [5, 6, 7]
    assert np.array_equal(r0, f3(intr, e2))  # extr t unused (ptzray_optimizer.cc:300)
    i2 = intr.copy(); i2[1] *= 1.1
    r1 = f3(i2, extr)
    assert r1[0] == r0[0] and r1[1] != r0[1]  # fy is live in the 2D-3D factor (:273,320)


def test_f4_f5_known_answers(orc):
    ref = _cam(f=2100.0, rvec=(0, 0, 0))
    cur = _cam(f=2500.0, rvec=(0.02, 0.1, -0.01))
    k1 = ref[:4].copy()
    R = orc.rodrigues(cur[4:7])
    uv1 = np.array([700.0, 400.0], dtype=np.float32)
    ray = np.array([(700 - 960) / 2100, (400 - 540) / 2100, 1.0]); ray /= np.linalg.norm(ray)
    P = R @ ray
    uv2 = np.array([2500 * P[0] / P[2] + 960, 2500 * P[1] / P[2] + 540], dtype=np.float32)
    assert np.abs(_res(orc, "orc_res_2d2d", cur, k1, uv1, uv2)).max() < 2e-4
    # FDist with zero distortion equals F up to the float32 rounding of the undistorted pixel
    d0 = np.zeros(5)
    assert np.abs(_res(orc, "orc_res_2d2d_dist", cur, k1, d0, uv1, uv2)).max() < 2e-4
    # border guard: a reference pixel that undistorts outside [0, 2cx) x [0, 2cy) gives residual 0 (krt_optimizer.cc:97-101)
    dist = np.array([0.8, 0, 0, 0, 0])
    und = np.zeros(2, dtype=np.float32)
    corner = np.array([5.0, 5.0], dtype=np.float32)
    orc.lib().orc_undistort_point(_p(k1), _p(dist), _p(corner), _p(und))
    if und[0] < 0 or und[1] < 0:
        assert np.array_equal(_res(orc, "orc_res_2d2d_dist", cur, k1, dist, corner, uv2), [0, 0])


def test_undistort_inverts_opencv_model(orc):
    """cv::undistortPoints with the reference's quirk: dist (k1,k2,k3,p1,p2) is read by OpenCV as (k1,k2,p1,p2,k3)."""
    k = np.array([2000.0, 2000.0, 960.0, 540.0])
    dist = np.array([-0.04, 0.01, 0.0, 0.0, 0.0])
    x, y = 0.21, -0.13
    r2 = x * x + y * y
    rad = 1 + dist[0] * r2 + dist[1] * r2 * r2
    uv = np.array([2000 * x * rad + 960, 2000 * y * rad + 540], dtype=np.float32)
    out = np.zeros(2, dtype=np.float32)
    orc.lib().orc_undistort_point(_p(k), _p(dist), _p(uv), _p(out))
    assert abs(out[0] - (2000 * x + 960)) < 0.05 and abs(out[1] - (2000 * y + 540)) < 0.05  # 5 fixed-point iterations


# ---------------------------------------------------------------- Jacobians: closed form vs Ceres-style central differences
@pytest.mark.parametrize("ftype", [0, 1])
def test_analytic_vs_numeric_jacobian(pkg, orc, ftype):
    sc = pkg.synth.make_scene(2, 20, 100, factor_type=ftype)
    cam = sc.cam_init.copy()
    if ftype:
        cam[:, 10] = 0.02
    a = orc.ba_linearize(sc, cam, sc.ray_init, jacobian_mode=orc.JAC_ANALYTIC)
    n = orc.ba_linearize(sc, cam, sc.ray_init, jacobian_mode=orc.JAC_NUMERIC)
    for k in ("U", "V", "W", "g_c", "g_r"):
        assert np.abs(a[k] - n[k]).max() / np.abs(a[k]).max() < 1e-7, k
    assert a["cost"] == n["cost"]
    assert np.abs(n["W"][:, 1, :]).max() == 0.0  # dummy fy column is exactly zero in 2D-2D factors


def test_displacement_variant_restatement(pkg, orc):
    """PTZRayDistDisp (ptzray_optimizer.cc:195-259, 334-396; dead from the reference's tools; on the device since round 2, tests/test_gpu_disp.py):
    at zero displacement the functor is PTZRayFxfyDist with fy := fx; the displacement enters the camera-frame z as
    d0 + d1 f + d2 f^2; closed-form and central-difference Jacobians agree, the displacement columns are the same parameter
    for every camera.  On the pure-rotation synthetic rigs the displacement is all but unobservable against the focal
    lengths: the closed-form and the central-difference solves take visibly different paths to the same cost -- the reason
    the device path is held to the closed-form mode for this variant."""
    intr = np.array([2100.0, 1700.0, 960, 540, 0.03, -0.01, 0.002, 0.001, -0.0005]); extr = np.array([0.02, -0.3, 0.01, 1, 2, 3.0])
    ray = np.array([0.2, -0.1, 1.3]); uv = np.array([1000.0, 500.0], dtype=np.float32)
    r0 = np.zeros(2); r1 = np.zeros(2)
    orc.lib().orc_res_ptzray_dist_disp(_p(intr), _p(np.zeros(3)), _p(extr), _p(ray), _p(uv), _p(r0))
    i2 = intr.copy(); i2[1] = i2[0]
    orc.lib().orc_res_ptzray_fxfy_dist(_p(i2), _p(extr), _p(ray), _p(uv), _p(r1))
    assert np.array_equal(r0, r1)
    d = np.array([0.05, 2e-5, -1e-9])
    orc.lib().orc_res_ptzray_dist_disp(_p(intr), _p(d), _p(extr), _p(ray), _p(uv), _p(r0))
    P = orc.rodrigues(extr[:3]) @ (ray / np.linalg.norm(ray)); P[2] += d[0] + d[1] * intr[0] + d[2] * intr[0] ** 2
    x, y = P[0] / P[2], P[1] / P[2]; r2 = x * x + y * y
    rad = 1 + intr[4] * r2 + intr[5] * r2 ** 2 + intr[6] * r2 ** 3
    xd = x * rad + 2 * intr[7] * x * y + intr[8] * (r2 + 2 * x * x); yd = y * rad + 2 * intr[8] * x * y + intr[7] * (r2 + 2 * y * y)
    assert np.allclose(r0, [uv[0] - (intr[0] * xd + 960), uv[1] - (intr[0] * yd + 540)], rtol=0, atol=1e-10)
    # Jacobians of the whole problem at a non-zero displacement
    sc = pkg.synth.make_scene(2, 20, 100, factor_type=3)
    cam = sc.cam_init.copy(); cam[:, 10] = 0.02
    a = orc.ba_linearize(sc, cam, sc.ray_init * 1.2, jacobian_mode=orc.JAC_ANALYTIC, disp=d)
    n = orc.ba_linearize(sc, cam, sc.ray_init * 1.2, jacobian_mode=orc.JAC_NUMERIC, disp=d)
    assert a["ncf"] == 9 and abs(a["cost"] - n["cost"]) <= 1e-14 * n["cost"]  # (x / |x| vs x * (1 / |x|): last-bit differences)
    # Every column but d2 agrees to 1e-6.  Ceres' central-difference step for d2 = 0 is sqrt(eps) = 1.5e-8, which moves the
    # camera-frame z of a UNIT ray by 1.5e-8 f^2 ~ 0.08: the reference's own Jacobian column for d2 carries a truncation
    # error of about a percent, which a closed-form Jacobian cannot (and should not) reproduce.
    for k in ("V", "g_r"):
        assert np.abs(a[k] - n[k]).max() / np.abs(a[k]).max() < 1e-6, k
    assert np.abs(a["U"][:, :8, :8] - n["U"][:, :8, :8]).max() / np.abs(a["U"][:, :8, :8]).max() < 1e-6
    assert np.abs(a["W"][:, :8] - n["W"][:, :8]).max() / np.abs(a["W"][:, :8]).max() < 1e-6
    assert np.abs(a["g_c"][:, :8] - n["g_c"][:, :8]).max() / np.abs(a["g_c"][:, :8]).max() < 1e-6
    rel_d2 = np.abs(a["W"][:, 8] - n["W"][:, 8]).max() / np.abs(a["W"][:, 8]).max()
    assert 1e-4 < rel_d2 < 0.1
    assert np.abs(a["W"][:, 6:9, :]).max() > 0  # the displacement columns are live
    # the solve: both Jacobian modes reach the same cost, along different paths
    da, dn = np.zeros(3), np.zeros(3)
    _, _, _, sa, _ = orc.ba_solve(sc, jacobian_mode=orc.JAC_ANALYTIC, disp=da, num_threads=4)
    _, _, _, sn, _ = orc.ba_solve(sc, jacobian_mode=orc.JAC_NUMERIC, disp=dn, num_threads=4)
    assert sa["termination_type"] == sn["termination_type"] == 0
    assert abs(sa["final_cost"] - sn["final_cost"]) / sn["final_cost"] < 1e-3
    assert da.any() and dn.any()


def test_f1_jacobian_against_sympy(orc):
    """Independent symbolic derivative of PTZRayFactor w.r.t. (f, rvec, ray)."""
    sp = pytest.importorskip("sympy")
    f, r1, r2, r3, x1, x2, x3, u, v, cx, cy = sp.symbols("f r1 r2 r3 x1 x2 x3 u v cx cy", real=True)
    th = sp.sqrt(r1 ** 2 + r2 ** 2 + r3 ** 2)
    k = sp.Matrix([r1, r2, r3]) / th
    K = sp.Matrix([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = sp.cos(th) * sp.eye(3) + (1 - sp.cos(th)) * k * k.T + sp.sin(th) * K
    X = sp.Matrix([x1, x2, x3]); Xn = X / sp.sqrt(x1 ** 2 + x2 ** 2 + x3 ** 2)
    P = R * Xn
    res = sp.Matrix([u - (f * P[0] / P[2] + cx), v - (f * P[1] / P[2] + cy)])
    J = res.jacobian([f, r1, r2, r3, x1, x2, x3])
    fn = sp.lambdify([f, r1, r2, r3, x1, x2, x3, u, v, cx, cy], J, "numpy")
    rng = np.random.default_rng(5)
    lib = orc.lib()
    for _ in range(5):
        cam = _cam(f=rng.uniform(1500, 3500), rvec=rng.standard_normal(3) * 0.4)
        X0 = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), 1.0]) * rng.uniform(0.5, 2)
        uv = np.array([900.0, 500.0], dtype=np.float32)

        class S:  # one-observation scene
            n_cam, n_ray, factor_type = 1, 1, 0
            obs_uv, obs_cam, obs_ray, ray_weight = uv[None], np.zeros(1, np.int32), np.zeros(1, np.int32), np.ones(1)
        lin = orc.ba_linearize(S, cam[None], X0[None], jacobian_mode=orc.JAC_ANALYTIC)
        Jsym = np.array(fn(cam[0], *cam[4:7], *X0, 900.0, 500.0, 960.0, 540.0), dtype=float)
        Jc = Jsym[:, [0, 1, 2, 3]]; Jr = Jsym[:, 4:7]
        # oracle free camera columns: [fx, fy(dummy), r1, r2, r3]
        W_want = Jc.T @ Jr
        assert np.allclose(lin["W"][0][[0, 2, 3, 4]], W_want, rtol=1e-9, atol=1e-9 * np.abs(W_want).max())
        assert np.allclose(lin["V"][0], Jr.T @ Jr, rtol=1e-9, atol=1e-9 * np.abs(Jr.T @ Jr).max())


# ---------------------------------------------------------------- LM: Ceres-1.14 policy
def test_lm_recovers_ground_truth_c1(orc, scene_c1):
    cam, ray, _, s, tr = orc.ba_solve(scene_c1, jacobian_mode=orc.JAC_NUMERIC, trace=True)
    assert s["termination_type"] == orc.CONVERGENCE
    assert s["num_residuals"] == 2 * scene_c1.n_obs
    assert np.abs(cam[:, 0] - scene_c1.cam_gt[:, 0]).mean() < 5.0  # px, at noise level for ~100 obs/view
    assert np.all(np.diff(tr.cost[tr.accepted == 1]) < 0)  # monotonic steps
    # untouched: cx, cy, t, distortion, and the dummy fy (never read by PTZRayFactor -> zero step)
    assert np.array_equal(cam[:, [1, 2, 3, 7, 8, 9, 10, 11, 12, 13, 14]], scene_c1.cam_init[:, [1, 2, 3, 7, 8, 9, 10, 11, 12, 13, 14]])
    # reported error formula (ptzray_optimizer.cc:962-963)
    err = math.sqrt(2) * math.sqrt(2 * s["final_cost"] / s["num_residuals"])
    assert 0.5 < err < 5.0


def test_lm_numeric_and_analytic_trajectories_agree(orc, scene_c1):
    _, _, _, sn, tn = orc.ba_solve(scene_c1, jacobian_mode=orc.JAC_NUMERIC, trace=True)
    _, _, _, sa, ta = orc.ba_solve(scene_c1, jacobian_mode=orc.JAC_ANALYTIC, trace=True)
    assert sn["num_iterations"] == sa["num_iterations"] and np.array_equal(tn.accepted, ta.accepted)
    assert np.allclose(tn.cost, ta.cost, rtol=1e-7)


def test_lm_radius_policy(orc):
    """LevenbergMarquardtStrategy: accepted -> radius / max(1/3, 1 - (2 rho - 1)^3), rejected -> radius / 2, / 4, ..."""
    import __graft_entry__ as ge
    sc = ge.load_package().synth.make_scene(5, 60, 300)
    _, _, _, s, tr = orc.ba_solve(sc, jacobian_mode=orc.JAC_ANALYTIC, trace=True, num_threads=4)
    assert tr.radius[0] == 1e4
    dec = 2.0
    for i in range(1, len(tr.cost)):
        if tr.accepted[i] == 1:
            want = min(1e16, tr.radius[i - 1] / max(1 / 3, 1 - (2 * tr.rho[i] - 1) ** 3)); dec = 2.0
        elif tr.accepted[i] == 0:
            want = tr.radius[i - 1] / dec; dec *= 2
        else:
            want = tr.radius[i - 1] * 0.5
        assert math.isclose(tr.radius[i], want, rel_tol=1e-12)
    assert (tr.accepted == 0).any()  # this seed exercises rejected steps


def test_lm_max_iterations_and_counts(orc, scene_c1):
    _, _, _, s, _ = orc.ba_solve(scene_c1, max_num_iterations=2)
    assert s["termination_type"] == orc.NO_CONVERGENCE and s["num_iterations"] == 2
    assert s["num_successful_steps"] + s["num_unsuccessful_steps"] == s["num_iterations"] + 1


def test_lm_golden_trajectories(pkg, orc):
    doc = json.load(open(os.path.join(GOLD, "lm_trajectories.json")))
    for g in doc["ba"][:2]:  # the two C1-sized cases (the 60-view case is covered by the GPU suite)
        sc = pkg.synth.make_scene(**g["scene"])
        assert (sc.n_obs, sc.n_ray) == (g["n_obs"], g["n_ray"])  # generator is bit-reproducible
        cam, _, _, s, tr = orc.ba_solve(sc, jacobian_mode=orc.JAC_NUMERIC, trace=True, num_threads=1)
        assert s["termination_type"] == g["summary"]["termination_type"]
        assert s["num_iterations"] == g["summary"]["num_iterations"]
        assert tr.accepted.tolist() == g["accepted"]
        assert np.allclose(tr.cost, g["cost"], rtol=1e-9)
        assert np.allclose(cam[:, 0], g["focal"], rtol=1e-9)


def _variant_scene(pkg, g):
    sc = pkg.synth.make_scene(**g["scene"])
    if g["annotated"]:
        sc = pkg.synth.add_annotations(sc)
    if g["fy_scale"] is not None:
        sc.cam_init = sc.cam_init.copy(); sc.cam_init[:, 1] = sc.cam_init[:, 0] * g["fy_scale"]
    return sc


def test_lm_golden_trajectories_of_the_variants(pkg, orc):
    """PTZRayFxfyDist, georeferencing, shared intrinsics, single-view LM with 2D-3D constraints: the oracle reproduces the
    committed trajectories (tests/golden/lm_trajectories_variants.json, oracle/gen_golden_lm_variants.py)."""
    doc = json.load(open(os.path.join(GOLD, "lm_trajectories_variants.json")))
    for g in doc["ba"]:
        sc = _variant_scene(pkg, g)
        assert (sc.n_obs, sc.n_ray) == (g["n_obs"], g["n_ray"])
        kw = dict(obs3d=sc.obs3d, tlw0=sc.tlw_init) if g["annotated"] else {}
        cam, _, tlw, s, tr = orc.ba_solve(sc, jacobian_mode=orc.JAC_NUMERIC, trace=True, num_threads=1, **kw)
        assert s["termination_type"] == g["summary"]["termination_type"] and s["num_iterations"] == g["summary"]["num_iterations"], g["name"]
        assert tr.accepted.tolist() == g["accepted"]
        assert np.allclose(tr.cost, g["cost"], rtol=1e-9)
        assert np.allclose(cam[:, 0], g["focal"], rtol=1e-9) and np.allclose(cam[:, 1], g["fy"], rtol=1e-9)
        assert np.allclose(tlw, g["tlw"], rtol=1e-7, atol=1e-9)
    rbs = {ft: pkg.synth.add_reloc_points(pkg.synth.make_reloc_batch(6, 96, seed_id=40 + ft, factor_type=ft), n_pt=10) for ft in (0, 3)}
    for g in doc["krt_2d3d"]:
        rb = rbs[g["factor_type"]]; q = g["query"]
        sl = slice(rb.match_ptr[q], rb.match_ptr[q + 1]); ps = slice(rb.point_ptr[q], rb.point_ptr[q + 1])
        loc0 = orc.krt_world_to_local(rb.cam_ref[q], rb.cam_init[q])
        loc, s, tr = orc.krt_solve(rb.uv_ref[sl], rb.uv_cur[sl], rb.cam_ref[q], loc0, factor_type=g["factor_type"], pts2d=rb.pts2d[ps],
                                   pts3d_local=orc.krt_point_to_local(rb.cam_ref[q], rb.pts3d[ps]), jacobian_mode=orc.JAC_NUMERIC, trace=True)
        assert s["num_iterations"] == g["summary"]["num_iterations"] and s["num_residuals"] == g["summary"]["num_residuals"]
        assert np.allclose(tr.cost, g["cost"], rtol=1e-9) and np.allclose(loc, g["cam_local"], rtol=1e-9, atol=1e-12)
        assert orc.krt_check(s, loc, 100.0) == g["accepted_by_gates"]


def test_krt_golden_and_gates(pkg, orc):
    doc = json.load(open(os.path.join(GOLD, "lm_trajectories.json")))
    rbs = {ft: pkg.synth.make_reloc_batch(8, 128, seed_id=ft, factor_type=ft) for ft in (0, 1)}
    for g in doc["krt"]:
        rb = rbs[g["factor_type"]]
        q = g["query"]
        sl = slice(rb.match_ptr[q], rb.match_ptr[q + 1])
        loc0 = orc.krt_world_to_local(rb.cam_ref[q], rb.cam_init[q])
        loc, s, tr = orc.krt_solve(rb.uv_ref[sl], rb.uv_cur[sl], rb.cam_ref[q], loc0, factor_type=g["factor_type"],
                                   jacobian_mode=orc.JAC_NUMERIC, trace=True)
        assert s["num_iterations"] == g["summary"]["num_iterations"]
        assert np.allclose(loc, g["cam_local"], rtol=1e-9, atol=1e-12)
        assert orc.krt_check(s, loc, 100.0) == g["accepted_by_gates"]
    # gates of KRTOptimizer::CheckResults (krt_optimizer.cc:504-533)
    s_ok = dict(g["summary"])
    cam = np.array(g["cam_local"])
    assert orc.krt_check(s_ok, cam, 1e9)
    assert not orc.krt_check(s_ok, cam, 1e-9)              # reprojection error gate
    bad = cam.copy(); bad[0] = bad[1] = 10.0               # fov = 2 atan(960 / 10) > 170 deg
    assert not orc.krt_check(s_ok, bad, 1e9)
    s_nc = dict(s_ok); s_nc["termination_type"] = orc.NO_CONVERGENCE
    assert not orc.krt_check(s_nc, cam, 1e9)


def test_krt_frames_roundtrip(orc):
    rng = np.random.default_rng(11)
    ref = _cam(rvec=rng.standard_normal(3) * 0.5); ref[7:10] = [1, 2, 3]
    cur = _cam(f=2600, rvec=rng.standard_normal(3) * 0.5); cur[7:10] = [-1, 0.5, 2]
    loc = orc.krt_world_to_local(ref, cur)
    back = orc.krt_local_to_world(ref, loc, 0)
    assert np.allclose(orc.rodrigues(back[4:7]), orc.rodrigues(cur[4:7]), atol=1e-12)
    assert np.allclose(back[7:10], cur[7:10], atol=1e-12)
    same = orc.krt_world_to_local(ref, ref)  # reloc init: R_cur = R_ref -> local rotation I, rvec 0
    assert np.allclose(same[4:7], 0, atol=1e-15)


# ---------------------------------------------------------------------------------------------------------------------------
# The oracle against minima found by an independent solver (scipy.optimize.least_squares on residuals restated in numpy,
# tests/golden/gen_minima.py -> tests/golden/minima_*.json): pins WHERE the minimum of the reference's objective lies without
# any code of oracle/ -- so "the oracle agrees with itself" is no longer the only statement about the floating-point path.
@pytest.mark.parametrize("name", ["c1", "c1_dist", "m60x300"])
def test_oracle_reaches_the_independent_minimum(pkg, orc, name):
    import minima_util as mu
    m = mu.load(name)
    sc = mu.scene_of(pkg, m)
    for mode in (orc.JAC_NUMERIC, orc.JAC_ANALYTIC):
        cam, ray, _, summ, _ = orc.ba_solve(sc, jacobian_mode=mode, num_threads=8)
        assert summ["termination_type"] == 0
        mu.check_against_minimum(cam, summ, m, tight=False)
    cam, ray, _, summ, _ = orc.ba_solve(sc, jacobian_mode=orc.JAC_ANALYTIC, num_threads=8, **mu.TIGHT)
    mu.check_against_minimum(cam, summ, m, tight=True)


def test_oracle_gradient_vanishes_at_the_independent_minimum(pkg, orc):
    """First-order optimality, checked with the oracle's own Jacobians at scipy's minimum of C1: the gradient there is 1e-9 of
    the gradient at the initial guess (so the two codes agree on the objective AND its derivative)."""
    import minima_util as mu
    m = mu.load("c1")
    sc = mu.scene_of(pkg, m)
    cam = sc.cam_init.copy()
    cam[:, 0] = cam[:, 1] = m["focal"]
    cam[:, 4:7] = m["rvec"]
    lin0 = orc.ba_linearize(sc, sc.cam_init, sc.ray_init)
    lin1 = orc.ba_linearize(sc, cam, np.asarray(m["ray"]))
    g0 = max(np.abs(lin0["g_c"]).max(), np.abs(lin0["g_r"]).max())
    g1 = max(np.abs(lin1["g_c"]).max(), np.abs(lin1["g_r"]).max())
    assert abs(lin1["cost"] - m["cost"]) / m["cost"] < 1e-12
    assert g1 < 1e-8 * g0, (g1, g0)


@pytest.mark.parametrize("ftype", [0, 1])
def test_oracle_krt_reaches_the_independent_minimum(pkg, orc, ftype):
    import json, os
    import minima_util as mu
    gold = json.load(open(os.path.join(mu.GOLD, "minima_reloc.json")))["queries"][str(ftype)]
    rb = pkg.synth.make_reloc_batch(16, 128, seed_id=ftype, factor_type=ftype)
    for q in range(rb.n_query):
        s = slice(rb.match_ptr[q], rb.match_ptr[q + 1])
        loc0 = orc.krt_world_to_local(rb.cam_ref[q], rb.cam_init[q])
        loc, summ, _ = orc.krt_solve(rb.uv_ref[s], rb.uv_cur[s], rb.cam_ref[q], loc0, factor_type=ftype, jacobian_mode=orc.JAC_NUMERIC, **mu.TIGHT)
        w = orc.krt_local_to_world(rb.cam_ref[q], loc, ftype)
        g = gold[q]
        assert abs(summ["final_cost"] - g["cost"]) / g["cost"] < 1e-9
        assert abs(w[0] - g["focal"]) / g["focal"] < 1e-7
        assert np.abs(orc.rodrigues(w[4:7]) - np.asarray(g["R_world"])).max() < 1e-7
        if ftype:
            assert abs(w[10] - g["k1"]) < 1e-7


def test_oracle_krt_batch_driver_equals_the_per_query_calls(pkg, orc):
    """orc_krt_solve_batch (the relocalization loop of run_ptz_reloc.cc:68-118 over packed queries; the CPU baseline of the
    benchmark's C5 leg) gives, query by query, what the single-query entry points give, for any thread count."""
    rb = pkg.synth.make_reloc_queries(48, 96, seed_id=3, factor_type=1)
    cam1, summ1, acc1 = orc.krt_solve_batch(rb, num_threads=1, jacobian_mode=orc.JAC_NUMERIC)
    cam4, summ4, acc4 = orc.krt_solve_batch(rb, num_threads=4, jacobian_mode=orc.JAC_NUMERIC)
    assert np.array_equal(cam1, cam4) and summ1 == summ4 and np.array_equal(acc1, acc4)
    for q in (0, 7, 19, 47):
        s = slice(rb.match_ptr[q], rb.match_ptr[q + 1])
        loc0 = orc.krt_world_to_local(rb.cam_ref[q], rb.cam_init[q])
        loc, osumm, _ = orc.krt_solve(rb.uv_ref[s], rb.uv_cur[s], rb.cam_ref[q], loc0, factor_type=1, jacobian_mode=orc.JAC_NUMERIC)
        good = orc.krt_check(osumm, loc, 100.0)
        assert osumm == summ1[q] and bool(acc1[q]) == good
        want = orc.krt_local_to_world(rb.cam_ref[q], loc, 1) if good else rb.cam_init[q]
        assert np.array_equal(cam1[q], want)
