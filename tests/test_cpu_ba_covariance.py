"""CPU tests of the per-view covariance of bundle-adjusted cameras (ptz_ba_batch_covariance): the algebra of
ptz-calib_amd/csrc/ptz_ba_cov.h -- the header the kernels of ptz_ba_cov.hip instantiate -- compiled for the host and finished in
plain loops (tests/cpu_harness/ba_cov_harness.cc) equals the independent restatement on the oracle's residuals (ba_cov_util.py);
the status rules; the C-ABI's checks that come before any device work; and the statistics of the restated covariance itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ba_cov_util as bu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -4
BOUND = 1e-6  # |C_ij - Cref_ij| <= BOUND sqrt(Cref_ii Cref_jj): the project's bound for covariances (test_cpu_krt_covariance.py)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(ROOT, "tests", "cpu_harness", "libba_cov_harness.so")
    src = os.path.join(ROOT, "tests", "cpu_harness", "ba_cov_harness.cc")
    srcs = [src] + [os.path.join(ROOT, "ptz-calib_amd", "csrc", h) for h in ("ptz_ba_cov.h", "ptz_factor.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    lib = C.CDLL(so)
    lib.ba_cov_harness_status.argtypes = [C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32]
    return lib


def _harness_run(lib, sc, cam, ray, gauge, pixel_sigma=0.0, cov=None, sigma0=None):
    uv, oc, orr, w = bu.problem_args(sc)
    nf = bu.NF[sc.factor_type]
    cov = np.zeros((sc.n_cam, nf, nf)) if cov is None else cov
    sg = C.c_double(0.0 if sigma0 is None else sigma0)
    cam = np.ascontiguousarray(cam, dtype=np.float64); ray = np.ascontiguousarray(ray, dtype=np.float64)
    st = lib.ba_cov_harness_run(sc.factor_type, sc.n_cam, sc.n_ray, C.c_int64(len(oc)), _p(uv), _p(oc), _p(orr), _p(w), _p(cam), _p(ray),
                                int(gauge), C.c_double(pixel_sigma), _p(cov), C.byref(sg))
    return st, cov, sg.value


@pytest.mark.parametrize("factor_type,shape,gauge", [(0, (6, 40), 0), (1, (6, 40), 3), (2, (6, 40), 5), (0, (20, 100), 10)])
def test_header_algebra_equals_the_restatement(harness, factor_type, shape, gauge):
    sc, cam, ray = bu.solved_scene(5, shape[0], shape[1], factor_type)
    st, ref, s0, cond = bu.restated(5, shape[0], shape[1], factor_type, gauge)
    assert st == bu.OK and cond < 1e6
    hst, cov, hs0 = _harness_run(harness, sc, cam, ray, gauge)
    d = bu.scaled_diff(cov, ref)
    print(f"type {factor_type} {shape} gauge {gauge}: scaled diff {d:.2e}, sigma0 rel {abs(hs0 / s0 - 1):.1e}, cond {cond:.1e}")
    assert hst == bu.OK
    assert d <= BOUND
    assert abs(hs0 / s0 - 1) <= 1e-9
    assert (cov == cov.transpose(0, 2, 1)).all()  # symmetric bit for bit
    r0 = bu.ROT0[factor_type]
    assert (cov[gauge, r0:r0 + 3, :] == 0).all() and (cov[gauge, :, r0:r0 + 3] == 0).all() and cov[gauge, 0, 0] > 0
    # a-priori scaling
    _, cov_p, _ = _harness_run(harness, sc, cam, ray, gauge, pixel_sigma=0.7)
    assert np.abs(cov_p - cov * (0.7 / hs0) ** 2).max() <= 1e-13 * np.abs(cov_p).max()


@pytest.mark.parametrize("factor_type", [0, 1, 2])
def test_regularised_ray_inverse_equals_the_pseudo_inverse_form(harness, factor_type):
    """W_r V_r^+ W_r^T from the header's P_r = (V_r + tr(V_r) / 2 x^ x^T)^-1 against numpy.linalg.pinv"""
    sc, cam, ray = bu.solved_scene(5, 6, 40, factor_type)
    nf = bu.NF[factor_type]
    worst = 0.0
    for r in range(0, sc.n_ray, 5):
        idx = np.flatnonzero(sc.obs_ray == r)
        ln = len(idx)
        cams = np.ascontiguousarray(cam[sc.obs_cam[idx]]); uv = np.ascontiguousarray(sc.obs_uv[idx], dtype=np.float32)
        x = np.ascontiguousarray(ray[r])
        V = np.zeros((3, 3)); E = np.zeros((ln * nf, 3)); EPE = np.zeros((ln * nf, ln * nf))
        assert harness.ba_cov_harness_ray(factor_type, ln, _p(cams), _p(uv), _p(x), C.c_double(sc.ray_weight[r]), _p(V), _p(E), _p(EPE)) == 0
        xh = x / np.linalg.norm(x)
        assert np.abs(V @ xh).max() <= 1e-9 * np.abs(V).max()      # the ray block is singular along the ray
        assert np.abs(E @ xh).max() <= 1e-9 * np.abs(E).max()
        ref = E @ np.linalg.pinv(V, rcond=1e-10) @ E.T
        sd = np.sqrt(np.abs(np.diag(ref))) + 1e-300
        worst = max(worst, np.abs((EPE - ref) / sd[:, None] / sd[None, :]).max())
    print(f"type {factor_type}: worst scaled difference {worst:.2e}")
    assert worst <= 1e-9


def test_status_rules_by_counting(harness):
    st = harness.ba_cov_harness_status
    # m = 2 n_obs against p = NF n_cam - 3 + 2 n_ray
    assert st(4, 6, 48, 217, 0, 0) == bu.OK
    assert st(4, 2, 10, 20, 0, 0) == bu.OK            # 40 > 8 - 3 + 20
    assert st(4, 2, 10, 12, 0, 0) == bu.DOF           # 24 <= 25
    assert st(6, 3, 5, 12, 0, 0) == bu.DOF            # 24 <= 25
    assert st(6, 3, 5, 13, 0, 0) == bu.OK             # 26 > 25
    assert st(5, 2, 10, 13, 0, 0) == bu.DOF           # 26 <= 27
    assert st(5, 2, 10, 14, 0, 0) == bu.OK
    for fail, flags in ((1, 0), (0, 1), (0, 2), (0, 4), (0, 8)):  # Cholesky, diagonal, non-finite, penalty branch, ray block
        assert st(4, 6, 48, 217, fail, flags) == bu.SINGULAR
        assert st(4, 2, 10, 12, fail, flags) == bu.DOF  # too few constraints comes first
    assert [harness.ba_cov_harness_dim(t) for t in (0, 1, 2, 3, -1)] == [4, 5, 6, -1, -1]


def test_harness_leaves_outputs_untouched_unless_ok(harness):
    sc, cam, ray = bu.solved_scene(5, 6, 40, 0)
    bad = cam.copy(); bad[2, 4] = np.nan
    cov = np.full((sc.n_cam, 4, 4), 7.5)
    st, cov, s0 = _harness_run(harness, sc, bad, ray, 0, cov=cov, sigma0=-3.0)
    assert st == bu.SINGULAR and (cov == 7.5).all() and s0 == -3.0
    # PTZRayDist: a camera turned away puts its observations into the penalty branch, which has no linearisation
    sc1, cam1, ray1 = bu.solved_scene(5, 6, 40, 1)
    away = cam1.copy(); away[1, 4:7] = bu._orc().rodrigues_inv(np.diag([-1.0, 1.0, -1.0]) @ bu._orc().rodrigues(cam1[1, 4:7]))
    cov = np.full((sc1.n_cam, 5, 5), 7.5)
    st, cov, s0 = _harness_run(harness, sc1, away, ray1, 0, cov=cov, sigma0=-3.0)
    assert st == bu.SINGULAR and (cov == 7.5).all() and s0 == -3.0


def test_abi_checks_come_before_the_device(pkg):
    lib = pkg.api.lib()
    for name in ("ptz_ba_cov_dim", "ptz_ba_batch_covariance", "ptz_ba_covariance"):
        assert name in pkg.api.EXPORTS
        getattr(lib, name)
    assert [pkg.api.ba_cov_dim(t) for t in range(3)] == [4, 5, 6]
    lib.ptz_ba_cov_dim.restype = C.c_int32
    assert lib.ptz_ba_cov_dim(3) == EUNSUPPORTED and lib.ptz_ba_cov_dim(-1) == EUNSUPPORTED and lib.ptz_ba_cov_dim(9) == EUNSUPPORTED
    cov = np.zeros(64); s0 = np.zeros(1); st = np.zeros(1, np.int32)
    # no batch
    assert lib.ptz_ba_batch_covariance(None, None, C.c_double(0.0), _p(cov), _p(s0), _p(st), None) == EINVAL
    sc = pkg.synth.make_scene(0, 6, 40)

    def one_shot(scene, gauge=0, pixel_sigma=0.0, null=()):
        keep = []
        p = pkg.api._pack_problem(scene, keep)
        nf = 6
        a = dict(cam=np.ascontiguousarray(scene.cam_init), ray=np.ascontiguousarray(scene.ray_init), cov=np.zeros(scene.n_cam * nf * nf),
                 s0=np.zeros(1), st=np.zeros(1, np.int32))
        for k in null:
            a[k] = None
        return lib.ptz_ba_covariance(C.byref(p), _p(a["cam"]), _p(a["ray"]), int(gauge), C.c_double(pixel_sigma), None, _p(a["cov"]), _p(a["s0"]),
                                     _p(a["st"]))

    for s in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert one_shot(sc, pixel_sigma=s) == EINVAL
    for g in (-1, sc.n_cam, sc.n_cam + 7):
        assert one_shot(sc, gauge=g) == EINVAL
    for k in ("cam", "ray", "cov", "s0", "st"):
        assert one_shot(sc, null=(k,)) == EINVAL, k
    assert lib.ptz_ba_covariance(None, _p(cov), _p(cov), 0, C.c_double(0.0), None, _p(cov), _p(s0), _p(st)) == EINVAL
    # the follow-ups: PTZRayDistDisp, 2D-3D annotations, shared intrinsics
    import copy
    disp = copy.copy(sc); disp.factor_type = 3
    assert one_shot(disp) == EUNSUPPORTED
    ann = copy.copy(sc)
    ann.obs3d = dict(uv=np.array([[900.0, 500.0], [1000.0, 600.0]], np.float32), xyz=np.array([[1.0, 2.0, 0.0], [3.0, 4.0, 0.0]]),
                     cam=np.array([0, 1], np.int32))
    assert one_shot(ann) == EUNSUPPORTED
    shared = pkg.synth.make_scene(0, 6, 40, n_intrinsics_groups=2)
    assert one_shot(shared) == EUNSUPPORTED


def test_restated_covariance_predicts_the_scatter_of_noisy_solves(orc):
    """N = 400 noisy copies of one 6-view x 40-obs geometry (0.5 px, fixed seed, float32 pixels), solved by the oracle; the
    restatement at each solution.  Every ratio observed / predicted lies in 1 +- 4 / sqrt(2 N) = [0.86, 1.14]."""
    base, copies = bu.noisy_copies()
    N = len(copies)
    cams, covs, s0s = [], [], []
    for s in copies:
        cam, ray, _, summ, _ = orc.ba_solve(s, jacobian_mode=orc.JAC_ANALYTIC)
        assert summ["termination_type"] == 0
        st, cov, s0, _ = bu.restate(s, cam, ray, 0, check=False)
        assert st == bu.OK
        cams.append(cam); covs.append(cov); s0s.append(s0)
    ratios = bu.stat_ratios(cams, covs, s0s, anchor=0)
    lo, hi = 1 - 4 / np.sqrt(2 * N), 1 + 4 / np.sqrt(2 * N)
    print({k: round(v, 3) for k, v in ratios.items()})
    assert len(ratios) == 6 + 5 * 3 + 1
    for k, v in ratios.items():
        assert lo <= v <= hi, (k, v, lo, hi)
