"""CPU tests of the per-query covariance of relocalized cameras (ptz_krt_covariance_batch): the C-ABI validates before it
looks for a device and has no CPU fallback, and the per-query algebra of ptz-calib_amd/csrc/ptz_krt_cov.h -- the header
k_krt_cov instantiates -- compiled for the host equals an independent restatement on the oracle's functors (krt_cov_util.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import krt_cov_util as ku

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK_, EINVAL, ENODEVICE, EUNSUPPORTED = 0, -1, -2, -4


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(ROOT, "tests", "cpu_harness", "libkrt_cov_harness.so")
    src = os.path.join(ROOT, "tests", "cpu_harness", "krt_cov_harness.cc")
    srcs = [src] + [os.path.join(ROOT, "ptz-calib_amd", "csrc", h) for h in ("ptz_krt_cov.h", "ptz_factor.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    return C.CDLL(so)


def _call(lib, qs, n=None, ptr=None, factor_type=None, pixel_sigma=0.0, cov=None, sigma0=None, status=None, null=(), points=True):
    """ptz_krt_covariance_batch on a query set, with single arguments replaced or nulled"""
    n = qs.n_query if n is None else n
    a = dict(match_ptr=qs.match_ptr if ptr is None else ptr, uv_ref=qs.uv_ref, uv_cur=qs.uv_cur,
             point_ptr=qs.point_ptr if points else None, pts2d=qs.pts2d if points else None, pts3d=qs.pts3d if points else None,
             cam_ref=qs.cam_ref, cam_cur=qs.cam_cur, mask=qs.mask, accepted=qs.accepted,
             cov=np.zeros(36 * qs.n_query) if cov is None else cov, sigma0=np.zeros(qs.n_query) if sigma0 is None else sigma0,
             status=np.zeros(qs.n_query, np.int32) if status is None else status)
    for k in null:
        a[k] = None
    ms = C.c_double()
    return lib.ptz_krt_covariance_batch(n, _p(a["match_ptr"]), _p(a["uv_ref"]), _p(a["uv_cur"]), _p(a["point_ptr"]), _p(a["pts2d"]),
                                        _p(a["pts3d"]), _p(a["cam_ref"]), _p(a["cam_cur"]), qs.factor_type if factor_type is None else factor_type,
                                        _p(a["mask"]), _p(a["accepted"]), C.c_double(pixel_sigma), 0, _p(a["cov"]), _p(a["sigma0"]),
                                        _p(a["status"]), C.byref(ms))


def test_abi_validates_before_the_device_and_has_no_cpu_fallback(pkg):
    lib = pkg.api.lib()
    for name in ("ptz_krt_free_dim", "ptz_krt_covariance_batch", "ptz_krt_covariance_batch_device"):
        assert name in pkg.api.EXPORTS
        getattr(lib, name)
    lib.ptz_krt_free_dim.restype = C.c_int32
    assert [lib.ptz_krt_free_dim(t) for t in range(4)] == [4, 5, 5, 6]
    assert lib.ptz_krt_free_dim(4) == EUNSUPPORTED and lib.ptz_krt_free_dim(-1) == EUNSUPPORTED
    assert [pkg.api.krt_free_dim(t) for t in range(4)] == [4, 5, 5, 6]
    assert (pkg.api.COV_OK, pkg.api.COV_DOF, pkg.api.COV_SINGULAR, pkg.api.COV_SKIPPED) == (0, 1, 2, 3)
    qs = ku.query_set(0)
    # malformed calls are PTZ_EINVAL whether or not a GPU exists
    assert _call(lib, qs, n=-1) == EINVAL
    bad = qs.match_ptr.copy(); bad[0] = 1
    assert _call(lib, qs, ptr=bad) == EINVAL
    bad = qs.match_ptr.copy(); bad[5] = bad[4] - 1
    assert _call(lib, qs, ptr=bad) == EINVAL
    for s in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert _call(lib, qs, pixel_sigma=s) == EINVAL
    for k in ("match_ptr", "uv_ref", "uv_cur", "cam_ref", "cam_cur", "cov", "sigma0", "status"):
        assert _call(lib, qs, null=(k,)) == EINVAL, k
    assert _call(lib, qs, null=("pts2d",)) == EINVAL and _call(lib, qs, null=("pts3d",)) == EINVAL
    for t in (-1, 4, 17):
        assert _call(lib, qs, factor_type=t) == EUNSUPPORTED
    # the device form checks the same before it looks for a device
    dv = lib.ptz_krt_covariance_batch_device
    one = C.c_void_p(256)  # never dereferenced: every call below is refused before any device work
    assert dv(-1, one, one, one, None, None, None, one, one, 0, None, None, C.c_double(0.0), one, one, one, None) == EINVAL
    assert dv(4, one, one, one, None, None, None, one, one, 0, None, None, C.c_double(-1.0), one, one, one, None) == EINVAL
    assert dv(4, one, one, one, one, None, None, one, one, 0, None, None, C.c_double(0.0), one, one, one, None) == EINVAL
    assert dv(4, one, one, one, None, None, None, one, one, 9, None, None, C.c_double(0.0), one, one, one, None) == EUNSUPPORTED
    assert dv(4, one, one, one, None, None, None, one, None, 0, None, None, C.c_double(0.0), one, one, one, None) == EINVAL
    assert dv(0, None, None, None, None, None, None, None, None, 0, None, None, C.c_double(0.0), None, None, None, None) == OK_
    # empty extents: no query needs no arrays
    assert _call(lib, qs, n=0) == OK_
    assert _call(lib, qs, n=0, null=("match_ptr", "uv_ref", "uv_cur", "cam_ref", "cam_cur", "cov", "sigma0", "status", "mask", "accepted",
                                     "point_ptr", "pts2d", "pts3d")) == OK_
    with pytest.raises(pkg.api.PtzError) as e:
        pkg.api.krt_covariance_batch(qs, qs.cam_cur, pixel_sigma=-1.0)
    assert e.value.code == EINVAL
    if pkg.api.device_count() == 0:
        # no GPU: the call fails loudly, never computes on the CPU
        cov = np.full(36 * qs.n_query, 7.0); s0 = np.full(qs.n_query, 7.0); st = np.full(qs.n_query, 7, np.int32)
        assert _call(lib, qs, cov=cov, sigma0=s0, status=st) == ENODEVICE
        assert (cov == 7).all() and (s0 == 7).all() and (st == 7).all()
        with pytest.raises(pkg.api.PtzError) as e:
            pkg.api.krt_covariance_batch(qs, qs.cam_cur)
        assert e.value.code == ENODEVICE


def _harness_query(h, qs, q, with_points, pixel_sigma=0.0):
    nf = ku.NF[qs.factor_type]
    a, b = int(qs.match_ptr[q]), int(qs.match_ptr[q + 1])
    pa, pb = (int(qs.point_ptr[q]), int(qs.point_ptr[q + 1])) if with_points else (0, 0)
    uvr, uvc, mk = (np.ascontiguousarray(x[a:b]) for x in (qs.uv_ref, qs.uv_cur, qs.mask))
    p2, p3 = np.ascontiguousarray(qs.pts2d[pa:pb]), np.ascontiguousarray(qs.pts3d[pa:pb])
    cov = np.full((nf, nf), -7.0); s0 = np.full(1, -7.0)
    st = h.h_krt_cov(qs.factor_type, b - a, _p(uvr), _p(uvc), _p(mk), pb - pa, _p(p2), _p(p3), _p(np.ascontiguousarray(qs.cam_ref[q])),
                     _p(np.ascontiguousarray(qs.cam_cur[q])), C.c_double(pixel_sigma), _p(cov), _p(s0))
    return st, cov, float(s0[0])


@pytest.mark.parametrize("with_points", [False, True])
@pytest.mark.parametrize("ft", [0, 1, 2, 3])
def test_header_algebra_equals_the_restatement(harness, ft, with_points):
    """accumulate + scaled inverse + status of ptz_krt_cov.h on the host, query by query, against central differences of the
    oracle's functors: status equal, |C_ij - C_ij^ref| <= 1e-6 sqrt(C_ii^ref C_jj^ref), sigma0 to 1e-9."""
    qs = ku.query_set(ft)
    st_ref, cov_ref, s0_ref, nskip = ku.reference(ft, with_points)
    # the restatement itself first: what counting the blocks says, OK for the whole regular set
    assert np.array_equal(st_ref, ku.expected_status_by_counting(qs, with_points, nskip))
    regular = [q for q in range(qs.n_query) if qs.names[q] == "grid" and qs.counts[q][0] >= 15]
    assert len(regular) == 27 and [int(st_ref[q]) for q in regular] == [ku.OK] * 27
    assert {int(s) for s in st_ref} == {ku.OK, ku.DOF, ku.SINGULAR, ku.SKIPPED}
    if ft & 1:
        border = [q for q in range(qs.n_query) if qs.names[q] == "border"]
        assert all(0 < nskip[q] < qs.counts[q][0] for q in border) and all(st_ref[q] == ku.OK for q in border)
    for q in range(qs.n_query):
        if qs.accepted[q] == 0:
            continue  # (decided by the kernel, not by the header)
        st, cov, s0 = _harness_query(harness, qs, q, with_points)
        assert st == st_ref[q], (q, qs.names[q], qs.counts[q])
        if st == ku.OK:
            assert np.array_equal(cov, cov.T)
            ku.assert_cov_close(cov, s0, cov_ref[q], s0_ref[q], (q, qs.names[q], qs.counts[q]))
        else:
            assert (cov == -7.0).all() and s0 == -7.0  # left untouched


def test_a_priori_scale_and_sigma0(harness):
    """pixel_sigma > 0: C = pixel_sigma^2 N^-1, i.e. the a-posteriori covariance times (pixel_sigma / sigma0)^2; sigma0 the same."""
    qs = ku.query_set(1)
    q = next(i for i in range(qs.n_query) if qs.counts[i] == (129, 5) and qs.names[i] == "grid")
    st0, c0, s0 = _harness_query(harness, qs, q, True)
    st1, c1, s1 = _harness_query(harness, qs, q, True, pixel_sigma=0.25)
    assert st0 == st1 == ku.OK and s0 == s1
    np.testing.assert_allclose(c1, c0 * (0.25 / s0) ** 2, rtol=1e-14)
    r = ku.Restatement()
    a, b = int(qs.match_ptr[q]), int(qs.match_ptr[q + 1]); pa, pb = int(qs.point_ptr[q]), int(qs.point_ptr[q + 1])
    st, cr, sr, _ = r.query(1, qs.cam_ref[q], qs.cam_cur[q], qs.uv_ref[a:b], qs.uv_cur[a:b], qs.mask[a:b], qs.pts2d[pa:pb], qs.pts3d[pa:pb], 0.25)
    assert st == ku.OK
    ku.assert_cov_close(c1, s1, cr, sr)


def test_reference_path_is_calibrated_for_the_chosen_seeds(orc):
    """The statistical test of test_gpu_krt_covariance.py on the CPU alone: orc_krt_solve_batch refines the 400 noisy copies of one
    geometry, the restatement predicts sigma_f and sigma0 (every tenth query: the geometry is one, the predictions differ in the
    fourth digit).  std(fx) / mean(sigma_f) and mean(sigma0) / 0.5 lie in 1 +- 4 / sqrt(800): the seeds are fit for the GPU test."""
    rb = ku.calibration_batch()
    cam, summ, acc = orc.krt_solve_batch(rb, num_threads=orc.usable_cores())
    assert acc.all()
    rs = ku.Restatement()
    sf, s0 = [], []
    for q in range(0, ku.CAL_N, 10):
        st, cov, sig0, _ = rs.query(0, rb.cam_ref[q], cam[q], rb.uv_ref[128 * q:128 * q + 128], rb.uv_cur[128 * q:128 * q + 128])
        assert st == ku.OK
        sf.append(np.sqrt(cov[0, 0])); s0.append(sig0)
    ratio_f = cam[:, 0].std(ddof=1) / np.mean(sf)
    ratio_0 = np.mean(s0) / ku.CAL_SIGMA
    print("reference path: std(fx) / mean(sigma_f) = %.4f, mean(sigma0) / 0.5 = %.4f, sigma_f = %.3f px" % (ratio_f, ratio_0, np.mean(sf)))
    assert ku.CAL_LO <= ratio_f <= ku.CAL_HI and ku.CAL_LO <= ratio_0 <= ku.CAL_HI


def test_class_reports_no_covariance_before_a_solve():
    """KRTOptimizer::Covariance is valid after a Solve() that returned true: before it the answer is false (no device is asked)."""
    import host_util as hu
    qs = ku.query_set(0)
    q = next(i for i in range(qs.n_query) if qs.counts[i] == (64, 0) and qs.names[i] == "grid")
    a, b = int(qs.match_ptr[q]), int(qs.match_ptr[q + 1])
    cov = np.zeros(36); sig = np.zeros(5); before = C.c_int32(7)
    cur = np.ascontiguousarray(qs.cam_cur[q]).copy()
    hu.lib().ptzh_krt_solve_cov(_p(np.ascontiguousarray(qs.cam_ref[q])), _p(cur), b - a, _p(np.ascontiguousarray(qs.uv_ref[a:b])),
                                _p(np.ascontiguousarray(qs.uv_cur[a:b])), 0, None, None, 200, C.c_double(100.0), 0, _p(cov), _p(sig),
                                C.byref(before))
    assert before.value == 0
