"""GPU tests of the per-query covariance of relocalized cameras (k_krt_cov, ptz_krt_covariance_batch[_device],
KRTOptimizer::Covariance, run_ptz_reloc --uncertainty).  The numbers are held to the independent restatement of
krt_cov_util.py (oracle functors, central differences, numpy.linalg.inv): |C_ij - C_ij^ref| <= 1e-6 sqrt(C_ii^ref C_jj^ref),
sigma0 to 1e-9 relative -- the bound the project already uses between closed-form Jacobians and the numeric-differentiation
oracle."""
import ctypes as C
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import host_util as hu
import krt_cov_util as ku

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -12345.0


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("with_points", [False, True])
@pytest.mark.parametrize("ft", [0, 1, 2, 3])
def test_parity_with_the_restatement(pkg, ft, with_points):
    """The query set of krt_cov_util.query_set (match counts 0 .. 300 around the 16-lane stride, 0 / 1 / 5 points, masks, rejected
    queries, skipped border pixels, a rank-2 query, m <= NF) through the C-ABI: statuses equal the restatement's, covariances and
    sigma0 within the bound, outputs of every query that is not computed left as they were."""
    qs = ku.query_set(ft)
    nf = ku.NF[ft]
    st_ref, cov_ref, s0_ref, nskip = ku.reference(ft, with_points)
    assert np.array_equal(st_ref, ku.expected_status_by_counting(qs, with_points, nskip))
    assert {int(s) for s in st_ref} == {ku.OK, ku.DOF, ku.SINGULAR, ku.SKIPPED}
    batch = qs if with_points else ku.without_points(qs)
    cov, s0, st, ms = pkg.api.krt_covariance_batch(batch, qs.cam_cur, match_mask=qs.mask, accepted=qs.accepted,
                                                   cov=np.full((qs.n_query, nf, nf), SENT), sigma0=np.full(qs.n_query, SENT))
    assert np.array_equal(st, st_ref), [(q, qs.names[q], qs.counts[q], int(st[q]), int(st_ref[q])) for q in np.flatnonzero(st != st_ref)]
    worst = 0.0
    for q in range(qs.n_query):
        if st[q] != ku.OK:
            assert (cov[q] == SENT).all() and s0[q] == SENT, (q, qs.names[q])
            continue
        assert np.array_equal(cov[q], cov[q].T)
        d = np.sqrt(np.diag(cov_ref[q]))
        worst = max(worst, float((np.abs(cov[q] - cov_ref[q]) / np.outer(d, d)).max()))
        ku.assert_cov_close(cov[q], s0[q], cov_ref[q], s0_ref[q], (q, qs.names[q], qs.counts[q]))
    print("factor type %d, points %d: worst scaled covariance error %.2e, device %.3f ms" % (ft, with_points, worst, ms))
    # a-priori scale: pixel_sigma^2 N^-1 = the a-posteriori covariance times (pixel_sigma / sigma0)^2, same sigma0
    cov2, s02, st2, _ = pkg.api.krt_covariance_batch(batch, qs.cam_cur, match_mask=qs.mask, accepted=qs.accepted, pixel_sigma=0.25)
    ok = st == ku.OK
    assert np.array_equal(st2, st) and np.array_equal(s02[ok], s0[ok])
    np.testing.assert_allclose(cov2[ok], cov[ok] * ((0.25 / s0[ok]) ** 2)[:, None, None], rtol=1e-13)


@pytest.mark.parametrize("with_points", [0, 1])
def test_device_form_equals_host_form_bit_for_bit(with_points):
    """ptz_krt_covariance_batch_device behind ptz_krt_solve_batch_device on one torch stream (device tensors, no host round trip)
    gives the bits of solve-then-covariance through the host forms; a fresh process with torch initialised first, as
    test_krt_device_resident_entry_matches_host_entry does."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "run_krt_cov_device_entry.py"), str(with_points)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "covariance device entry ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_bits_do_not_depend_on_the_launch(pkg):
    """One reduction order: a query's covariance has the same bits alone, among 45 and among 20 000 queries (45: a query's place
    in its wave and workgroup changes from copy to copy)."""
    qs = ku.query_set(1)
    unit = 45
    small = ku.tiled(qs, unit, unit)
    c45, s45, t45, _ = pkg.api.krt_covariance_batch(small, small.cam_cur, match_mask=small.mask, accepted=small.accepted)
    assert (t45 == ku.OK).sum() > 30
    big = ku.tiled(qs, 20000, unit)
    cb, sb, tb, _ = pkg.api.krt_covariance_batch(big, big.cam_cur, match_mask=big.mask, accepted=big.accepted)
    idx = np.arange(20000) % unit
    assert np.array_equal(tb, t45[idx])
    assert np.array_equal(cb.view(np.uint64), c45[idx].view(np.uint64)) and np.array_equal(sb.view(np.uint64), s45[idx].view(np.uint64))
    for q in (0, 5, 44):
        one = types.SimpleNamespace(n_query=1, factor_type=1, match_ptr=qs.match_ptr[q:q + 2] - qs.match_ptr[q],
                                    uv_ref=qs.uv_ref[qs.match_ptr[q]:qs.match_ptr[q + 1]], uv_cur=qs.uv_cur[qs.match_ptr[q]:qs.match_ptr[q + 1]],
                                    cam_ref=qs.cam_ref[q:q + 1])
        c1, s1, t1, _ = pkg.api.krt_covariance_batch(one, qs.cam_cur[q:q + 1], match_mask=qs.mask[qs.match_ptr[q]:qs.match_ptr[q + 1]],
                                                     accepted=qs.accepted[q:q + 1])
        assert t1[0] == t45[q]
        assert np.array_equal(c1[0].view(np.uint64), c45[q].view(np.uint64)) and np.array_equal(s1.view(np.uint64), s45[q:q + 1].view(np.uint64))


def test_predicted_sigma_matches_the_scatter_of_the_solves(pkg):
    """400 noisy copies of one geometry (0.5 px on uv_cur, fixed seed; the CPU suite holds the reference path to the same interval
    for these seeds): the standard deviation of the 400 refined fx over the mean predicted sigma_f, and the mean sigma0 over 0.5,
    lie in 1 +- 4 / sqrt(2 * 400) = [0.86, 1.14]."""
    rb = ku.calibration_batch()
    cam, summ, acc, _ = pkg.api.krt_solve_batch(rb)
    assert acc.all()
    cov, s0, st, _ = pkg.api.krt_covariance_batch(rb, cam, accepted=acc)
    assert (st == ku.OK).all()
    ratio_f = cam[:, 0].std(ddof=1) / np.sqrt(cov[:, 0, 0]).mean()
    ratio_0 = s0.mean() / ku.CAL_SIGMA
    print("std(fx) / mean(sigma_f) = %.4f, mean(sigma0) / 0.5 = %.4f, sigma_f = %.3f px" % (ratio_f, ratio_0, np.sqrt(cov[:, 0, 0]).mean()))
    assert ku.CAL_LO <= ratio_f <= ku.CAL_HI
    assert ku.CAL_LO <= ratio_0 <= ku.CAL_HI


def _wrong_matches(pkg, ft, n_query, n_match, seed_id):
    """one match in three replaced by a uniform pixel"""
    rb = pkg.synth.make_reloc_batch(n_query, n_match, seed_id=seed_id, factor_type=ft)
    rb.uv_cur = np.array(rb.uv_cur, dtype=np.float32)
    rng = np.random.default_rng(17)
    k = rng.random(len(rb.uv_cur)) < 1.0 / 3.0
    rb.uv_cur[k] = rng.uniform([0, 0], [1920, 1080], (int(k.sum()), 2))
    return rb


def test_gated_chain(pkg):
    """ptz_krt_solve_batch_gated's inlier_mask goes into the covariance call as it is: the result is the covariance of the same
    queries given their kept matches only; without the mask the wrong matches inflate sigma0 of every query."""
    rb = _wrong_matches(pkg, 0, 24, 128, 9)
    cam, summ, acc, ninl, mask, _, _ = pkg.api.krt_solve_batch_gated(rb)
    assert acc.all() and ninl.min() > 6 and 0 < mask.sum() < len(mask)
    cov_m, s0_m, st_m, _ = pkg.api.krt_covariance_batch(rb, cam, match_mask=mask, accepted=acc)
    keep = mask.astype(bool)
    ptr = np.concatenate([[0], np.cumsum(ninl)]).astype(np.int64)
    kept = types.SimpleNamespace(n_query=rb.n_query, factor_type=0, match_ptr=ptr, uv_ref=rb.uv_ref[keep], uv_cur=rb.uv_cur[keep], cam_ref=rb.cam_ref)
    cov_k, s0_k, st_k, _ = pkg.api.krt_covariance_batch(kept, cam)
    assert (st_m == ku.OK).all() and (st_k == ku.OK).all()
    for q in range(rb.n_query):
        ku.assert_cov_close(cov_m[q], s0_m[q], cov_k[q], s0_k[q], q)
    cov_a, s0_a, st_a, _ = pkg.api.krt_covariance_batch(rb, cam)
    print("sigma0 over the kept matches %.2f .. %.2f px, over all matches %.1f .. %.1f px" % (s0_m.min(), s0_m.max(), s0_a.min(), s0_a.max()))
    assert (st_a == ku.OK).all() and (s0_a > s0_m).all()


def test_class_covariance_equals_the_batch_call(pkg):
    """KRTOptimizer::Covariance / StdDevs after Solve(): the numbers of ptz_krt_covariance_batch for the same query (FDist, with
    2D-3D constraints); before Solve() the class has none."""
    rb = pkg.synth.add_reloc_points(pkg.synth.make_reloc_batch(3, 96, seed_id=13, factor_type=1), n_pt=7)
    cam, _, acc, _ = pkg.api.krt_solve_batch(rb, max_num_iterations=200)
    cov, s0, st, _ = pkg.api.krt_covariance_batch(rb, cam, accepted=acc)
    q = 1
    assert acc[q] and st[q] == ku.OK
    a, b, pa, pb = int(rb.match_ptr[q]), int(rb.match_ptr[q + 1]), int(rb.point_ptr[q]), int(rb.point_ptr[q + 1])
    out = np.zeros(36); sig = np.zeros(5); before = C.c_int32(7)
    cur = np.ascontiguousarray(rb.cam_init[q]).copy()
    code = hu.lib().ptzh_krt_solve_cov(_p(np.ascontiguousarray(rb.cam_ref[q])), _p(cur), b - a, _p(np.ascontiguousarray(rb.uv_ref[a:b], np.float32)),
                                       _p(np.ascontiguousarray(rb.uv_cur[a:b], np.float32)), pb - pa,
                                       _p(np.ascontiguousarray(rb.pts2d[pa:pb], np.float32)), _p(np.ascontiguousarray(rb.pts3d[pa:pb])), 200,
                                       C.c_double(100.0), 1, _p(out), _p(sig), C.byref(before))
    assert code == 7 and before.value == 0
    # the class hands the camera on as K, R, t (rotation vector -> matrix -> vector): the same camera to round-off
    np.testing.assert_allclose(out[:25].reshape(5, 5), cov[q], rtol=1e-7, atol=0)
    np.testing.assert_allclose(sig, [np.sqrt(cov[q, 0, 0]), np.sqrt(cov[q, 1, 1]), np.sqrt(cov[q, 2, 2]), np.sqrt(cov[q, 3, 3]), s0[q]], rtol=1e-7)


def _run_tool(name, *args):
    exe = os.path.join(ROOT, "ptz-calib_amd", "bin", name)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize("ftype,gated", [(0, False), (1, False), (0, True)])
def test_run_ptz_reloc_uncertainty(pkg, tmp_path, ftype, gated):
    """run_ptz_reloc --uncertainty on the tiny written set of the tool tests: every registered image carries finite, positive
    sigma_f, sigma_rot_deg and sigma0, equal to api.krt_covariance_batch on the same inputs (the files round key points to %.9g
    and pass cameras through K, R, t: 1e-6); the same command without the flag writes none of the keys."""
    if gated:
        rb = _wrong_matches(pkg, ftype, 12, 96, 6)
    else:
        rb = pkg.synth.make_reloc_batch(12, 96, seed_id=6, factor_type=ftype)
        rb.uv_cur[rb.match_ptr[3]:rb.match_ptr[4]] = rb.uv_cur[rb.match_ptr[3]:rb.match_ptr[4]][::-1]  # query 3 fails
    paths = pkg.dataset_io.write_reloc_set(str(tmp_path), rb)
    args = ["--ref_images", paths["ref_images"], "--ref_features", paths["ref_features"], "--ref_params", paths["ref_params"],
            "--test_images", paths["test_images"], "--test_features", paths["test_features"]]
    args += (["--dist"] if ftype else []) + (["--inlier_matches"] if gated else [])
    out0, out1 = str(tmp_path / "out_plain"), str(tmp_path / "out_sigma")
    r0 = _run_tool("run_ptz_reloc", *args, "--output", out0)
    r1 = _run_tool("run_ptz_reloc", *args, "--output", out1, "--uncertainty")
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    plain = json.load(open(os.path.join(out0, "tests.json")))["cameras"]
    res = json.load(open(os.path.join(out1, "tests.json")))["cameras"]
    if gated:
        cam, _, acc, ninl, mask, _, _ = pkg.api.krt_solve_batch_gated(rb, min_inliers=6, max_num_iterations=200)
        acc = acc * (ninl > 0)
        cov, s0, st, _ = pkg.api.krt_covariance_batch(rb, cam, match_mask=mask, accepted=acc)
    else:
        cam, _, acc, _ = pkg.api.krt_solve_batch(rb, max_num_iterations=200)
        cov, s0, st, _ = pkg.api.krt_covariance_batch(rb, cam, accepted=acc)
    want = [os.path.splitext(paths["test_names"][q])[0] for q in range(rb.n_query) if acc[q]]
    assert list(res.keys()) == want == list(plain.keys()) and len(want) >= rb.n_query - 1
    for q in range(rb.n_query):
        name = os.path.splitext(paths["test_names"][q])[0]
        if not acc[q]:
            continue
        c = res[name]
        assert st[q] == ku.OK
        sig = [c["sigma_f"]] + list(c["sigma_rot_deg"]) + [c["sigma0"]]
        assert len(c["sigma_rot_deg"]) == 3 and all(np.isfinite(x) and x > 0 for x in sig)
        want_sig = [np.sqrt(cov[q, 0, 0])] + [np.degrees(np.sqrt(cov[q, k, k])) for k in (1, 2, 3)] + [s0[q]]
        np.testing.assert_allclose(sig, want_sig, rtol=1e-6)
        assert not any(k in plain[name] for k in ("sigma_f", "sigma_rot_deg", "sigma0"))
        assert {k: v for k, v in c.items() if k not in ("sigma_f", "sigma_rot_deg", "sigma0")} == plain[name]
