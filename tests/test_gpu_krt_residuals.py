"""GPU tests of the residual report of relocalized cameras (k_krt_resid, ptz_krt_residuals_batch[_device]).  The errors are held to
the oracle's functors as krt_cov_util.Restatement takes them, within 1e-9 px -- the bound of the sibling bundle-adjustment test:
FP64 round-off on residuals of up to ~2e3 px is ~1e-12 px; the statistics to numpy on the device's own errors."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import krt_cov_util as cu
import krt_trim_util as tu

pytestmark = pytest.mark.gpu

SENT = -12345.0


@functools.lru_cache(maxsize=None)
def _oracle_report(ft):
    """(err [n_match], err3 [n_point]) of krt_cov_util.query_set(ft) through the oracle's functors; NaN for rejected queries"""
    qs = cu.query_set(ft)
    err, e3 = np.full(int(qs.match_ptr[-1]), np.nan), np.full(int(qs.point_ptr[-1]), np.nan)
    for q in range(qs.n_query):
        if qs.accepted[q] == 0:
            continue
        a, b, pa, pb = int(qs.match_ptr[q]), int(qs.match_ptr[q + 1]), int(qs.point_ptr[q]), int(qs.point_ptr[q + 1])
        err[a:b] = tu.oracle_errors(ft, qs.cam_ref[q], qs.cam_cur[q], qs.uv_ref[a:b], qs.uv_cur[a:b])
        e3[pa:pb] = tu.oracle_point_errors(ft, qs.cam_ref[q], qs.cam_cur[q], qs.pts2d[pa:pb], qs.pts3d[pa:pb])
    return err, e3


def _poison(qs, with_points):
    n, nm = qs.n_query, int(qs.match_ptr[-1])
    out = dict(err_px=np.full(nm, SENT), rms=np.full(n, SENT), max=np.full(n, SENT), median=np.full(n, SENT), rms3d=np.full(n, SENT),
               count=np.full(n, -77, dtype=np.int32))
    if with_points:
        out["err3d_px"] = np.full(int(qs.point_ptr[-1]), SENT)
    return out


@pytest.mark.parametrize("with_points", [False, True])
@pytest.mark.parametrize("ft", [0, 1, 2, 3])
def test_report_against_the_oracle(pkg, ft, with_points):
    qs = cu.query_set(ft)
    want_err, want_e3 = _oracle_report(ft)
    batch = qs if with_points else cu.without_points(qs)
    r = pkg.api.krt_residuals_batch(batch, qs.cam_cur, match_mask=qs.mask, accepted=qs.accepted, out=_poison(qs, with_points))
    worst = worst3 = 0.0
    n_skipped = n_rejected = n_empty = 0
    for q in range(qs.n_query):
        a, b, pa, pb = int(qs.match_ptr[q]), int(qs.match_ptr[q + 1]), int(qs.point_ptr[q]), int(qs.point_ptr[q + 1])
        e = r["err_px"][a:b]
        if qs.accepted[q] == 0:  # the camera is NaN: nothing read, nothing written
            n_rejected += 1
            assert (e == SENT).all() and r["count"][q] == -77
            assert all(r[k][q] == SENT for k in ("rms", "max", "median", "rms3d"))
            assert not with_points or (r["err3d_px"][pa:pb] == SENT).all()
            continue
        skip = want_err[a:b] < 0
        n_skipped += int(skip.sum())
        assert np.array_equal(e == -1.0, skip) and (e[~skip] >= 0).all(), (q, qs.names[q])  # -1.0 exactly where the restatement's guard skips
        if (~skip).any():
            worst = max(worst, float(np.abs(e[~skip] - want_err[a:b][~skip]).max()))
        c = e[(qs.mask[a:b] != 0) & ~skip]  # the statistics: over the counted matches, from the device's own errors
        assert r["count"][q] == len(c)
        if len(c) == 0:
            n_empty += 1
            assert np.isnan(r["rms"][q]) and np.isnan(r["max"][q]) and np.isnan(r["median"][q])
        else:
            assert abs(r["rms"][q] - np.sqrt(np.mean(c ** 2))) <= 1e-12 * np.sqrt(np.mean(c ** 2))
            assert r["max"][q] == c.max()
            assert r["median"][q] == np.sort(c)[(len(c) - 1) // 2]  # bit for bit: one of the errors
        if with_points and pb > pa:
            e3 = r["err3d_px"][pa:pb]
            worst3 = max(worst3, float(np.abs(e3 - want_e3[pa:pb]).max()))
            assert abs(r["rms3d"][q] - np.sqrt(np.mean(e3 ** 2))) <= 1e-12 * np.sqrt(np.mean(e3 ** 2))
        else:
            assert np.isnan(r["rms3d"][q])
    print("factor type %d, points %d: worst |err_px - oracle| %.3e px, points %.3e px, device %.3f ms" % (ft, with_points, worst, worst3, r["device_ms"]))
    assert worst <= 1e-9 and worst3 <= 1e-9
    assert n_rejected == 2 and n_empty >= 2 and (n_skipped >= 15 if ft & 1 else n_skipped == 0)


def _bits(r, qs, q):
    a, b = int(qs.match_ptr[q]), int(qs.match_ptr[q + 1])
    out = [r["err_px"][a:b].view(np.uint64).tolist(), int(r["count"][q])] + [np.float64(r[k][q]).view(np.uint64) for k in ("rms", "max", "median", "rms3d")]
    if r["err3d_px"] is not None:
        out.append(r["err3d_px"][int(qs.point_ptr[q]):int(qs.point_ptr[q + 1])].view(np.uint64).tolist())
    return out


@pytest.mark.parametrize("ft", [1, 2])
def test_bits_depend_on_the_query_alone(pkg, ft):
    """a query's report: the same bits with 64 and with 16 lanes per query, in two runs, and alone as inside the batch"""
    qs = cu.query_set(ft)
    runs = [pkg.api.krt_residuals_batch(qs, qs.cam_cur, match_mask=qs.mask, accepted=qs.accepted, lanes_per_query=g) for g in (64, 16, 64, 16)]
    for q in range(qs.n_query):
        if qs.accepted[q]:
            want = _bits(runs[0], qs, q)
            assert all(_bits(r, qs, q) == want for r in runs[1:]), (q, qs.names[q], qs.counts[q])
    for q in [q for q in range(qs.n_query) if qs.accepted[q]][::5]:
        a, b = int(qs.match_ptr[q]), int(qs.match_ptr[q + 1])
        one = tu.sub_batch(qs, [q], cam_init=qs.cam_cur)
        for g in (64, 16):
            r1 = pkg.api.krt_residuals_batch(one, qs.cam_cur[q:q + 1], match_mask=qs.mask[a:b], lanes_per_query=g)
            assert _bits(r1, one, 0) == _bits(runs[0], qs, q), (q, g)


def test_device_forms_equal_the_host_forms_bit_for_bit():
    """ptz_krt_residuals_batch_device behind ptz_krt_solve_batch_device, and ptz_krt_solve_batch_trimmed_device, on one torch stream
    (device tensors, no host round trip) give the bits of the host forms; a fresh process with torch initialised first"""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "run_krt_trim_device_entry.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "residual and trimmed device entries ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
