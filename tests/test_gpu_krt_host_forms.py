"""The four host-form relocalization entry points on ONE ragged batch with 2D-3D points: they stage their inputs through one shared
path (krt_batch_upload, ptz-calib_amd/csrc/ptz_krt.hip) -- the plain solve through the pinned mirror, the other three array by array --
and must agree with each other to the bit.  (Host form against _device form is run_krt*_device_entry.py's.)"""
import numpy as np
import pytest

import krt_trim_util as tu

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 15, 17, 40, 40)  # matches per query: none, one, either side of a row of sixteen lanes, two full ones
NO_POINTS = 2                    # the query whose point range is empty
S = -7.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _batch(pkg):
    rb = pkg.synth.add_reloc_points(pkg.synth.make_reloc_batch(6, 40, factor_type=1), n_pt=5)
    sel = np.concatenate([np.arange(40) < c for c in COUNTS])
    b = tu.sub_batch(rb, list(range(6)), sel)
    lo, hi = int(b.point_ptr[NO_POINTS]), int(b.point_ptr[NO_POINTS + 1])
    b.pts2d, b.pts3d = np.delete(b.pts2d, slice(lo, hi), axis=0), np.delete(b.pts3d, slice(lo, hi), axis=0)
    b.point_ptr = b.point_ptr.copy()
    b.point_ptr[NO_POINTS + 1:] -= hi - lo
    assert np.diff(b.match_ptr).tolist() == list(COUNTS) and np.diff(b.point_ptr).tolist() == [5, 5, 0, 5, 5, 5]
    return b


def _report_and_covariance(api, b, cam, acc):
    """ptz_krt_residuals_batch and ptz_krt_covariance_batch at `cam` into poisoned outputs, with the rules of `accepted` asserted:
    a query with accepted = 0 keeps every sentinel, an accepted one is computed.  Returns the report."""
    n, nm, npt = b.n_query, int(b.match_ptr[-1]), int(b.point_ptr[-1])
    out = dict(err_px=np.full(nm, S), err3d_px=np.full(npt, S), rms=np.full(n, S), max=np.full(n, S), median=np.full(n, S), rms3d=np.full(n, S),
               count=np.full(n, -7, np.int32))
    r = api.krt_residuals_batch(b, cam, accepted=acc, out=out)
    cov, s0, st, _ = api.krt_covariance_batch(b, cam, accepted=acc, cov=np.full((n, 5, 5), S), sigma0=np.full(n, S))
    for q in range(n):
        m = slice(int(b.match_ptr[q]), int(b.match_ptr[q + 1]))
        p = slice(int(b.point_ptr[q]), int(b.point_ptr[q + 1]))
        if acc[q]:
            # the count is the matches the border guard did not skip
            assert r["count"][q] == int((r["err_px"][m] != -1.0).sum())
            assert (r["err_px"][m] != S).all() and (r["err3d_px"][p] != S).all() and r["rms3d"][q] != S
            assert st[q] != api.COV_SKIPPED
            assert (cov[q] != S).all() == (st[q] == api.COV_OK) == (s0[q] != S)
        else:
            assert (r["err_px"][m] == S).all() and (r["err3d_px"][p] == S).all()
            assert all(r[k][q] == S for k in ("rms", "max", "median", "rms3d")) and r["count"][q] == -7
            assert st[q] == api.COV_SKIPPED and (cov[q] == S).all() and s0[q] == S
    return r, cov, s0, st


def test_host_forms_agree_on_one_ragged_batch_with_points(pkg):
    """On the commit before the shared path this test passed as it stands.  Its plain solve accepted all six queries -- also the one
    without a match and the one with a single match, on their five points -- so with the solve's own `accepted` nothing keeps a
    sentinel; the report and the covariance are therefore taken a second time with one query struck from `accepted`, which takes the
    other side of that rule in both."""
    api = pkg.api
    b = _batch(pkg)
    cam, summ, acc, _ = api.krt_solve_batch(b)
    print("accepted", acc.tolist(), "termination", [s["termination_type"] for s in summ])
    ok = acc != 0
    assert np.array_equal(_bits(cam[~ok]), _bits(b.cam_init[~ok]))  # a refused query's camera is the caller's
    # the trimmed solve that trims nothing: the plain solve's bits
    tc, ts, ta, tk, tr, _ = api.krt_solve_batch_trimmed(b, max_rounds=1, trim_px=1e9)
    assert np.array_equal(acc, ta) and np.array_equal(_bits(cam), _bits(tc)) and tk.all()
    assert [repr(s) for s in summ] == [repr(s) for s in ts]
    # the report and the covariance at the solved cameras, with the solve's accepted
    r, cov, s0, st = _report_and_covariance(api, b, cam, acc)
    for q in np.nonzero(ok)[0]:
        # the trimmed solve's own report of its only round is the residual report's rms, bit for bit
        assert _bits(tr[q]["rms_last"]) == _bits(r["rms"][q]) or (np.isnan(tr[q]["rms_last"]) and np.isnan(r["rms"][q]))
    # one query struck: its outputs keep the sentinels, every other query's bits are what they were
    struck = acc.copy()
    struck[4] = 0
    r2, cov2, s02, st2 = _report_and_covariance(api, b, cam, struck)
    keep = struck != 0
    for k in ("rms", "max", "median", "rms3d"):
        assert np.array_equal(_bits(r2[k][keep]), _bits(r[k][keep])), k
    assert np.array_equal(r2["count"][keep], r["count"][keep]) and np.array_equal(st2[keep], st[keep])
    assert np.array_equal(_bits(cov2[keep]), _bits(cov[keep])) and np.array_equal(_bits(s02[keep]), _bits(s0[keep]))
