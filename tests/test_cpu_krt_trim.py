"""CPU tests of the trimmed relocalization's host side: the rule of ptz-calib_amd/csrc/ptz_krt_trim.h -- the header the kernels of
ptz_krt_resid.hip instantiate -- compiled for the host (tests/cpu_harness/krt_trim_harness.cc) against a numpy restatement on oracle
residuals; the rule itself: the loop solve / measure / judge / re-solve written on the CPU oracle recovers the contaminated batches
(krt_trim_util.py); and the argument checks of the new entry points, which come before any device work."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import krt_trim_util as tu

_p = tu._p
EINVAL, EUNSUPPORTED = -1, -4


# ---- the rule header against the numpy restatement -------------------------------------------------------------------------------------
def _oracle_query_errors(ft, q, frac=0.3, mode="displaced"):
    """err_px of query q of a contaminated batch at its ground-truth camera, through the oracle's functors"""
    b, _ = tu.contaminated_batch(ft, frac, mode)
    lo, hi = int(b.match_ptr[q]), int(b.match_ptr[q + 1])
    return tu.oracle_errors(ft, b.cam_ref[q], b.cam_gt[q], b.uv_ref[lo:hi], b.uv_cur[lo:hi])


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    assert (a[1] == b[1]).all()
    assert a[2] == b[2], (a[2], b[2])
    assert a[3] == b[3] or (np.isnan(a[3]) and np.isnan(b[3])), (a[3], b[3])


@pytest.mark.parametrize("ft", [0, 1])
def test_rule_header_equals_the_restatement_on_oracle_residuals(ft):
    rng = np.random.default_rng(5 + ft)
    seen = set()
    for q in range(6):
        full = _oracle_query_errors(ft, q)
        for n in (0, 1, 2, 7, 8, 9, 64, 65, 127, 128):  # even and odd counts on both sides of min_keep
            err = full[:n].copy()
            if n > 4:
                err[rng.integers(0, n, 2)] = -1.0  # two matches the border guard skips
            for in_u, in_k in ((None, np.ones(n, bool)), (rng.random(n) < 0.8, None)):
                if in_k is None:
                    in_k = in_u & (rng.random(n) < 0.7)
                for k_sigma in (3.0, 0.0):
                    for rounds_run in (1, 8):
                        a = tu.round_header(err, in_u, in_k, rounds_run, k_sigma=k_sigma)
                        _same(a, tu.round_restated(err, in_u, in_k, rounds_run, k_sigma=k_sigma))
                        seen.add(a[0])
    assert seen == {tu.CONTINUE, tu.DONE, tu.MAX_ROUNDS, tu.MIN_KEEP}, seen  # every way a round can end was exercised


def test_lower_median_at_even_and_odd_counts():
    for n in (1, 2, 3, 4, 9, 10):
        err = np.arange(n, 0, -1, dtype=np.float64)  # n .. 1
        d, new_k, t, med = tu.round_header(err, None, np.ones(n, bool), 1, trim_px=1000.0)
        assert med == np.sort(err)[(n - 1) // 2] == (n + 1) // 2
    # a kept set that counts nothing: no median, the floor is the threshold
    d, new_k, t, med = tu.round_header(np.array([-1.0, -1.0]), None, np.ones(2, bool), 1)
    assert np.isnan(med) and t == 4.0 and d == tu.DONE and new_k.all()


def test_ties_at_the_threshold_are_kept():
    err = np.array([4.0, np.nextafter(4.0, 5.0), 3.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    d, new_k, t, med = tu.round_header(err, None, np.ones(10, bool), 1, k_sigma=0.0)
    assert t == 4.0
    assert new_k.tolist() == [True, False] + [True] * 8 and d == tu.CONTINUE
    # with the median's threshold: t = 3 * 2 / 1.1774 exactly as the header forms it, an error equal to it stays
    base = np.array([2.0] * 9)
    t_exp = 3.0 * 2.0 / tu.RAYLEIGH_MEDIAN
    err = np.concatenate([base, [t_exp, np.nextafter(t_exp, 10.0)]])
    d, new_k, t, med = tu.round_header(err, None, np.ones(11, bool), 1)
    assert med == 2.0 and t == t_exp and new_k.tolist() == [True] * 10 + [False]


def test_skipped_never_rejected_masked_never_admitted_and_readmission():
    err = np.array([-1.0, 50.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.1, 0.2])
    in_u = np.ones(12, bool); in_u[10] = False  # a masked match with a tiny error
    in_k = in_u.copy(); in_k[11] = False        # a match of the universe an earlier round dropped
    for rule in (tu.round_header, tu.round_restated):
        d, new_k, t, med = rule(err, in_u, in_k, 1)
        assert new_k[0] and not new_k[1] and not new_k[10] and new_k[11] and d == tu.CONTINUE
        assert med == 0.5 and t == 4.0  # over the counted matches of K: the skipped and the dropped one are not in it


def test_min_keep_stops_and_keeps_the_set():
    err = np.concatenate([np.full(7, 1.0), np.full(9, 90.0)])
    for rule in (tu.round_header, tu.round_restated):
        d, new_k, t, med = rule(err, None, np.ones(16, bool), 1, k_sigma=0.0)
        assert d == tu.MIN_KEEP and int(new_k.sum()) == 7
        d, _, _, _ = rule(err, None, np.ones(16, bool), 1, k_sigma=0.0, min_keep=7)
        assert d == tu.CONTINUE


def test_rule_header_under_sanitizers(tmp_path):
    """the header's host instantiation as a stand-alone program built with the address and undefined-behaviour sanitizers"""
    exe = str(tmp_path / "krt_trim_harness_main")
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DKRT_TRIM_HARNESS_MAIN", "-o", exe, tu.HARNESS_SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout


# ---- the rule itself, on the CPU oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tu.CASES, ids=lambda c: "type%d-%d%%-%s" % (c[0], round(100 * c[1]), c[2]))
def test_oracle_loop_recovers_the_contaminated_batch(case):
    ft = case[0]
    b, wrong = tu.contaminated_batch(*case)
    r = tu.oracle_loop(*case)
    kept = r["kept"] != 0
    assert r["accepted"].all()
    assert not (kept & wrong).any()  # every contaminated match is removed
    assert int((~kept & ~wrong).sum()) <= 0.01 * int((~wrong).sum())
    assert all(x["flags"] == 0 and 1 <= x["rounds"] <= 8 for x in r["reports"])  # finished inside max_rounds, nobody flagged
    assert sum(x["n_removed"] for x in r["reports"]) == int((~kept).sum())
    # the focal lengths are as good as the clean batch's (plain oracle solve, no trimming)
    clean = tu.clean_as_batch(ft)
    cam_clean, _, acc_clean = tu.orc().krt_solve_batch(clean)
    assert acc_clean.all()
    med_clean = np.median(np.abs(cam_clean[:, 0] - clean.cam_gt[:, 0]))
    med = np.median(np.abs(r["cam"][:, 0] - b.cam_gt[:, 0]))
    assert med <= 1.5 * med_clean, (med, med_clean)
    # and the plain solve of the contaminated batch is NOT: the loop does the work
    cam_plain, _, _ = tu.orc().krt_solve_batch(b)
    assert np.median(np.abs(cam_plain[:, 0] - b.cam_gt[:, 0])) > 3 * med_clean


# ---- argument checks of the new entry points ------------------------------------------------------------------------------------------
def _resid_call(b, cam, **over):
    """ptz_krt_residuals_batch through ctypes with poisoned outputs: (rc, outputs)"""
    api = tu.pkg().api
    n, nm = b.n_query, int(b.match_ptr[-1])
    a = dict(n=n, ptr=np.ascontiguousarray(b.match_ptr, dtype=np.int64), uvr=np.ascontiguousarray(b.uv_ref, dtype=np.float32),
             uvc=np.ascontiguousarray(b.uv_cur, dtype=np.float32), pptr=None, p2=None, p3=None, cref=np.ascontiguousarray(b.cam_ref),
             ccur=np.ascontiguousarray(cam), ft=b.factor_type, mask=None, acc=None, lanes=0, dev=0,
             err=np.full(nm, -7.0), e3=None, rms=np.full(n, -7.0), mx=np.full(n, -7.0), med=np.full(n, -7.0), cnt=np.full(n, -7, np.int32),
             rms3=np.full(n, -7.0))
    a.update(over)
    ms = C.c_double(-7.0)
    rc = api.lib().ptz_krt_residuals_batch(a["n"], _p(a["ptr"]), _p(a["uvr"]), _p(a["uvc"]), _p(a["pptr"]), _p(a["p2"]), _p(a["p3"]), _p(a["cref"]),
                                           _p(a["ccur"]), a["ft"], _p(a["mask"]), _p(a["acc"]), a["lanes"], a["dev"], _p(a["err"]), _p(a["e3"]),
                                           _p(a["rms"]), _p(a["mx"]), _p(a["med"]), _p(a["cnt"]), _p(a["rms3"]), C.byref(ms))
    untouched = all((a[k] == -7).all() for k in ("err", "rms", "mx", "med", "cnt", "rms3") if a[k] is not None) and ms.value == -7.0
    return rc, untouched


def test_residuals_argument_checks_leave_the_outputs_untouched():
    b = tu.sub_batch(tu.clean_as_batch(0), [0, 1, 2])
    cam = b.cam_init
    bad_ptr0 = b.match_ptr.copy(); bad_ptr0[0] = 1
    bad_dec = b.match_ptr.copy(); bad_dec[1] = bad_dec[2] + 1
    pptr = np.array([0, 1, 2, 3], dtype=np.int64)
    cases = [dict(n=-1), dict(ptr=bad_ptr0), dict(ptr=bad_dec), dict(ptr=None), dict(uvr=None), dict(uvc=None), dict(cref=None), dict(ccur=None),
             dict(pptr=pptr), dict(pptr=pptr, p2=np.zeros((3, 2), np.float32)), dict(dev=-1),
             dict(err=None, rms=None, mx=None, med=None, cnt=None, rms3=None)]
    for over in cases:
        rc, untouched = _resid_call(b, cam, **over)
        assert rc == EINVAL and untouched, over.keys()
    for ft in (-1, 4):
        rc, untouched = _resid_call(b, cam, ft=ft)
        assert rc == EUNSUPPORTED and untouched
    rc, untouched = _resid_call(b, cam, n=0)
    assert rc == 0 and untouched


def _trimmed_call(b, **over):
    api = tu.pkg().api
    n, nm = b.n_query, int(b.match_ptr[-1])
    t = api.krt_trim_options()
    a = dict(n=n, ptr=np.ascontiguousarray(b.match_ptr, dtype=np.int64), uvr=np.ascontiguousarray(b.uv_ref, dtype=np.float32),
             uvc=np.ascontiguousarray(b.uv_cur, dtype=np.float32), pptr=None, p2=None, p3=None, cref=np.ascontiguousarray(b.cam_ref),
             ccur=np.full((n, 15), -7.0), ft=b.factor_type, mask=None, summ=(api.LmSummary * n)(), acc=np.full(n, -7, np.int32),
             kept=np.full(nm, 7, np.uint8), rep=(api.KrtTrimReport * n)(), trim={})
    a.update(over)
    for k, v in a["trim"].items():
        setattr(t, k, v)
    for r in a["rep"]:
        r.rounds = -7
    o = api.default_options(**a.get("opt", {}))
    ms = C.c_double(-7.0)
    rc = api.lib().ptz_krt_solve_batch_trimmed(a["n"], _p(a["ptr"]), _p(a["uvr"]), _p(a["uvc"]), _p(a["pptr"]), _p(a["p2"]), _p(a["p3"]),
                                               _p(a["cref"]), _p(a["ccur"]), a["ft"], C.c_double(100.0), _p(a["mask"]), C.byref(t), C.byref(o),
                                               a["summ"], _p(a["acc"]) if a["acc"] is not None else None, _p(a["kept"]), a["rep"], C.byref(ms))
    untouched = ((a["ccur"] is None or (a["ccur"] == -7).all()) and (a["acc"] is None or (a["acc"] == -7).all()) and (a["kept"] == 7).all()
                 and all(r.rounds == -7 for r in a["rep"]) and ms.value == -7.0)
    return rc, untouched


def test_trimmed_solve_argument_checks_leave_the_outputs_untouched():
    b = tu.sub_batch(tu.clean_as_batch(1), [0, 1, 2])
    bad_ptr0 = b.match_ptr.copy(); bad_ptr0[0] = 1
    bad_dec = b.match_ptr.copy(); bad_dec[2] = bad_dec[1] - 1
    pptr = np.array([0, 1, 2, 3], dtype=np.int64)
    cases = [dict(n=-1), dict(ptr=bad_ptr0), dict(ptr=bad_dec), dict(ptr=None), dict(uvr=None), dict(uvc=None), dict(cref=None), dict(ccur=None),
             dict(pptr=pptr), dict(summ=None), dict(acc=None), dict(opt=dict(device_id=-1)),
             dict(trim=dict(trim_px=0.0)), dict(trim=dict(trim_px=-1.0)), dict(trim=dict(trim_px=float("nan"))), dict(trim=dict(trim_px=float("inf"))),
             dict(trim=dict(k_sigma=-0.5)), dict(trim=dict(k_sigma=float("nan"))), dict(trim=dict(max_rounds=0)), dict(trim=dict(max_rounds=65)),
             dict(trim=dict(min_keep=-1))]
    for over in cases:
        rc, untouched = _trimmed_call(b, **over)
        assert rc == EINVAL and untouched, over
    for ft in (-1, 4):
        rc, untouched = _trimmed_call(b, ft=ft)
        assert rc == EUNSUPPORTED and untouched
    rc, untouched = _trimmed_call(b, n=0)
    assert rc == 0 and untouched
    api = tu.pkg().api
    t = api.krt_trim_options()
    assert (t.trim_px, t.k_sigma, t.max_rounds, t.min_keep) == (4.0, 3.0, 8, 8)
    assert api.krt_trim_workspace_bytes(3, 384) > 0 and api.krt_trim_workspace_bytes(-1, 0) == EINVAL
    assert C.sizeof(api.KrtTrimReport) == 48 and C.sizeof(api.KrtTrimOptions) == 24

