"""CPU tests of the trimmed bundle adjustment's host side: the re-packing (ptz_ba_problem_trim) against a numpy restatement, the
selection rule of ptz-calib_amd/csrc/ptz_ba_trim.h -- the header the kernel of ptz_ba_resid.hip instantiates -- compiled for the
host (tests/cpu_harness/ba_trim_harness.cc) against a numpy restatement on oracle residuals, and the rule itself: the loop
solve / measure / select / re-pack written on the CPU oracle recovers the contaminated rigs (ba_trim_util.py)."""
import ctypes as C

import numpy as np
import pytest

import ba_trim_util as tu

_p = tu._p


def _trim_raw(sc, reject, **override):
    """ptz_ba_problem_trim through ctypes with poisoned outputs: (rc, outputs dict)"""
    api = tu.pkg().api
    keep = []
    p = api._pack_problem(sc, keep)
    for k, v in override.items():
        setattr(p, k, v)
    n_obs, n_ray = len(sc.obs_cam), sc.n_ray
    out = dict(uv=np.full((n_obs, 2), -7.0, dtype=np.float32), cam=np.full(n_obs, -7, dtype=np.int32), ray=np.full(n_obs, -7, dtype=np.int32),
               w=np.full(n_ray, -7.0), ray_map=np.full(n_ray, -7, dtype=np.int32))
    nr, no = C.c_int32(-7), C.c_int64(-7)
    rej = None if reject is None else np.ascontiguousarray(reject, dtype=np.uint8)
    rc = api.lib().ptz_ba_problem_trim(C.byref(p), _p(rej), _p(out["uv"]), _p(out["cam"]), _p(out["ray"]), _p(out["w"]), _p(out["ray_map"]),
                                       C.byref(nr), C.byref(no))
    out["n_ray"], out["n_obs"] = nr.value, no.value
    return rc, out


def _untouched(out):
    return ((out["uv"] == -7).all() and (out["cam"] == -7).all() and (out["ray"] == -7).all() and (out["w"] == -7).all()
            and (out["ray_map"] == -7).all() and out["n_ray"] == -7 and out["n_obs"] == -7)


@pytest.mark.parametrize("case", tu.CONTAMINATED, ids=lambda c: "scene%d-type%d" % (c[0], c[3]))
@pytest.mark.parametrize("p_reject", [0.02, 0.3])
def test_repacking_equals_the_restatement(case, p_reject):
    sc = tu.contaminated_scene(*case)[0]
    rng = np.random.default_rng(100 + case[0])
    n_dropped_rays = 0
    for trial in range(4):
        reject = (rng.random(sc.n_obs) < p_reject).astype(np.uint8)
        # weights above the counts, as a view of a larger rig has them
        sc2 = tu.copy.copy(sc)
        sc2.ray_weight = sc.ray_weight + rng.integers(0, 3, sc.n_ray)
        ref = tu.trim_restated(sc2, reject)
        rc, out = _trim_raw(sc2, reject)
        if ref is None:
            assert rc == tu.ENOOBS and _untouched(out)
            continue
        assert rc == 0
        no, nr = out["n_obs"], out["n_ray"]
        assert no == len(ref["cam"]) and nr == len(ref["w"])
        assert (out["uv"][:no] == ref["uv"]).all() and (out["cam"][:no] == ref["cam"]).all() and (out["ray"][:no] == ref["ray"]).all()
        assert (out["w"][:nr] == ref["w"]).all() and (out["ray_map"] == ref["ray_map"]).all()
        assert (np.diff(out["ray"][:no]) >= 0).all() and (np.bincount(out["ray"][:no], minlength=nr) >= 2).all()
        assert (out["uv"][no:] == -7).all() and (out["w"][nr:] == -7).all()  # nothing beyond the new extents
        n_dropped_rays += int((ref["ray_map"] < 0).sum())
    if p_reject == 0.3:
        assert n_dropped_rays > 0  # the case of a ray falling below two observations is exercised


def test_repacking_drops_a_ray_left_with_one_observation_and_keeps_views():
    sc = tu.clean_scene(*tu.CLEAN)
    api = tu.pkg().api
    start = np.searchsorted(sc.obs_ray, np.arange(sc.n_ray + 1))
    r = int(np.argmin(np.diff(start)))  # a shortest ray: reject all but one of its observations
    reject = np.zeros(sc.n_obs, dtype=np.uint8)
    reject[start[r] + 1:start[r + 1]] = 1
    t, ray_map = api.ba_trim_problem(sc, reject)
    assert ray_map[r] == -1 and (ray_map[:r] == np.arange(r)).all() and (ray_map[r + 1:] == np.arange(r, sc.n_ray - 1)).all()
    assert t.n_ray == sc.n_ray - 1 and t.n_obs == sc.n_obs - (start[r + 1] - start[r])
    assert (t.ray_weight == np.delete(sc.ray_weight, r)).all()
    # one observation of a ray rejected: the ray stays, its weight goes down by one
    r2 = int(np.argmax(np.diff(start)))
    reject[:] = 0
    reject[start[r2]] = 1
    t, ray_map = api.ba_trim_problem(sc, reject)
    assert (ray_map == np.arange(sc.n_ray)).all() and t.n_obs == sc.n_obs - 1 and t.ray_weight[r2] == sc.ray_weight[r2] - 1
    # a camera emptied: PTZ_ENOOBS, outputs untouched
    reject[:] = (sc.obs_cam == 2).astype(np.uint8)
    rc, out = _trim_raw(sc, reject)
    assert rc == tu.ENOOBS and _untouched(out)
    with pytest.raises(api.PtzError) as ei:
        api.ba_trim_problem(sc, reject)
    assert ei.value.code == tu.ENOOBS


def test_repacking_rejects_malformed_input():
    sc = tu.clean_scene(*tu.CLEAN)
    api = tu.pkg().api
    zero = np.zeros(sc.n_obs, dtype=np.uint8)
    assert _trim_raw(sc, None)[0] == tu.EINVAL
    assert api.lib().ptz_ba_problem_trim(None, _p(zero), None, None, None, None, None, None, None) == tu.EINVAL
    for override in (dict(n_cam=0), dict(n_ray=0), dict(n_obs=0), dict(obs_uv=None), dict(obs_cam=None), dict(obs_ray=None), dict(ray_weight=None),
                     dict(n_cam=sc.n_cam - 1), dict(n_ray=sc.n_ray - 1)):
        rc, out = _trim_raw(sc, zero, **override)
        assert rc == tu.EINVAL and _untouched(out), override
    bad = tu.copy.copy(sc)
    bad.obs_ray = sc.obs_ray.copy()
    bad.obs_ray[[3, 4]] = bad.obs_ray[[40, 3]]  # decreasing
    rc, out = _trim_raw(bad, zero)
    assert rc == tu.EINVAL and _untouched(out)
    keep = []
    p = api._pack_problem(sc, keep)
    rc, out = _trim_raw(sc, zero)
    assert rc == 0 and out["n_obs"] == sc.n_obs and out["n_ray"] == sc.n_ray  # nothing rejected: the same problem
    nr, no = C.c_int32(), C.c_int64()
    assert api.lib().ptz_ba_problem_trim(C.byref(p), _p(zero), _p(out["uv"]), _p(out["cam"]), _p(out["ray"]), _p(out["w"]), None, C.byref(nr),
                                         C.byref(no)) == tu.EINVAL


@pytest.mark.parametrize("case", tu.CONTAMINATED + [tu.CLEAN + (0.0,)], ids=lambda c: "scene%d-type%d" % (c[0], c[3]))
def test_selection_header_agrees_with_the_restatement_on_oracle_residuals(case):
    o = tu.orc()
    sc = tu.contaminated_scene(*case)[0] if case[4] > 0 else tu.clean_scene(*case[:4])
    cam, ray = o.ba_solve(sc, jacobian_mode=o.JAC_ANALYTIC)[:2]
    err = tu.err_norm(o.ba_residuals(sc, cam, ray))
    for trim_px, k_sigma in ((4.0, 3.0), (4.0, 0.0), (0.5, 3.0), (0.25, 0.0), (1.0, 12.0)):
        for n in (len(err), len(err) - 1):  # an even and an odd count (the last observation left out: its ray is one shorter)
            obs_ray, e = sc.obs_ray[:n], err[:n]
            n_ray = int(obs_ray[-1]) + 1
            ref = tu.select_restated(obs_ray, n_ray, e, trim_px, k_sigma)
            got = tu.select_host(obs_ray, n_ray, e, trim_px, k_sigma)
            assert (got[0] == ref[0]).all() and got[1] == ref[1]
            assert (np.isnan(got[2]) and ref[2] is None) or got[2] == ref[2]
            assert (got[3] == ref[3]).all() and (got[4] == ref[4]).all()
            assert (np.bincount(obs_ray[got[0] != 0], minlength=n_ray) <= 1).all()  # at most one per ray
            if k_sigma == 0:
                assert got[1] == trim_px


def test_selection_lower_median_and_lowest_index_on_a_tie():
    obs_ray = np.array([0, 0, 0, 1, 1, 2, 2, 2], dtype=np.int32)
    err = np.array([5.0, 9.0, 9.0, 1.0, 1.0, 2.0, 7.0, 3.0])
    rej, t, med, ray_max, ray_worst = tu.select_host(obs_ray, 3, err, 4.0, 0.0)
    assert list(ray_worst) == [1, 3, 6] and list(ray_max) == [9.0, 1.0, 7.0] and t == 4.0 and np.isnan(med)
    assert list(rej) == [0, 1, 0, 0, 0, 0, 1, 0]  # the worst only, the first of two equal
    # even count: the LOWER median, element (8 - 1) // 2 = 3 of [1, 1, 2, 3, 5, 7, 9, 9]
    _, t, med, _, _ = tu.select_host(obs_ray, 3, err, 4.0, 3.0)
    assert med == 3.0 and t == 3.0 * 3.0 / 1.1774
    # odd count: the middle element, 3 of [1, 1, 2, 3, 5, 7, 9]
    _, t, med, _, _ = tu.select_host(obs_ray[:7], 3, np.delete(err, 2), 4.0, 1.0)
    assert med == 3.0 and t == 4.0
    # equal to the threshold is not above it
    rej = tu.select_host(np.array([0, 0], dtype=np.int32), 1, np.array([4.0, 3.0]), 4.0, 0.0)[0]
    assert rej.sum() == 0
    assert tu.harness().ba_trim_harness_survives(1) == 0 and tu.harness().ba_trim_harness_survives(2) == 1
    assert tu.harness().ba_trim_harness_select(C.c_int64(0), 0, None, None, C.c_double(0.0), C.c_double(3.0), None, None, None, None, None) == -1


@pytest.mark.parametrize("case", tu.CONTAMINATED, ids=lambda c: "scene%d-type%d" % (c[0], c[3]))
def test_rule_recovers_the_contaminated_rig_on_the_oracle(case):
    sc, bad = tu.contaminated_scene(*case)
    assert bad.sum() == int(round(case[4] * sc.n_obs))
    r = tu.oracle_loop(*case)
    good_removed = int((r["kept"][~bad] == 0).sum())
    ferr, clean = tu.focal_error(sc, r["cam"]), tu.clean_fit_focal_error(*case[:4])
    print(f"{case}: {int(bad.sum())} of {sc.n_obs} displaced, rounds {r['rounds']}, displaced left {int(r['kept'][bad].sum())}, "
          f"good removed {good_removed} ({100.0 * good_removed / (~bad).sum():.1f} %), focal error {ferr:.3f} px (clean fit {clean:.3f}), "
          f"threshold {r['threshold']:.3f}, margin {r['margin']:.2e}")
    assert r["kept"][bad].sum() == 0               # every displaced observation is removed
    assert good_removed <= 0.05 * (~bad).sum()     # at most 5 % of the untouched ones
    assert r["rounds"] < 8 and not r["flagged"]    # the loop ends before max_rounds
    assert ferr <= 1.5 * clean
    assert r["n_obs_removed"] == int((r["kept"] == 0).sum())


def test_rule_leaves_the_clean_rig_alone_on_the_oracle():
    r = tu.oracle_loop(*tu.CLEAN, 0.0)
    assert r["rounds"] == 1 and r["n_obs_removed"] == 0 and r["n_ray_removed"] == 0 and r["kept"].all() and not r["flagged"]


def test_trimmed_solve_checks_come_before_any_device_work():
    api = tu.pkg().api
    sc = tu.clean_scene(*tu.CLEAN)
    keep = []
    p = api._pack_problem(sc, keep)
    cam, ray = np.array(sc.cam_init), np.array(sc.ray_init)
    o = api.default_options()
    to = api.TrimOptions()
    api.lib().ptz_trim_options_default(C.byref(to))
    assert (to.trim_px, to.k_sigma, to.max_rounds) == (4.0, 3.0, 8)

    def call(prob, topt):
        return api.lib().ptz_ba_solve_trimmed(C.byref(prob) if prob is not None else None, _p(cam), _p(ray), None, C.byref(topt), C.byref(o), None, None, None)

    assert call(None, to) == tu.EINVAL
    for k, v in (("trim_px", 0.0), ("trim_px", float("nan")), ("k_sigma", -1.0), ("max_rounds", 0)):
        bad = api.TrimOptions(to.trim_px, to.k_sigma, to.max_rounds, 0)
        setattr(bad, k, v)
        assert call(p, bad) == tu.EINVAL, (k, v)
    p.factor_type = api.BA_PTZRayDistDisp
    assert call(p, to) == tu.EUNSUPPORTED
    p.factor_type = sc.factor_type
    ic = np.zeros(sc.n_cam, dtype=np.int32)
    p.ic_of_cam = _p(ic)
    assert call(p, to) == tu.EUNSUPPORTED
    assert api.lib().ptz_ba_batch_residuals(None, _p(cam), None, None, None, None, None, None, None, None, None, None) == tu.EINVAL
    assert api.lib().ptz_ba_batch_trim_select(None, C.c_double(4.0), C.c_double(3.0), _p(cam), None, None, None) == tu.EINVAL
