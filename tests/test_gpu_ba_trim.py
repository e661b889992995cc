"""GPU tests of the trimmed bundle adjustment (ptz_ba_solve_trimmed / _batch, ptz-calib_amd/csrc/ptz_ba_trim.cc on top of the
residual report of ptz_ba_resid.hip): the kept set, rounds and cameras against the loop written on the CPU oracle
(ba_trim_util.oracle_loop, the loop test_cpu_ba_trim.py checks), the clean rig, the batch form against the solo calls, the
manual loop over the public calls, the C++ class (SetTrimming, ViewResiduals) and run_ptz_ba --trim_px."""
import copy
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import ba_trim_util as tu
import host_util as hu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = ["scene%d-type%d" % (c[0], c[3]) for c in tu.CONTAMINATED]


@pytest.mark.parametrize("case", tu.CONTAMINATED, ids=CASE_IDS)
def test_trimmed_solve_equals_the_oracle_loop(case):
    api = tu.pkg().api
    sc, bad = tu.contaminated_scene(*case)
    ref = tu.oracle_loop(*case)
    # the condition under which the two kept sets must be identical: no ray_max of any round within 1e-6 px of the round's threshold
    assert ref["margin"] > 1e-6, ref["margin"]
    cam, ray, summ, kept, rep = api.ba_solve_trimmed(sc)
    rel = float(np.abs(cam - ref["cam"]).max() / np.abs(ref["cam"]).max())
    relf = float((np.abs(cam[:, 0] - ref["cam"][:, 0]) / ref["cam"][:, 0]).max())
    print(f"{case}: rounds {rep['rounds']} (oracle {ref['rounds']}), removed {rep['n_obs_removed']} obs / {rep['n_ray_removed']} rays, threshold "
          f"{rep['threshold']:.3f}, rms {rep['rms_first']:.3f} -> {rep['rms_last']:.3f} px, cameras vs oracle: max rel {rel:.2e}, focal rel {relf:.2e}")
    assert (kept == ref["kept"]).all()
    assert rep["rounds"] == ref["rounds"] and rep["n_obs_removed"] == ref["n_obs_removed"] and rep["n_ray_removed"] == ref["n_ray_removed"]
    assert rep["flags"] == 0 and abs(rep["threshold"] / ref["threshold"] - 1) <= 1e-9
    assert abs(rep["rms_first"] / ref["rms_first"] - 1) <= 1e-6 and abs(rep["rms_last"] / ref["rms_last"] - 1) <= 1e-6
    assert rel <= 1e-6 and relf <= 1e-6  # the project's bound for cameras against the oracle
    assert summ["termination_type"] == api.CONVERGENCE
    assert kept[bad].sum() == 0
    # rays removed come back as given, the others moved
    gone = np.bincount(sc.obs_ray[kept != 0], minlength=sc.n_ray) == 0
    assert gone.sum() == rep["n_ray_removed"] and (ray[gone] == sc.ray_init[gone]).all() and (ray[~gone] != sc.ray_init[~gone]).any(axis=1).all()


def test_trimmed_solve_is_the_manual_loop_over_the_public_calls():
    api = tu.pkg().api
    case = tu.CONTAMINATED[1]
    sc = tu.contaminated_scene(*case)[0]
    cam_t, ray_t, _, kept_t, rep = api.ba_solve_trimmed(sc)
    cur, cam, ray, obs = sc, sc.cam_init, sc.ray_init, np.arange(sc.n_obs)
    rounds = 0
    while True:
        cam, ray, _ = api.ba_solve(cur, cam0=cam, ray0=ray)
        rounds += 1
        b = api.BaBatch([cur])
        b.set_state(cams=[cam], rays=[ray])
        rej, thr, nrej, _ = b.trim_select()
        r = b.residuals()[0]
        b.close()
        host = tu.select_host(cur.obs_ray, cur.n_ray, r["err_px"], 4.0, 3.0)  # the report and the header on the host: the same selection
        assert (host[0] == rej[0]).all() and host[1] == thr[0]
        if nrej[0] == 0:
            break
        new, rmap = api.ba_trim_problem(cur, rej[0])
        keep = (rej[0] == 0) & (rmap[cur.obs_ray] >= 0)
        obs, ray, cur = obs[keep], ray[rmap >= 0], new
    kept = np.zeros(sc.n_obs, dtype=np.uint8)
    kept[obs] = 1
    assert rounds == rep["rounds"] and (kept == kept_t).all()
    assert (cam == cam_t).all()  # the same bits
    assert (ray == ray_t[np.bincount(sc.obs_ray[kept != 0], minlength=sc.n_ray) > 0]).all()


def test_clean_rig_is_left_alone():
    api = tu.pkg().api
    sc = tu.clean_scene(*tu.CLEAN)
    cam0, ray0, s0 = api.ba_solve(sc)
    cam, ray, summ, kept, rep = api.ba_solve_trimmed(sc)
    assert kept.all() and rep["rounds"] == 1 and rep["n_obs_removed"] == 0 and rep["n_ray_removed"] == 0 and rep["flags"] == 0
    assert (cam == cam0).all() and (ray == ray0).all() and summ == s0
    assert rep["rms_first"] == rep["rms_last"]


def test_batch_gives_the_bits_of_the_solo_calls():
    api = tu.pkg().api
    scenes = [tu.contaminated_scene(*c)[0] for c in tu.CONTAMINATED if c[3] == 0] + [tu.clean_scene(*tu.CLEAN)]
    scenes += [tu.contaminated_scene(15, 12, 60, 0, 0.10)[0]]  # five rigs of one factor type, finishing in different rounds
    assert len(scenes) == 5
    cams, rays, summ, kept, rep = api.ba_solve_trimmed_batch(scenes)
    rounds = [r["rounds"] for r in rep]
    print(f"batch of five: rounds {rounds}, removed {[r['n_obs_removed'] for r in rep]}")
    assert len(set(rounds)) >= 3
    for i, sc in enumerate(scenes):
        c, r, s, k, p = api.ba_solve_trimmed(sc)
        assert (cams[i] == c).all() and (rays[i] == r).all() and (kept[i] == k).all() and summ[i] == s and rep[i] == p, i
    # the other two factor types, each beside a second problem of its type
    for ft_case in (tu.CONTAMINATED[1], tu.CONTAMINATED[4]):
        a = tu.contaminated_scene(*ft_case)[0]
        b = tu.clean_scene(tu.CLEAN[0], tu.CLEAN[1], tu.CLEAN[2], ft_case[3])
        cams, rays, summ, kept, rep = api.ba_solve_trimmed_batch([b, a])
        c, r, s, k, p = api.ba_solve_trimmed(a)
        assert (cams[1] == c).all() and (rays[1] == r).all() and (kept[1] == k).all() and rep[1] == p


def test_rounds_run_out_and_a_view_is_never_dropped():
    api = tu.pkg().api
    case = tu.CONTAMINATED[3]
    sc = tu.contaminated_scene(*case)[0]
    cam, ray, summ, kept, rep = api.ba_solve_trimmed(sc, max_rounds=2)
    assert rep["rounds"] == 2 and rep["flags"] == api.TRIM_MAX_ROUNDS and 0 < rep["n_obs_removed"] < tu.oracle_loop(*case)["n_obs_removed"]
    # one camera's pixels all displaced by 200 px, and a threshold no fit can meet: trimming stops where a view would go, flagged
    s2 = copy.copy(tu.clean_scene(*tu.CLEAN))
    s2.obs_uv = s2.obs_uv.copy()
    s2.obs_uv[s2.obs_cam == 2] += np.float32(200.0)
    cam, ray, summ, kept, rep = api.ba_solve_trimmed(s2, trim_px=1e-3, k_sigma=0.0, max_rounds=50)
    print(f"hopeless threshold: rounds {rep['rounds']}, flags {rep['flags']}, removed {rep['n_obs_removed']} of {s2.n_obs}")
    assert rep["flags"] in (api.TRIM_ENOOBS, api.TRIM_MAX_ROUNDS)
    assert (np.bincount(s2.obs_cam[kept != 0], minlength=s2.n_cam) > 0).all()


# ---- the C++ class ---------------------------------------------------------------------------------------------------------------
def _class_solve(sc, trim_px=0.0, k_sigma=3.0, max_rounds=8, use_rig=False, cand=()):
    """PTZRayOptimizer through ptzh_ptzray_solve_trim: dict(ok, view_ok, cam, summary, report, kept, view_rms/max/count, packed)"""
    api = tu.pkg().api
    kps, plist = hu.scene_to_features_matches(sc)
    n_img = len(kps)
    kp_ptr = np.concatenate([[0], np.cumsum([len(k) for k in kps])]).astype(np.int64)
    kp_xy = np.ascontiguousarray(np.concatenate([np.asarray(k, dtype=np.float32).reshape(-1, 2) for k in kps]), dtype=np.float32)
    src = np.array([p[0] for p in plist], dtype=np.int64); dst = np.array([p[1] for p in plist], dtype=np.int64)
    mptr = np.concatenate([[0], np.cumsum([len(p[2]) for p in plist])]).astype(np.int64)
    q = np.array([m[0] for p in plist for m in p[2]], dtype=np.int32); t = np.array([m[1] for p in plist for m in p[2]], dtype=np.int32)
    cam = np.array(sc.cam_init, dtype=np.float64, order="C").copy()
    cand = np.array(list(cand), dtype=np.int64)
    ncam = len(cand) if len(cand) else n_img
    summ, rep = api.LmSummary(), api.TrimReport()
    kept, n_kept = C.POINTER(C.c_uint8)(), C.c_int32()
    vr, vm, vc = np.zeros(ncam), np.zeros(ncam), np.zeros(ncam, dtype=np.int32)
    n_obs, n_ray = C.c_int32(), C.c_int32()
    puv, pcam, pray, pw = C.POINTER(C.c_float)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)()
    pc15, pr3, pci = C.POINTER(C.c_double)(), C.POINTER(C.c_double)(), C.POINTER(C.c_int64)()
    rc = hu.lib().ptzh_ptzray_solve_trim(n_img, hu._p(kp_ptr), hu._p(kp_xy), len(plist), hu._p(src), hu._p(dst), hu._p(mptr), hu._p(q), hu._p(t), hu._p(cam),
                                         hu._p(cand) if len(cand) else None, len(cand), 200, sc.factor_type, C.c_double(trim_px), C.c_double(k_sigma),
                                         int(max_rounds), int(use_rig), C.byref(summ), C.byref(rep), C.byref(kept), C.byref(n_kept), hu._p(vr), hu._p(vm),
                                         hu._p(vc), C.byref(n_obs), C.byref(n_ray), C.byref(puv), C.byref(pcam), C.byref(pray), C.byref(pw), C.byref(pc15),
                                         C.byref(pr3), C.byref(pci))
    assert rc >= 0
    no, nr = n_obs.value, n_ray.value
    packed = dict(obs_uv=np.ctypeslib.as_array(puv, (max(no, 1), 2))[:no].copy(), obs_cam=np.ctypeslib.as_array(pcam, (max(no, 1),))[:no].copy(),
                  obs_ray=np.ctypeslib.as_array(pray, (max(no, 1),))[:no].copy(), ray_weight=np.ctypeslib.as_array(pw, (max(nr, 1),))[:nr].copy(),
                  cam=np.ctypeslib.as_array(pc15, (ncam, 15)).copy(), ray=np.ctypeslib.as_array(pr3, (max(nr, 1), 3))[:nr].copy())
    k = np.ctypeslib.as_array(kept, (max(n_kept.value, 1),))[:n_kept.value].copy()
    for x in (puv, pcam, pray, pw, pc15, pr3, pci, kept):
        hu.lib().ptzh_free(x)
    return dict(ok=bool(rc & 1), view_ok=bool(rc & 2), cam=cam, summary=summ.as_dict(), report=rep.as_dict(), kept=k, view_rms=vr, view_max=vm,
                view_count=vc, packed=packed)


def _packed_scene(sc, packed):
    """the problem the class packed (its own track order), as a scene"""
    ps = copy.copy(sc)
    ps.n_ray = len(packed["ray_weight"])
    ps.obs_uv, ps.obs_cam, ps.obs_ray, ps.ray_weight = packed["obs_uv"], packed["obs_cam"], packed["obs_ray"], packed["ray_weight"]
    return ps


def _obs_keys(obs_cam, obs_uv):
    """an observation's identity whatever the track order: (camera, pixel)"""
    return {(int(c), float(u), float(v)) for c, (u, v) in zip(obs_cam, obs_uv)}


def test_class_with_trimming_keeps_the_same_set_and_reports_the_views():
    api = tu.pkg().api
    case = tu.CONTAMINATED[0]
    sc = tu.contaminated_scene(*case)[0]
    ref = tu.oracle_loop(*case)
    ps = _packed_scene(sc, _class_solve(sc)["packed"])  # the class numbers the tracks its own way: the problem as it packs it
    assert ps.n_obs == sc.n_obs and _obs_keys(ps.obs_cam, ps.obs_uv) == _obs_keys(sc.obs_cam, sc.obs_uv) and len(_obs_keys(sc.obs_cam, sc.obs_uv)) == sc.n_obs
    r = _class_solve(sc, trim_px=4.0)
    assert r["ok"] and r["view_ok"]
    assert len(r["kept"]) == sc.n_obs
    k = r["kept"] != 0
    assert _obs_keys(ps.obs_cam[k], ps.obs_uv[k]) == _obs_keys(sc.obs_cam[ref["kept"] != 0], sc.obs_uv[ref["kept"] != 0])  # the same kept set
    assert r["report"]["rounds"] == ref["rounds"] and r["report"]["n_obs_removed"] == ref["n_obs_removed"]
    assert r["report"]["n_ray_removed"] == ref["n_ray_removed"]
    # packed() is the trimmed problem: what the C re-packing makes of the packed problem and the kept set
    t, rmap = api.ba_trim_problem(ps, 1 - r["kept"])
    p = r["packed"]
    assert (p["obs_uv"] == t.obs_uv).all() and (p["obs_cam"] == t.obs_cam).all() and (p["obs_ray"] == t.obs_ray).all() and (p["ray_weight"] == t.ray_weight).all()
    assert len(p["ray"]) == t.n_ray
    assert (np.abs(r["cam"][:, 0] - ref["cam"][:, 0]) / ref["cam"][:, 0]).max() <= 1e-6
    # ViewResiduals is the batch report of that problem at that state
    b = api.BaBatch([t])
    b.set_state(cams=[p["cam"]], rays=[p["ray"]])
    rep = b.residuals()[0]
    b.close()
    assert (r["view_rms"] == rep["view_rms"]).all() and (r["view_max"] == rep["view_max"]).all() and (r["view_count"] == rep["view_count"]).all()


def test_class_without_trimming_is_what_it_was_and_reports_views_on_both_paths():
    api = tu.pkg().api
    sc = tu.contaminated_scene(*tu.CONTAMINATED[0])[0]
    kps, plist = hu.scene_to_features_matches(sc)
    ok0, cam0, err0, summ0, packed0 = hu.ptzray_solve(kps, plist, sc.cam_init, ftype=sc.factor_type)  # the helper that predates trimming
    r = _class_solve(sc)
    assert ok0 and r["ok"] and (r["cam"] == cam0).all() and r["summary"] == summ0
    assert len(r["kept"]) == 0 and r["report"]["rounds"] == 0
    assert (r["packed"]["obs_uv"] == packed0["obs_uv"]).all() and (r["packed"]["cam"] == packed0["cam"]).all() and (r["packed"]["ray"] == packed0["ray"]).all()
    # packed path: the report of the packed problem at the solution
    b = api.BaBatch([_packed_scene(sc, packed0)])
    b.set_state(cams=[packed0["cam"]], rays=[packed0["ray"]])
    rep = b.residuals()[0]
    b.close()
    assert r["view_ok"] and (r["view_rms"] == rep["view_rms"]).all() and (r["view_max"] == rep["view_max"]).all() and (r["view_count"] == rep["view_count"]).all()
    # rig-view path: trimming is ignored (the solve is the untrimmed one), the views are still reported
    g = _class_solve(sc, trim_px=4.0, use_rig=True)
    assert g["ok"] and g["view_ok"] and len(g["kept"]) == 0 and g["report"]["rounds"] == 0
    assert (np.abs(g["cam"][:, 0] - cam0[:, 0]) / cam0[:, 0]).max() <= 1e-9
    assert (g["view_count"] == rep["view_count"]).all()
    assert np.abs(g["view_rms"] / rep["view_rms"] - 1).max() <= 1e-6 and np.abs(g["view_max"] / rep["view_max"] - 1).max() <= 1e-6


# ---- the tool --------------------------------------------------------------------------------------------------------------------
def _run_tool(*args):
    return subprocess.run([os.path.join(ROOT, "ptz-calib_amd", "bin", "run_ptz_ba"), *args], capture_output=True, text=True, timeout=600)


def _tool_cams(out_dir):
    f = os.path.join(out_dir, "rig0.json")
    return json.load(open(f))["cameras"] if os.path.exists(f) else None


def _max_focal_error(cams, sc, names):
    idx = {os.path.splitext(n)[0]: i for i, n in enumerate(names)}
    return max(abs(np.array(c["K"])[0] - sc.cam_gt[idx[n], 0]) for n, c in cams.items())


def test_run_ptz_ba_trim_px(tmp_path):
    """A 20-view annotated data set written by dataset_io.  In the contaminated copy key points are displaced by 20..80 px (the
    contamination of ba_trim_util) so that 10 % of the pair matches have a displaced end: a match displaced on its own would put two
    key points of one image into its track, and the track builder drops such tracks whole -- nothing wrong would reach the bundle
    adjustment."""
    pkg = tu.pkg()
    sc = pkg.synth.add_annotations(pkg.synth.make_scene(1, 20, 100))
    clean = pkg.dataset_io.write_rig(str(tmp_path / "clean"), sc, pkg.synth.make_match_table(sc), annotations=sc.obs3d)
    rng = np.random.default_rng(tu.CONTAMINATION_SEED)
    idx = rng.choice(sc.n_obs, size=int(round(0.0513 * sc.n_obs)), replace=False)  # 1 - (1 - f)^2 = 0.10
    ang, mag = rng.uniform(0.0, 2.0 * np.pi, len(idx)), rng.uniform(20.0, 80.0, len(idx))
    dirty_sc = copy.copy(sc)
    dirty_sc.obs_uv = np.array(sc.obs_uv, dtype=np.float32).copy()
    dirty_sc.obs_uv[idx] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1).astype(np.float32)
    tb = pkg.synth.make_match_table(dirty_sc)
    moved = np.zeros(sc.n_obs, dtype=bool); moved[idx] = True
    order = np.argsort(sc.obs_cam, kind="stable")
    moved_kp = moved[order]  # per key point of the table (camera-major)
    pair_of = np.repeat(np.arange(tb.n_pairs), np.diff(tb.match_ptr))
    share = float(np.mean(moved_kp[tb.kp_ptr[tb.src[pair_of]] + tb.q] | moved_kp[tb.kp_ptr[tb.dst[pair_of]] + tb.t]))
    assert 0.08 <= share <= 0.12, share
    dirty = pkg.dataset_io.write_rig(str(tmp_path / "dirty"), dirty_sc, tb, annotations=sc.obs3d)

    def run(paths, out, *flags):
        r = _run_tool("-i", paths["images"], "-f", paths["features"], "-a", paths["annotation"], "--output=" + str(tmp_path / out), *flags)
        return r, _tool_cams(str(tmp_path / out))

    rc, cams_clean = run(clean, "out_clean")
    rp, cams_plain = run(dirty, "out_plain")
    rt, cams_trim = run(dirty, "out_trim", "--trim_px", "4")
    assert rc.returncode == 0 and rp.returncode == 0 and rt.returncode == 0, (rc.stderr[-2000:], rp.stderr[-2000:], rt.stderr[-2000:])
    fe = [_max_focal_error(c, sc, clean["names"]) for c in (cams_clean, cams_plain, cams_trim)]
    print(f"run_ptz_ba: {100 * share:.1f} % of the pair matches displaced; max focal error clean {fe[0]:.3f} px, contaminated {fe[1]:.3f} px, "
          f"contaminated with --trim_px 4 {fe[2]:.3f} px; registered {len(cams_clean)} / {len(cams_plain)} / {len(cams_trim)}")
    # without the flag no side file appears; with it the main output differs from the run without
    assert not os.path.exists(str(tmp_path / "out_plain" / "rig0_residuals.json"))
    assert open(str(tmp_path / "out_trim" / "rig0.json"), "rb").read() != open(str(tmp_path / "out_plain" / "rig0.json"), "rb").read()
    side = json.load(open(str(tmp_path / "out_trim" / "rig0_residuals.json")))
    reg = set(cams_trim.keys())
    assert {os.path.splitext(n)[0] for n in side["images"]} == reg  # every registered image is listed
    assert side["rounds"] >= 2 and side["observations_removed"] > 0 and side["threshold"] >= 4.0
    assert sum(v["n_removed"] for v in side["images"].values()) == side["observations_removed"]
    assert all(v["n_obs"] > 0 and 0 < v["rms_px"] <= v["max_px"] for v in side["images"].values())
    assert fe[2] <= 1.5 * fe[0]
    # --uncertainty with --trim_px: the side files are written, the main output is the trimmed run's
    ru, cams_u = run(dirty, "out_trim_u", "--trim_px", "4", "--uncertainty")
    assert ru.returncode == 0
    assert open(str(tmp_path / "out_trim_u" / "rig0.json"), "rb").read() == open(str(tmp_path / "out_trim" / "rig0.json"), "rb").read()
    assert os.path.exists(str(tmp_path / "out_trim_u" / "rig0_uncertainty.json")) and os.path.exists(str(tmp_path / "out_trim_u" / "rig0_residuals.json"))
    # bad options
    assert _run_tool("-i", clean["images"], "-f", clean["features"], "-a", clean["annotation"], "--output=" + str(tmp_path / "x"), "--trim_px", "0").returncode == 1
