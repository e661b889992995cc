"""GPU tests of relocalization against the landmark map from a prior camera (ptz_relocalizer_run_landmarks_tracked,
api.Relocalizer.run(landmarks=, landmark_prior=)) on the data set of test_gpu_relocalizer_prior.py: the 20-view rig
make_scene(0, 20, 100), make_reloc_scene(n_query=24, n_feat=600, visible_share=0.5, noise_px=0.5, seed=0), REPEATED texture
make_reloc_descriptors(D=128, noise=12, n_distractors=50, seed=0, repeat_share=0.7, repeat_group=4, repeat_noise=6), the tracks of
synth_reloc.scene_tracks(sc, 50).  Priors: perturb_cameras(cam_gt, 0.3 degrees, 2 %, seed=0), radius 40 px; the matcher runs with
min_matches = 8.

THE CPU EXPERIMENT behind the accuracy test, before any device run (tools/probes/probe_landmark_prior_accuracy_cpu.py, figures in
profiles/landmark_prior_accuracy_cpu.json): the numpy map (landmark_util), the restated view (landmark_prior_util), the restated
guided matcher under identity H (desc_guided_util.match_pairs_guided), the numpy landmark assembly, the homography_harness RANSAC
(4 px) as the gate on the assembled query and the ORACLE's krt_solve_batch; scene, descriptor and perturbation seed equal, 0 .. 5.
24 of 24 queries accepted in every row of every seed, no query lost; min_inliers 6 and 30 give the same cameras.

                 median error: dense landmark run / prior, no gate / prior + gate        matches per query (median)
    F (relative focal)   seed 0: 3.14e-5 2.39e-4 2.90e-5   1: 6.76e-5 4.56e-5 3.58e-5   2: 7.53e-5 8.10e-5 4.05e-5     162 / 510 / 508 (seed 0)
                              3: 4.63e-5 8.22e-5 3.97e-5   4: 5.42e-5 7.72e-5 3.74e-5   5: 6.05e-5 5.87e-5 2.00e-5
      ratio prior + gate / dense: 0.92 0.53 0.54 0.86 0.69 0.33      (no gate / dense: 7.61 0.67 1.08 1.78 1.42 0.97)
    FDist (k1)           seed 0: 1.53e-3 1.53e-3 7.97e-4   1: 1.83e-3 3.65e-3 6.99e-4   2: 1.36e-3 1.74e-3 4.25e-4     163 / 528 / 526 (seed 0)
                              3: 1.16e-3 1.73e-3 9.74e-4   4: 1.37e-3 1.49e-3 8.09e-4   5: 1.64e-3 1.54e-3 1.02e-3
      ratio prior + gate / dense: 0.52 0.38 0.31 0.84 0.59 0.62      (no gate / dense: 1.00 1.99 1.27 1.50 1.08 0.94)
      (FDist seed 0, relative focal: 1.25e-4 2.03e-4 7.33e-5)
All twelve ratios prior + gate / dense are below 1 and the match count triples in every run, so the assertions of the accuracy test
hold for 6 of 6 seeds, F and FDist; the test uses seed 0.  12 165 to 12 964 landmarks, 2 580 to 3 342 of them visible per query at
the median, at most 8 268.  The lone-candidate finding of the tracked run repeats: WITHOUT the gate the prior path is worse than the
dense one in 8 of 12 runs, which is why the run forces the gate on.
Priors 30 degrees off (F, seed 0; 1 628 landmarks visible at the median, all of them wrong): min_inliers = 6 accepts queries 5, 11
and 19 of 24, min_inliers = 30 none."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import desc_guided_util as gu
import homography_corpus as hc
import landmark_prior_util as lp
import reloc_prior_util as pu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM = dict(max_num_iterations=200)
TRIM = dict(trim_px=2.0, k_sigma=3.0, max_rounds=8, min_keep=8)
MATCH = dict(min_matches=8)
RADIUS = 40.0
I9 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.float64)
PER_QUERY = ("cam", "accepted", "summaries", "sel_ref", "n_sel", "n_matches", "n_inliers", "trim_report", "cov", "sigma0", "cov_status")


def _same(x, y):
    if x is None or y is None:
        return x is None and y is None
    if isinstance(x, (list, tuple)):
        return len(x) == len(y) and all(_same(u, v) for u, v in zip(x, y))
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(_same(x[k], y[k]) for k in x)
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


@pytest.fixture(scope="module")
def scenes(pkg):
    """per factor type: the scene, the resident sets, the map, the relocalizer, the priors (shared: the tests only run them)"""
    out = {}
    for ft in (0, 1):
        rig = pkg.synth.make_scene(0, 20, 100).cam_gt.copy()
        if ft:
            rig[:, 10] = np.random.default_rng(100).uniform(-0.05, 0.05, len(rig))
        sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=24, n_feat=600, visible_share=0.5, noise_px=0.5, factor_type=ft, seed=0)
        rf, qf = pkg.synth_reloc.make_reloc_descriptors(sc, D=128, noise=12, n_distractors=50, seed=0, repeat_share=0.7, repeat_group=4,
                                                        repeat_noise=6)
        tp, ti, tf, _ = pkg.synth_reloc.scene_tracks(sc, 50)
        refs, tests = pkg.api.DescSet(*rf), pkg.api.DescSet(*qf)
        lmap = pkg.api.LandmarkMap(refs, rig, tp, ti, tf, factor_type=ft)
        out[ft] = types.SimpleNamespace(sc=sc, rig=rig, refs=refs, tests=tests, qf=qf, lmap=lmap, rl=pkg.api.Relocalizer(refs, rig),
                                        prior=pkg.synth_reloc.perturb_cameras(sc.cam_gt, 0.3, 0.02, seed=0))
    yield out
    for s in out.values():
        s.rl.close(); s.lmap.close(); s.tests.close(); s.refs.close()


def _lift(view, g):
    pair_of = np.repeat(np.arange(len(g["match_ptr"]) - 1), np.diff(g["match_ptr"]))
    return view["vis_lm"][view["vis_ptr"][pair_of] + g["idx_a"]].astype(np.int32)


@pytest.fixture(scope="module")
def expected(pkg, scenes):
    """the hand composition of the public calls, once per (factor type, kernel)"""
    api = pkg.api
    out = {}
    for ft, s in scenes.items():
        nq = s.sc.n_query
        ia = np.arange(nq, dtype=np.int32)
        with api.landmark_visible(s.lmap, s.prior, s.sc.query_wh, factor_type=ft, radius_px=RADIUS) as v:
            view = v.arrays()
            tables = [api.match_descriptors_guided(v.desc_set(), s.tests, ia, ia, np.tile(I9, (nq, 1)), None, RADIUS, grid=bool(grid), **MATCH)
                      for grid in (0, 1)]
        for grid, g in enumerate(tables):
            asm = api.landmark_assemble(s.lmap, g["match_ptr"], _lift(view, g), g["uv_b"], s.sc.query_wh)
            b = types.SimpleNamespace(n_query=nq, match_ptr=asm["match_ptr"], uv_ref=asm["uv_ref"], uv_cur=asm["uv_cur"], cam_ref=asm["cam_ref"],
                                      cam_init=pu.prior_camera(asm["cam_init"], s.prior, ft), factor_type=ft)
            e = dict(view=view, table=g, asm=asm, n_matches=np.diff(asm["match_ptr"]).astype(np.int32))
            cam, summ, acc, ninl, gmask, _, _ = api.krt_solve_batch_gated(b, ransac_thresh=4.0, min_inliers=6, **LM)
            acc = acc * (ninl > 0)
            e["gated"] = dict(cam=cam, summaries=summ, accepted=acc, n_inliers=ninl, trim_report=None,
                              cov=api.krt_covariance_batch(b, cam, match_mask=gmask, accepted=acc)[:3])
            cam, summ, acc, kept, rep, _ = api.krt_solve_batch_trimmed(b, match_mask=gmask, **TRIM, **LM)
            acc = acc * (ninl > 0)
            e["gated_trimmed"] = dict(cam=cam, summaries=summ, accepted=acc, n_inliers=ninl, trim_report=rep,
                                      cov=api.krt_covariance_batch(b, cam, match_mask=kept, accepted=acc)[:3])
            out[ft, grid] = e
    return out


@pytest.mark.parametrize("ft", [0, 1])
@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("variant", ["gated", "gated_trimmed"])
def test_1_run_is_bit_equal_to_the_hand_composition(pkg, scenes, expected, ft, grid, variant):
    """landmark_visible -> match_descriptors_guided (identity H) -> the lift in numpy -> landmark_assemble -> the prior camera rule
    in numpy -> krt_solve_batch_gated / _trimmed -> krt_covariance_batch: every per-query output, the view and the table, bit
    for bit, through the scan kernel and the grid kernel.  inlier_matches is left off: the run forces the gate on."""
    s, e = scenes[ft], expected[ft, grid]
    want = e[variant]
    got = s.rl.run(s.tests, s.sc.query_wh, factor_type=ft, landmarks=s.lmap, landmark_prior=dict(cams=s.prior, radius_px=RADIUS),
                   guided_grid=bool(grid), trim=TRIM if "trimmed" in variant else None, uncertainty=True, match=MATCH, **LM)
    view, table, asm = s.rl.view(), s.rl.table(), s.rl.matches()
    lp.assert_equal(view, e["view"], (ft, "view"))
    assert np.array_equal(got["n_visible"], np.diff(e["view"]["vis_ptr"])) and got["n_visible"].min() > 500 and got["view_ms"] > 0
    for key in ("match_ptr", "idx_a", "idx_b", "dist2", "uv_a", "uv_b"):
        assert np.array_equal(table[key], e["table"][key]), key
    assert np.array_equal(s.rl.pairs()["pair_ref"], np.arange(24))
    for key in ("match_ptr", "uv_ref", "uv_cur", "src"):
        assert np.array_equal(asm[key], e["asm"][key]), key
    assert got["sel_ref"].shape == (24, 1) and np.array_equal(got["sel_ref"][:, 0], e["asm"]["anchor_ref"]) and (got["n_sel"] == 1).all()
    assert np.array_equal(got["n_matches"], e["n_matches"]) and e["n_matches"].min() >= 100
    for key in ("cam", "accepted", "summaries", "n_inliers", "trim_report"):
        assert _same(got[key], want[key]), (ft, grid, variant, key)
    cov, s0, status = want["cov"]
    ok = status == pkg.api.COV_OK
    assert np.array_equal(got["cov_status"], status) and ok.sum() >= 20
    assert np.array_equal(got["cov"][ok], cov[ok]) and np.array_equal(got["sigma0"][ok], s0[ok])
    assert want["accepted"].all() and (got["stage_ms"][:5] > 0).all() and got["stage_ms"][0] == got["view_ms"]


def test_2_the_table_is_the_numpy_restatements(pkg, scenes):
    """The first six queries alone (a query's view depends on its own prior and image only): the run's view against the restated
    one, its match table against desc_guided_util.match_pairs_guided on the restated view under identity H."""
    s = scenes[0]
    n = 6
    qp, qd, qk = s.qf
    cut = int(qp[n])
    lm = s.lmap.arrays()
    view = lp.visible(lm["lm_ray"], s.prior[:n], s.sc.query_wh[:n], 0, RADIUS, prior_R=pkg.api.reloc_ref_rotations(s.prior[:n]))
    want = gu.match_pairs_guided(lm["lm_desc"][view["vis_lm"]], view["vis_ptr"], view["vis_uv"], qd, qp, qk, np.arange(n), np.arange(n),
                                 np.tile(I9, (n, 1)), None, RADIUS, **MATCH)
    with pkg.api.DescSet(qp[:n + 1], qd[:cut], qk[:cut]) as tests:
        got = s.rl.run(tests, s.sc.query_wh[:n], landmarks=s.lmap, landmark_prior=dict(cams=s.prior[:n], radius_px=RADIUS), match=MATCH, **LM)
        lp.assert_equal(s.rl.view(), view, "view")
        gu.assert_equal(s.rl.table(), want)
    assert want["match_ptr"][-1] > 2000 and got["accepted"].all()


@pytest.mark.parametrize("ft", [0, 1])
def test_3_a_prior_beats_the_dense_landmark_run(pkg, scenes, ft):
    """Against the dense landmark run of the same relocalizer on the same descriptors, seed 0: no query the dense run accepts is
    lost, the median match count is larger, and the median relative focal error (F) or k1 error (FDist) is at most the dense
    run's.  The CPU experiment in the module's docstring finds this for 6 of 6 seeds, F and FDist."""
    s = scenes[ft]
    dense = s.rl.run(s.tests, s.sc.query_wh, factor_type=ft, landmarks=s.lmap, match=MATCH, **LM)
    got = s.rl.run(s.tests, s.sc.query_wh, factor_type=ft, landmarks=s.lmap, landmark_prior=dict(cams=s.prior, radius_px=RADIUS), guided_grid=True,
                   match=MATCH, **LM)
    ad, at = dense["accepted"], got["accepted"]
    both = (ad == 1) & (at == 1)
    gt = s.sc.cam_gt
    err = lambda r, col: float(np.median(np.abs(r["cam"][both, col] - gt[both, col]) / (gt[both, col] if col == 0 else 1.0)))
    n_d, n_t = np.median(dense["n_matches"]), np.median(got["n_matches"])
    print(f"factor {ft}: accepted {int(ad.sum())} -> {int(at.sum())}, matches {n_d:.0f} -> {n_t:.0f} ({np.median(got['n_inliers']):.0f} kept), "
          f"focal {err(dense, 0):.3e} -> {err(got, 0):.3e}, k1 {err(dense, 10):.3e} -> {err(got, 10):.3e}, visible {np.median(got['n_visible']):.0f} "
          f"of {s.lmap.n_landmarks}, stage ms dense {dense['stage_ms'].round(3)} tracked {got['stage_ms'].round(3)}")
    assert ad.sum() >= 20 and not ((ad == 1) & (at == 0)).any()
    assert n_t > n_d and np.median(got["n_inliers"]) > n_d, (n_t, n_d)
    col = 10 if ft else 0
    assert err(got, col) <= err(dense, col), (err(got, col), err(dense, col))


def test_4_priors_thirty_degrees_off(pkg, orc, scenes):
    """min_inliers = 30 loses every query.  With the default 6 the gate's inlier counts are the restatement's, match for match (the
    homography harness on the run's assembled queries), and the accepted set is the restatement's: those inliers solved by the
    oracle from the prior -- queries 5, 11 and 19 in the CPU experiment."""
    s = scenes[0]
    far = pkg.synth_reloc.perturb_cameras(s.sc.cam_gt, 30.0, 0.02, seed=0)
    kw = dict(landmarks=s.lmap, landmark_prior=dict(cams=far, radius_px=RADIUS), match=MATCH, **LM)
    got30 = s.rl.run(s.tests, s.sc.query_wh, min_inliers=30, **kw)
    assert not got30["accepted"].any() and np.isfinite(got30["cam"]).all()
    got = s.rl.run(s.tests, s.sc.query_wh, min_inliers=6, **kw)
    asm = s.rl.matches()
    harness = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "libhomography_harness.so"))
    _, found, mask = hc.run_per_pair(harness.h_find_homography, asm["match_ptr"], asm["uv_ref"], asm["uv_cur"], 4.0)
    ptr, keep = [0], np.zeros(len(mask), dtype=bool)
    for q in range(24):
        sl = slice(int(asm["match_ptr"][q]), int(asm["match_ptr"][q + 1]))
        if found[q] == 1 and mask[sl].sum() >= 6:
            keep[sl] = mask[sl] == 1
        ptr.append(ptr[-1] + int(keep[sl].sum()))
    ninl = np.diff(ptr).astype(np.int32)
    print("n_visible", got["n_visible"], "n_matches", got["n_matches"], "n_inliers", got["n_inliers"], "restated", ninl, "accepted", got["accepted"])
    assert np.array_equal(got["n_inliers"], ninl)
    # (the assembly's two cameras are no output of the run: the hand composition gives them)
    with pkg.api.landmark_visible(s.lmap, far, s.sc.query_wh, radius_px=RADIUS) as v:
        view = v.arrays()
        g = pkg.api.match_descriptors_guided(v.desc_set(), s.tests, np.arange(24), np.arange(24), np.tile(I9, (24, 1)), None, RADIUS, **MATCH)
    a = pkg.api.landmark_assemble(s.lmap, g["match_ptr"], _lift(view, g), g["uv_b"], s.sc.query_wh)
    cam_ref, cam_init = a["cam_ref"], pu.prior_camera(a["cam_init"], far, 0)
    b = types.SimpleNamespace(n_query=24, match_ptr=np.asarray(ptr, dtype=np.int64), uv_ref=asm["uv_ref"][keep], uv_cur=asm["uv_cur"][keep],
                              cam_ref=cam_ref, cam_init=cam_init, factor_type=0)
    acc = np.asarray(orc.krt_solve_batch(b)[2]) * (ninl > 0)
    assert np.array_equal(got["accepted"], acc) and np.nonzero(acc)[0].tolist() == [5, 11, 19], (got["accepted"], acc)


def test_5_the_other_runs_keep_their_bits_around_a_tracked_landmark_run(pkg, scenes):
    s = scenes[0]
    n = 6
    qp, qd, qk = s.qf
    cut = int(qp[n])
    kw = dict(max_refs=4, match=MATCH, **LM)
    wh = s.sc.query_wh[:n]
    with pkg.api.DescSet(qp[:n + 1], qd[:cut], qk[:cut]) as tests:
        runs = (lambda: s.rl.run(tests, wh, landmarks=s.lmap, match=MATCH, **LM),
                lambda: s.rl.run(tests, wh, prior=dict(cams=s.prior[:n], radius_px=RADIUS), **kw),
                lambda: s.rl.run(tests, wh, **kw),
                lambda: s.rl.run(tests, wh, landmarks=s.lmap, landmark_prior=dict(cams=s.prior[:n], radius_px=RADIUS), match=MATCH, **LM))
        before = [r() for r in runs]
        with pytest.raises(pkg.api.PtzError):  # a run that fails in between
            s.rl.run(tests, wh, landmarks=s.lmap, landmark_prior=dict(cams=s.prior[:n], radius_px=-1.0))
        after = [r() for r in runs]
        assert len(s.rl.view()["vis_ptr"]) == n + 1
        runs[2]()
        with pytest.raises(pkg.api.PtzError):  # an all-pairs run leaves no view
            s.rl.view()
    for x, y in zip(before, after):
        for key in PER_QUERY:
            assert _same(x[key], y[key]), key
    assert all(r["accepted"].all() for r in before)


def test_6_errors(pkg, scenes):
    api = pkg.api
    s = scenes[0]
    lpri = dict(cams=s.prior, radius_px=RADIUS)

    def code(fn):
        with pytest.raises(api.PtzError) as e:
            fn()
        return e.value.code

    with pytest.raises(ValueError):
        s.rl.run(s.tests, s.sc.query_wh, landmark_prior=lpri)                                  # landmark_prior without landmarks
    with pytest.raises(ValueError):
        s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, landmark_prior=dict(cams=s.prior[:5]))  # not one prior per query
    with pytest.raises(ValueError):
        s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, landmark_prior=lpri, prior=dict(cams=s.prior))
    L, o, r = api.lib(), api.RelocOptions(), api.RelocResult()
    L.ptz_reloc_options_default(C.byref(o))
    wh = np.ascontiguousarray(s.sc.query_wh, dtype=np.int32)
    assert L.ptz_relocalizer_run_landmarks_tracked(s.rl.handle, s.lmap.handle, s.tests.handle, 24, wh.ctypes.data_as(C.c_void_p), None, C.byref(o),
                                                   None, C.byref(r), None) == -1           # missing priors
    for rad in (0.0, -3.0, float("nan"), float("inf")):
        assert code(lambda: s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, landmark_prior=dict(cams=s.prior, radius_px=rad))) == -1
    assert code(lambda: s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, landmark_prior=dict(cams=s.prior, max_view_bytes=1 << 16))) == -5
    bad = s.prior.copy()
    bad[2, 4] = np.nan
    assert code(lambda: s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, landmark_prior=dict(cams=bad))) == -1
    rp = np.array([0, 3], dtype=np.int64)
    with api.DescSet(rp, np.zeros((3, 64), np.uint8), np.zeros((3, 2), np.float32)) as d64:  # another D than the map's
        assert code(lambda: s.rl.run(d64, s.sc.query_wh[:1], landmarks=s.lmap, landmark_prior=dict(cams=s.prior[:1]))) == -1
    with api.DescSet(rp, np.zeros((3, 128), np.uint8), np.zeros((3, 2), np.float32)) as one, api.Relocalizer(one, s.rig[:1]) as small:
        assert code(lambda: small.run(s.tests, s.sc.query_wh, landmarks=s.lmap, landmark_prior=lpri)) == -1  # a map of another reference count
    ok = s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, landmark_prior=lpri, guided_radius=4.0, match=MATCH, **LM)  # guided_radius is ignored
    assert ok["accepted"].all()
