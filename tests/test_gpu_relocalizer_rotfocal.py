"""GPU tests of the rotation-and-focal gate as stage 4 of the resident serving loop (ptz_relocalizer_set_gate_model(r, 1, iters),
api.Relocalizer.run(gate_model=1)): every per-query output is bit-equal to the composition by hand of the public calls on the run's own
match table -- reloc_assemble / landmark_assemble -> RotFocalGate.run -> krt_solve_batch on the gate's compacted CSR (or
krt_solve_batch_trimmed with the gate's kept set as its universe) -> krt_covariance_batch -- on the 24-query data sets the other
relocalizer tests use: desc_guided_util.repeated_reloc for the image run (K = 1 and K = 4), the tracked landmark data set of
test_gpu_relocalizer_landmarks_prior.py for the tracked landmark run.  With gate_model = 0 a run returns what it returns without the
argument."""
import types

import numpy as np
import pytest

import desc_guided_util as gu
import reloc_prior_util as pu

pytestmark = pytest.mark.gpu

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


def by_hand(api, asm, cam_init, ft, trimmed, tracked, iters=128, min_inliers=6):
    """the gate and everything behind it, from the assembly's outputs"""
    ptr = asm["match_ptr"]
    nq = len(ptr) - 1
    with api.RotFocalGate(nq, len(asm["uv_ref"])) as gate:
        g = gate.run(ptr, asm["uv_ref"], asm["uv_cur"], asm["cam_ref"], cam_init, thresh=4.0, min_inliers=min_inliers, iters=iters)
    ninl = np.diff(g["out_ptr"]).astype(np.int32)
    gmask = (g["mask"] * np.repeat(ninl > 0, np.diff(ptr))).astype(np.uint8)  # zero for a query that does not pass
    full = types.SimpleNamespace(n_query=nq, match_ptr=ptr, uv_ref=asm["uv_ref"], uv_cur=asm["uv_cur"], cam_ref=asm["cam_ref"], cam_init=cam_init,
                                 factor_type=ft)
    rep = None
    if trimmed:
        cam, summ, acc, kept, rep, _ = api.krt_solve_batch_trimmed(full, match_mask=gmask, **TRIM, **LM)
    else:
        kept = gmask
        cam, summ, acc, _ = api.krt_solve_batch(types.SimpleNamespace(n_query=nq, match_ptr=g["out_ptr"], uv_ref=g["out_uv_a"], uv_cur=g["out_uv_b"],
                                                                      cam_ref=asm["cam_ref"], cam_init=cam_init, factor_type=ft), **LM)
    if tracked:
        acc = acc * (ninl > 0)  # a query the gate kept nothing of is not accepted
    return dict(cam=cam, summaries=summ, accepted=acc, n_inliers=ninl, trim_report=rep, gate=g,
                cov=api.krt_covariance_batch(full, cam, match_mask=kept, accepted=acc)[:3])


def check(api, got, want, models, least=20):
    for key in ("cam", "accepted", "summaries", "n_inliers", "trim_report"):
        assert _same(got[key], want[key]), key
    cov, s0, status = want["cov"]
    ok = status == api.COV_OK
    assert np.array_equal(got["cov_status"], status) and ok.sum() >= least
    assert np.array_equal(got["cov"][ok], cov[ok]) and np.array_equal(got["sigma0"][ok], s0[ok])
    g = want["gate"]
    assert np.array_equal(models["found"], g["found"]) and np.array_equal(models["model"], g["model"])  # (zeros where found != 1, both)
    assert want["accepted"].sum() >= least and got["stage_ms"][3] > 0


# ---- the image run -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def image_data(pkg, tmp_path_factory):
    rb, (rp, rd, rk), (qp, qd, qk), _ = gu.repeated_reloc(pkg, str(tmp_path_factory.mktemp("relocalizer_rotfocal")))
    refs, tests = pkg.api.DescSet(rp, rd, rk), pkg.api.DescSet(qp, qd, qk)
    rl = pkg.api.Relocalizer(refs, rb.cam_ref)
    yield types.SimpleNamespace(rb=rb, refs=refs, tests=tests, rl=rl, wh=np.tile(np.array([1920, 1080], dtype=np.int32), (rb.n_query, 1)))
    rl.close(); tests.close(); refs.close()


@pytest.mark.parametrize("variant", ["gated", "gated_trimmed"])
@pytest.mark.parametrize("K", [1, 4])
def test_image_run_is_bit_equal_to_the_hand_composition(pkg, image_data, K, variant):
    api, d = pkg.api, image_data
    got = d.rl.run(d.tests, d.wh, max_refs=K, inlier_matches=1, gate_model=1, trim=TRIM if "trimmed" in variant else None, uncertainty=True,
                   match=MATCH, **LM)
    m, pairs, mine, models = d.rl.table(), d.rl.pairs(), d.rl.matches(), d.rl.gate_models()
    asm = api.reloc_assemble(m["match_ptr"], m["uv_a"], m["uv_b"], pairs["pair_ref"], pairs["query_ptr"], d.rb.cam_ref, d.wh, factor_type=0, max_refs=K)
    for key in ("match_ptr", "uv_ref", "uv_cur", "src"):
        assert np.array_equal(mine[key], asm[key]), key
    want = by_hand(api, asm, asm["cam_init"], 0, "trimmed" in variant, tracked=False)
    check(api, got, want, models, least=20 if K == 1 else 1)  # (K = 1: the count the existing K = 1 test asserts for the homography gate)
    print("K", K, variant, "accepted", int(want["accepted"].sum()), "n_sel", asm["n_sel"].tolist(), "kept", want["n_inliers"].tolist())
    assert np.array_equal(got["n_sel"], asm["n_sel"])
    if K == 4:  # the virtual anchor
        assert (asm["cam_ref"][:, 2] == 8192.0).all() and (asm["cam_ref"][:, 3] == 8192.0).all()


def test_k4_with_several_views_per_query(pkg):
    """the repeated-texture data set gives every query one usable reference; on the 6-query scene of
    test_k4_is_the_assembly_and_the_solve_on_the_downloaded_table every query has at least two, so the gate sees matches of several
    references transferred into the virtual anchor"""
    api = pkg.api
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=6, n_feat=200, seed=3)
    (rp, rd, rk), (qp, qd, qk) = pkg.synth_reloc.make_reloc_descriptors(sc, D=64, noise=8, n_distractors=20, seed=1)
    with api.DescSet(rp, rd, rk) as refs, api.DescSet(qp, qd, qk) as tests, api.Relocalizer(refs, rig) as rl:
        got = rl.run(tests, sc.query_wh, max_refs=4, inlier_matches=1, gate_model=1, uncertainty=True, match=MATCH, **LM)
        m, pairs, mine, models = rl.table(), rl.pairs(), rl.matches(), rl.gate_models()
    asm = api.reloc_assemble(m["match_ptr"], m["uv_a"], m["uv_b"], pairs["pair_ref"], pairs["query_ptr"], rig, sc.query_wh, factor_type=0, max_refs=4)
    for key in ("match_ptr", "uv_ref", "uv_cur", "src"):
        assert np.array_equal(mine[key], asm[key]), key
    want = by_hand(api, asm, asm["cam_init"], 0, False, tracked=False)
    check(api, got, want, models, least=6)
    ferr = np.abs(got["cam"][:, 0] - sc.cam_gt[:, 0]) / sc.cam_gt[:, 0]
    print("n_sel", asm["n_sel"].tolist(), "assembled", np.diff(asm["match_ptr"]).tolist(), "kept", want["n_inliers"].tolist(), "focal error", ferr)
    assert (asm["n_sel"] >= 2).all() and want["accepted"].all() and ferr.max() < 5e-3  # (what the ungated K = 4 test states of this scene)


def test_gate_model_0_is_the_run_without_the_argument(pkg, image_data):
    d = image_data
    for kw in (dict(max_refs=1, inlier_matches=1), dict(max_refs=4, inlier_matches=1, trim=TRIM), dict(max_refs=4)):
        a = d.rl.run(d.tests, d.wh, uncertainty=True, match=MATCH, **kw, **LM)
        b = d.rl.run(d.tests, d.wh, uncertainty=True, match=MATCH, gate_model=0, gate_iters=77, **kw, **LM)
        for key in PER_QUERY:
            assert _same(a[key], b[key]), key
        with pytest.raises(pkg.api.PtzError, match="PTZ_EINVAL"):  # a homography run leaves no models
            d.rl.gate_models()
    for bad in (dict(gate_model=2), dict(gate_model=-1), dict(gate_model=1, gate_iters=0), dict(gate_model=1, gate_iters=4097)):
        with pytest.raises(pkg.api.PtzError, match="PTZ_EINVAL"):
            d.rl.run(d.tests, d.wh, inlier_matches=1, match=MATCH, **bad, **LM)


# ---- the tracked landmark run -------------------------------------------------------------------------------------------------------------
def _landmark_scene(pkg, ft):
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt.copy()
    if ft:
        rig[:, 10] = np.random.default_rng(100).uniform(-0.05, 0.05, len(rig))
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=24, n_feat=600, visible_share=0.5, noise_px=0.5, factor_type=ft, seed=0)
    rf, qf = pkg.synth_reloc.make_reloc_descriptors(sc, D=128, noise=12, n_distractors=50, seed=0, repeat_share=0.7, repeat_group=4, repeat_noise=6)
    tp, ti, tf, _ = pkg.synth_reloc.scene_tracks(sc, 50)
    refs, tests = pkg.api.DescSet(*rf), pkg.api.DescSet(*qf)
    lmap = pkg.api.LandmarkMap(refs, rig, tp, ti, tf, factor_type=ft)
    return types.SimpleNamespace(sc=sc, rig=rig, refs=refs, tests=tests, lmap=lmap, rl=pkg.api.Relocalizer(refs, rig),
                                 prior=pkg.synth_reloc.perturb_cameras(sc.cam_gt, 0.3, 0.02, seed=0))


@pytest.fixture(scope="module")
def landmark_scenes(pkg):
    out = {ft: _landmark_scene(pkg, ft) for ft in (0, 1)}
    yield out
    for s in out.values():
        s.rl.close(); s.lmap.close(); s.tests.close(); s.refs.close()


@pytest.fixture(scope="module")
def landmark_data(landmark_scenes):
    return landmark_scenes[0]


@pytest.mark.parametrize("variant", ["gated", "gated_trimmed"])
def test_tracked_landmark_run_is_bit_equal_to_the_hand_composition(pkg, landmark_data, variant):
    """inlier_matches is left off: the tracked run forces the gate on, whichever model it is"""
    api, s = pkg.api, landmark_data
    got = s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, landmark_prior=dict(cams=s.prior, radius_px=RADIUS), gate_model=1,
                   trim=TRIM if "trimmed" in variant else None, uncertainty=True, match=MATCH, **LM)
    view, g, mine, models = s.rl.view(), s.rl.table(), s.rl.matches(), s.rl.gate_models()
    pair_of = np.repeat(np.arange(24), np.diff(g["match_ptr"]))
    lifted = view["vis_lm"][view["vis_ptr"][pair_of] + g["idx_a"]].astype(np.int32)
    asm = api.landmark_assemble(s.lmap, g["match_ptr"], lifted, g["uv_b"], s.sc.query_wh)
    for key in ("match_ptr", "uv_ref", "uv_cur", "src"):
        assert np.array_equal(mine[key], asm[key]), key
    want = by_hand(api, asm, pu.prior_camera(asm["cam_init"], s.prior, 0), 0, "trimmed" in variant, tracked=True)
    check(api, got, want, models)
    assert want["accepted"].all() and np.diff(asm["match_ptr"]).min() >= 100
    # the same run under the homography gate: another gate, the same data, every query accepted by both
    old = s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, landmark_prior=dict(cams=s.prior, radius_px=RADIUS), match=MATCH, **LM)
    gt = s.sc.cam_gt[:, 0]
    print("median relative focal error: rotation-and-focal gate %.3e, homography gate %.3e; kept per query (median) %d and %d of %d"
          % (np.median(np.abs(got["cam"][:, 0] - gt) / gt), np.median(np.abs(old["cam"][:, 0] - gt) / gt), np.median(got["n_inliers"]),
             np.median(old["n_inliers"]), np.median(got["n_matches"])))
    assert old["accepted"].all()


@pytest.mark.parametrize("ft", [0, 1])
def test_accuracy_of_the_tracked_landmark_run_under_the_new_gate(pkg, landmark_scenes, ft):
    """Seed 0 of the data set, F and FDist.  The CPU experiment came first (tools/probes/probe_rotfocal_gate_accuracy_cpu.py: the numpy
    gate in the pipeline of probe_landmark_prior_accuracy_cpu.py, the oracle's solve; profiles/rotfocal_gate_accuracy_cpu.json): 24
    of 24 accepted in every row of seeds 0 .. 5, and the median error of prior + gate below the dense landmark run's in 12 of 12 rows
    (ratios F 0.92 0.53 0.54 0.86 0.69 0.33, FDist k1 0.53 0.30 0.44 0.75 0.49 0.61).  The device run accepts 24 of 24, reproduces the
    seed-0 medians to the three digits of the JSON, and its median error (relative focal for F, k1 for FDist) is below the dense
    landmark run's -- the statement test_3_a_prior_beats_the_dense_landmark_run makes for the homography gate."""
    import json
    import os
    s = landmark_scenes[ft]
    recs = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rotfocal_gate_accuracy_cpu.json")))
    rec = next(r for r in recs if r["seed"] == 0 and r["factor_type"] == ft)
    dense = s.rl.run(s.tests, s.sc.query_wh, factor_type=ft, landmarks=s.lmap, match=MATCH, **LM)
    got = s.rl.run(s.tests, s.sc.query_wh, factor_type=ft, landmarks=s.lmap, landmark_prior=dict(cams=s.prior, radius_px=RADIUS), guided_grid=True,
                   gate_model=1, match=MATCH, **LM)
    gt = s.sc.cam_gt
    both = (dense["accepted"] == 1) & (got["accepted"] == 1)
    focal = lambda r: float(np.median(np.abs(r["cam"][both, 0] - gt[both, 0]) / gt[both, 0]))
    k1 = lambda r: float(np.median(np.abs(r["cam"][both, 10] - gt[both, 10])))
    print("factor %d: accepted %d, focal %.3e (CPU %.3e, dense %.3e), k1 %.3e (CPU %.3e, dense %.3e)"
          % (ft, int(got["accepted"].sum()), focal(got), rec["prior_gate6"]["median_focal_err"], focal(dense), k1(got), rec["prior_gate6"]["median_k1_err"],
             k1(dense)))
    assert got["accepted"].sum() == 24 and rec["prior_gate6"]["accepted"] == 24
    assert "%.2e" % focal(got) == "%.2e" % rec["prior_gate6"]["median_focal_err"]
    if ft:
        assert "%.2e" % k1(got) == "%.2e" % rec["prior_gate6"]["median_k1_err"]
    err = k1 if ft else focal
    assert err(got) < err(dense), (err(got), err(dense))
