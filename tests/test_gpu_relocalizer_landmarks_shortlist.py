"""GPU tests of relocalization against the landmark map through a probe-vote shortlist
(ptz_relocalizer_run_landmarks_shortlisted, api.Relocalizer.run(landmarks=, landmark_shortlist=)) on the data set of
test_gpu_relocalizer_landmarks.py: the 20-view rig make_scene(0, 20, 100), make_reloc_scene(n_query=24, n_feat=600,
visible_share=0.5, noise_px=0.5, seed=0), make_reloc_descriptors(D=128, noise=12, n_distractors=50, seed=0), the tracks of
synth_reloc.scene_tracks(sc, 50); the matcher runs with min_matches = 8, the vote pass with M = 256 probes.

THE CPU EXPERIMENT behind R and the accuracy test, before any device run (tools/probes/probe_landmark_shortlist_accuracy_cpu.py,
figures in profiles/landmark_shortlist_accuracy_cpu.json): the numpy map, the restated votes, lists and view
(landmark_shortlist_util), the numpy matcher on (view q, query q), the numpy landmark assembly and the ORACLE's krt_solve_batch,
seeds 0 .. 5, F and FDist, R in {2, 4, 6, 8, 12, 20}.  24 of 24 queries are accepted in every row.  The rule -- the smallest R with
24 of 24 on all six seeds and a median focal error (F) and k1 error (FDist) below the K = 1 image run's on seed 0 and on at least
five of six seeds -- is evaluated by the probe and its answer recorded as chosen_R; the tests read R and the seed-0 medians from
that file.  The answer is R = 6: R = 2 loses to K = 1 in 7 of the 12 rows and R = 4 in seeds 3 and 5 of F (6.12e-5 against 4.56e-5,
3.48e-5 against 3.45e-5), while R = 6 wins all 12.  Median error, K = 1 / dense landmarks / R = 6:
      F (relative focal)   seed 0: 7.37e-5 2.91e-5 3.70e-5   1: 7.07e-5 3.30e-5 3.91e-5   2: 6.92e-5 4.31e-5 4.20e-5
                                3: 4.56e-5 3.96e-5 4.01e-5   4: 6.35e-5 3.95e-5 3.93e-5   5: 3.45e-5 2.81e-5 2.83e-5
      FDist (k1)           seed 0: 2.02e-3 6.44e-4 5.90e-4   1: 1.49e-3 4.61e-4 6.69e-4   2: 1.10e-3 5.57e-4 5.83e-4
                                3: 1.96e-3 6.90e-4 7.93e-4   4: 1.44e-3 7.27e-4 6.29e-4   5: 1.24e-3 9.11e-4 8.86e-4
On this rig a query's probes give at least 4 of the 20 homes a vote, 10 at the median; with R = 6 a query is matched against 3 907
to 5 083 of some 12 500 landmarks (median over its 24 queries) and keeps 86 to 92 % of the dense run's matches (R = 2: 42 to 51 %,
R = 4: 71 to 78 %, R = 8: 94 to 98 %, R = 12: 99 %).

THE WHOLE-MAP SCENE (test_2): the rig's first TWO views (pans -59.7 and -54.0 degrees), make_reloc_scene seed 0, descriptor seed 0,
M = 256.  Checked on the CPU with the restatement: each of the 24 queries gives both homes a vote (at least 30 of its 256 probes
vote for its weaker home), so max_refs = n_ref, min_votes = 1 lists every non-empty home for 24 of 24 queries.  With three or more
views of this rig some query always looks away from one of them (the restatement finds 20 to 23 of 24), and on the 20-view rig a
query's probes reach half of the homes: no scene of the accuracy table has the property, so this one was made for it."""
import ctypes as C
import json
import math
import os
import types

import numpy as np
import pytest

import landmark_shortlist_util as lsu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM = dict(max_num_iterations=200)
TRIM = dict(trim_px=2.0, k_sigma=3.0, max_rounds=8, min_keep=8)
MATCH = dict(min_matches=8)
M = 256
PER_QUERY = ("cam", "accepted", "summaries", "sel_ref", "n_sel", "n_matches", "n_inliers", "trim_report", "cov", "sigma0", "cov_status")

with open(os.path.join(ROOT, "profiles", "landmark_shortlist_accuracy_cpu.json")) as _f:
    PROBE = json.load(_f)
assert PROBE["n_probes"] == M
R = PROBE["chosen_R"]


def _same(x, y):
    if x is None or y is None:
        return x is None and y is None
    if isinstance(x, (list, tuple)):
        return len(x) == len(y) and all(_same(u, v) for u, v in zip(x, y))
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(_same(x[k], y[k]) for k in x)
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


def _scene(pkg, rig, ft):
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=24, n_feat=600, visible_share=0.5, noise_px=0.5, factor_type=ft, seed=0)
    rf, qf = pkg.synth_reloc.make_reloc_descriptors(sc, D=128, noise=12, n_distractors=50, seed=0)
    tp, ti, tf, _ = pkg.synth_reloc.scene_tracks(sc, 50)
    refs, tests = pkg.api.DescSet(*rf), pkg.api.DescSet(*qf)
    lmap = pkg.api.LandmarkMap(refs, rig, tp, ti, tf, factor_type=ft)
    return types.SimpleNamespace(sc=sc, rig=rig, refs=refs, tests=tests, qf=qf, lmap=lmap, rl=pkg.api.Relocalizer(refs, rig))


@pytest.fixture(scope="module")
def scenes(pkg):
    """per factor type: the scene, the resident sets, the map, the relocalizer (shared: the tests only run them); "two": the
    whole-map scene"""
    out = {}
    full = pkg.synth.make_scene(0, 20, 100).cam_gt.copy()
    for ft in (0, 1):
        rig = full.copy()
        if ft:
            rig[:, 10] = np.random.default_rng(100).uniform(-0.05, 0.05, len(rig))
        out[ft] = _scene(pkg, rig, ft)
    out["two"] = _scene(pkg, full[:2].copy(), 0)
    yield out
    for s in out.values():
        s.rl.close(); s.lmap.close(); s.tests.close(); s.refs.close()


@pytest.fixture(scope="module")
def expected(pkg, scenes):
    """the hand composition of the public calls, once per factor type"""
    api = pkg.api
    out = {}
    for ft in (0, 1):
        s = scenes[ft]
        nq = s.sc.n_query
        ia = np.arange(nq, dtype=np.int32)
        sl = api.landmark_shortlist(s.lmap, s.tests, max_refs=R, n_probes=M, min_votes=1, **MATCH)
        with api.landmark_view_from_homes(s.lmap, sl["shortlist"]) as v:
            view = v.arrays()
            t = api.match_descriptors(v.desc_set(), s.tests, ia, ia, **MATCH)
        asm = api.landmark_assemble(s.lmap, t["match_ptr"], lsu.lift(view, t), t["uv_b"], s.sc.query_wh)
        b = types.SimpleNamespace(n_query=nq, match_ptr=asm["match_ptr"], uv_ref=asm["uv_ref"], uv_cur=asm["uv_cur"], cam_ref=asm["cam_ref"],
                                  cam_init=asm["cam_init"], factor_type=ft)
        e = dict(sl=sl, view=view, table=t, asm=asm, n_matches=np.diff(asm["match_ptr"]).astype(np.int32))
        cam, summ, acc, _ = api.krt_solve_batch(b, **LM)
        e["plain"] = dict(cam=cam, summaries=summ, accepted=acc, n_inliers=e["n_matches"], trim_report=None,
                          cov=api.krt_covariance_batch(b, cam, accepted=acc)[:3])
        cam, summ, acc, ninl, gmask, _, _ = api.krt_solve_batch_gated(b, ransac_thresh=4.0, min_inliers=6, **LM)
        e["gated"] = dict(cam=cam, summaries=summ, accepted=acc, n_inliers=ninl, trim_report=None,
                          cov=api.krt_covariance_batch(b, cam, match_mask=gmask, accepted=acc)[:3])
        cam, summ, acc, kept, rep, _ = api.krt_solve_batch_trimmed(b, **TRIM, **LM)
        e["trimmed"] = dict(cam=cam, summaries=summ, accepted=acc, n_inliers=e["n_matches"], trim_report=rep,
                            cov=api.krt_covariance_batch(b, cam, match_mask=kept, accepted=acc)[:3])
        cam, summ, acc, kept, rep, _ = api.krt_solve_batch_trimmed(b, match_mask=gmask, **TRIM, **LM)
        e["gated_trimmed"] = dict(cam=cam, summaries=summ, accepted=acc, n_inliers=ninl, trim_report=rep,
                                  cov=api.krt_covariance_batch(b, cam, match_mask=kept, accepted=acc)[:3])
        out[ft] = e
    return out


def _run(s, ft, variant="plain", **kw):
    kw.setdefault("landmark_shortlist", dict(max_refs=R, n_probes=M, min_votes=1))
    return s.rl.run(s.tests, s.sc.query_wh, factor_type=ft, landmarks=s.lmap, inlier_matches="gated" in variant,
                    trim=TRIM if "trimmed" in variant else None, uncertainty=True, match=MATCH, **LM, **kw)


def test_0_the_probe_chose_an_R():
    """the rule of the module's docstring has an answer in the table (were there none, the tests below would assert the acceptance
    count only and the README would say so)"""
    assert R in PROBE["table_R"], R


@pytest.mark.parametrize("ft", [0, 1])
@pytest.mark.parametrize("variant", ["plain", "gated", "trimmed", "gated_trimmed"])
def test_1_run_is_bit_equal_to_the_hand_composition(pkg, scenes, expected, ft, variant):
    """landmark_shortlist -> landmark_view_from_homes -> match_descriptors -> the lift in numpy -> landmark_assemble ->
    krt_solve_batch / _gated / _trimmed -> krt_covariance_batch: the lists, the view, the table and every per-query output"""
    s, e = scenes[ft], expected[ft]
    want = e[variant]
    got = _run(s, ft, variant)
    view, table, asm = s.rl.view(), s.rl.table(), s.rl.matches()
    for key in ("shortlist", "n_short", "votes"):
        assert np.array_equal(got[key], e["sl"][key]), key
    assert (got["n_short"] > 0).all() and got["votes_ms"] > 0 and got["view_ms"] > 0
    lsu.assert_equal(view, e["view"], (ft, "view"))
    assert not view["vis_uv"].any()
    assert np.array_equal(got["n_visible"], np.diff(e["view"]["vis_ptr"])) and 500 < got["n_visible"].min() and got["n_visible"].max() < s.lmap.n_landmarks
    for key in ("match_ptr", "idx_a", "idx_b", "dist2", "uv_b"):
        assert np.array_equal(table[key], e["table"][key]), key
    assert np.array_equal(s.rl.pairs()["pair_ref"], np.arange(24))
    for key in ("match_ptr", "uv_ref", "uv_cur", "src"):
        assert np.array_equal(asm[key], e["asm"][key]), key
    assert got["sel_ref"].shape == (24, 1) and np.array_equal(got["sel_ref"][:, 0], e["asm"]["anchor_ref"]) and (got["n_sel"] == 1).all()
    assert np.array_equal(got["n_matches"], e["n_matches"]) and e["n_matches"].min() >= 100
    for key in ("cam", "accepted", "summaries", "n_inliers", "trim_report"):
        assert _same(got[key], want[key]), (ft, variant, key)
    cov, s0, status = want["cov"]
    ok = status == pkg.api.COV_OK
    assert np.array_equal(got["cov_status"], status) and ok.sum() >= 20
    assert np.array_equal(got["cov"][ok], cov[ok]) and np.array_equal(got["sigma0"][ok], s0[ok])
    assert want["accepted"].sum() >= 20 and (got["stage_ms"][[0, 2, 4, 5]] > 0).all() and got["stage_ms"][1] == 0


def test_2_every_home_listed_is_the_dense_landmark_run(pkg, scenes):
    """The whole-map scene of the module's docstring (two views, seed 0, M = 256): the RESTATEMENT gives every non-empty home a
    vote for 24 of 24 queries, the device lists are the restated ones, and with max_refs = n_ref, min_votes = 1 the run equals
    ptz_relocalizer_run_landmarks bit for bit, plain and gated + trimmed with covariance"""
    s = scenes["two"]
    lm = s.lmap.arrays()
    qp, qd, _ = s.qf
    n_ref = len(s.rig)
    want = lsu.shortlist(lm["lm_desc"], lm["lm_home"], n_ref, qd, qp, max_refs=n_ref, n_probes=M, min_votes=1)
    non_empty = np.unique(lm["lm_home"])
    voted = (want["votes"][:, non_empty] > 0).all(axis=1)
    assert len(non_empty) == n_ref == 2 and voted.sum() == 24, (non_empty, np.nonzero(~voted)[0])
    assert want["votes"].min() >= 30
    for variant in ("plain", "gated_trimmed"):
        got = _run(s, 0, variant, landmark_shortlist=dict(max_refs=n_ref, n_probes=M, min_votes=1))
        view, table = s.rl.view(), s.rl.table()
        for key in ("shortlist", "n_short", "votes"):
            assert np.array_equal(got[key], want[key]), key
        assert np.array_equal(view["vis_lm"], np.tile(np.arange(s.lmap.n_landmarks, dtype=np.int32), 24))
        dense = s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, inlier_matches="gated" in variant, trim=TRIM if "trimmed" in variant else None,
                         uncertainty=True, match=MATCH, **LM)
        dtable = s.rl.table()
        for key in ("match_ptr", "idx_a", "idx_b", "dist2", "uv_b"):  # the whole map in order: view-local IS the landmark index
            assert np.array_equal(table[key], dtable[key]), key
        for key in PER_QUERY:
            assert _same(got[key], dense[key]), (variant, key)
        assert dense["accepted"].all()


def _digits(x):
    """one unit of the third significant digit of x: what the probe's JSON records"""
    return 10.0 ** (math.floor(math.log10(abs(x))) - 2)


@pytest.mark.parametrize("ft", [0, 1])
def test_3_accuracy_at_the_probes_R(pkg, scenes, ft):
    """Seed 0, against the K = 1 run (the reference image with the most matches) of the same relocalizer on the same descriptors:
    24 of 24 queries accepted; the median relative focal error (F) or k1 error (FDist) is below K = 1's; and both medians are the
    probe's seed-0 figures to the three digits the JSON records (one unit of the last digit: the device solve and the oracle's
    agree to about 1e-8, and a figure may sit on a rounding edge).  The probe's figures come from the restatement and the oracle."""
    s = scenes[ft]
    rec = [r for r in PROBE["records"] if r["seed"] == 0 and r["factor_type"] == ft][0]["shortlist"][str(R)]
    one = s.rl.run(s.tests, s.sc.query_wh, factor_type=ft, max_refs=1, match=MATCH, **LM)
    got = s.rl.run(s.tests, s.sc.query_wh, factor_type=ft, landmarks=s.lmap, landmark_shortlist=dict(max_refs=R, n_probes=M, min_votes=1), match=MATCH,
                   **LM)
    col = 10 if ft else 0
    gt = s.sc.cam_gt
    err = lambda r: float(np.median(np.abs(r["cam"][:, col] - gt[:, col]) / (gt[:, col] if col == 0 else 1.0)))
    e1, eg = err(one), err(got)
    print(f"factor {ft}, R {R}: accepted {int(got['accepted'].sum())}, matches {np.median(one['n_matches']):.0f} -> {np.median(got['n_matches']):.0f}, "
          f"visible {np.median(got['n_visible']):.0f} of {s.lmap.n_landmarks}, median error K = 1 {e1:.3e} shortlisted {eg:.3e}; probe {rec['median_err_K1']:.2e} "
          f"{rec['median_err']:.2e}; stage ms {got['stage_ms'].round(3)} votes {got['votes_ms']:.3f} view {got['view_ms']:.3f}")
    assert got["accepted"].sum() == 24 and one["accepted"].sum() == 24 and rec["accepted"] == 24
    assert eg < e1, (eg, e1)
    assert abs(eg - rec["median_err"]) <= _digits(rec["median_err"]), (eg, rec["median_err"])
    assert abs(e1 - rec["median_err_K1"]) <= _digits(rec["median_err_K1"]), (e1, rec["median_err_K1"])
    assert np.median(got["n_visible"]) == rec["median_view"] and np.median(got["n_matches"]) == rec["median_matches"]


def test_4_a_query_without_a_list_and_the_other_runs_keep_their_bits(pkg, scenes):
    """min_votes above the probe budget: no home ranks, every view is empty, every query goes on with n_sel = 0 and is not
    accepted; the runs around it return what they returned before"""
    s = scenes[0]
    before = _run(s, 0), s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, match=MATCH, **LM)
    none = _run(s, 0, landmark_shortlist=dict(max_refs=R, n_probes=M, min_votes=M + 1))
    assert (none["n_short"] == 0).all() and (none["shortlist"] == -1).all() and (none["n_visible"] == 0).all()
    assert (none["n_sel"] == 0).all() and (none["sel_ref"] == -1).all() and (none["n_matches"] == 0).all() and np.isfinite(none["cam"]).all()
    assert s.rl.view()["vis_ptr"].tolist() == [0] * 25
    after = _run(s, 0), s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, match=MATCH, **LM)
    with pytest.raises(pkg.api.PtzError):  # a dense landmark run leaves no view
        s.rl.view()
    for x, y in zip(before, after):
        for key in PER_QUERY:
            assert _same(x[key], y[key]), key


def test_5_errors(pkg, scenes):
    api = pkg.api
    s = scenes[0]
    sl = dict(max_refs=R, n_probes=M)
    with pytest.raises(api.PtzError) as e:
        s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, landmark_shortlist=sl, guided_radius=4.0, match=MATCH)
    assert e.value.code == -4  # PTZ_EUNSUPPORTED
    with pytest.raises(ValueError):
        s.rl.run(s.tests, s.sc.query_wh, landmark_shortlist=sl)  # without landmarks=
    with pytest.raises(ValueError):
        s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, landmark_shortlist=sl, landmark_prior=dict(cams=s.sc.cam_gt))
    with pytest.raises(ValueError):
        s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, landmark_shortlist=sl, shortlist={})
    with pytest.raises(ValueError):
        s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, landmark_shortlist=sl, prior=dict(cams=s.sc.cam_gt))
    with pytest.raises(ValueError):  # the existing exclusion stands
        s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, shortlist={})
    for bad in (dict(max_refs=0), dict(n_probes=0), dict(min_votes=-1)):
        with pytest.raises(api.PtzError) as e:
            s.rl.run(s.tests, s.sc.query_wh, landmarks=s.lmap, landmark_shortlist=bad, match=MATCH)
        assert e.value.code == -1, bad
    L, o, r = api.lib(), api.RelocOptions(), api.RelocResult()
    L.ptz_reloc_options_default(C.byref(o))
    wh = np.ascontiguousarray(s.sc.query_wh, dtype=np.int32)
    assert L.ptz_relocalizer_run_landmarks_shortlisted(s.rl.handle, None, s.tests.handle, 24, wh.ctypes.data_as(C.c_void_p), C.byref(o), None, C.byref(r),
                                                       None, None) == -1  # no map
    with api.DescSet(np.array([0, 3]), np.zeros((3, 64), np.uint8), np.zeros((3, 2), np.float32)) as d64:  # another D than the map's
        with pytest.raises(api.PtzError) as e:
            s.rl.run(d64, s.sc.query_wh[:1], landmarks=s.lmap, landmark_shortlist=sl)
        assert e.value.code == -1
