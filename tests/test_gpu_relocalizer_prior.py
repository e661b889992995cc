"""GPU tests of relocalization from a prior camera (ptz_relocalizer_run_tracked, api.Relocalizer.run(prior=...)) on the rig and scene
of test_four_references_beat_one_on_the_same_data -- the 20-view rig make_scene(0, 20, 100), make_reloc_scene(n_query=24,
n_feat=600, visible_share=0.5, noise_px=0.5, seed=0) -- with REPEATED texture: make_reloc_descriptors(D=128, noise=12,
n_distractors=50, seed=0, repeat_share=0.7, repeat_group=4, repeat_noise=6).  Priors: perturb_cameras(cam_gt, 0.3 degrees, 2 %,
seed=0).  Prior options: radius 40 px, R = 8, min_overlap 8; the matcher runs with min_matches = 8 as in test_gpu_relocalizer.py.

THE CPU EXPERIMENT behind test (c), before any device run: the numpy restatements alone (desc_match_util.match_pairs for the
all-pairs table, reloc_prior_util + desc_guided_util.match_pairs_guided for the prior path, reloc_assemble_util, the host homography
harness with 4 px and min_inliers 6 as the gate on the assembled query) and the ORACLE's krt_solve_batch, scene and perturbation seeds
0 .. 5, descriptor seed 0.  24 of 24 queries accepted in every row of every seed; the four references with the most true matches were
on the overlap list of every query but one (FDist, seed 4).  Seed 0, F:

                                   matches (of 26 549 true)  wrong   median matches / query K=1 / K=4   median rel. focal error K=1 / K=4
    all pairs (dense)                     7 948                0            76 / 213.5                    1.14e-4 / 8.62e-5
    prior, no gate                       24 704              914           247 / 714.5                    9.00e-4 / 9.88e-4
    prior + gate on the assembled query  same table   (dropped by it)      247 / 714.5 (241.5 / 679 kept) 7.26e-5 / 3.73e-5

Ratios prior + gate / all pairs, seeds 0 .. 5 (below 1: the prior path is the more accurate):
    F     focal, K = 1:  0.64 0.41 0.59 0.51 0.87 0.44        K = 4:  0.43 0.43 0.96 0.73 0.38 0.45
    FDist k1,    K = 1:  0.78 0.59 0.42 0.80 0.54 0.63        K = 4:  0.68 0.50 0.52 1.29 0.54 0.56
    (FDist seed 0: k1 2.87e-3 -> 2.24e-3 at K = 1, 1.83e-3 -> 1.25e-3 at K = 4)
The match count at least triples in every run.  So the accuracy assertion holds for 6 of 6 seeds but FDist, K = 4, where it holds for
5 of 6 (seed 3 is above 1: with 24 queries a median is noisy); the tests use seed 0, for which all four hold -- a statement about that
data set, not about every draw.  The lone-candidate finding shows in the middle row: without the gate the prior path is ten times
WORSE than the dense one.

THE EXPERIMENT behind test (d), same data, priors 30 degrees off (perturb_cameras(cam_gt, 30, 0.02, seed=0)): the overlap lists then
name references that see another part of the rig, and every match is a lone wrong candidate within 40 px of a wrong prediction --
904 of them (F), at most 29 per pair, 0 .. 74 per assembled query at K = 4.  With the default min_inliers = 6 the 4 px RANSAC gate
finds SOME homography with 6 .. 13 inliers in 8 (K = 1) / 15 (K = 4) of the 24 queries, and the solve, started at the prior, fits those few matches: the
default gate does not reject a wrong prior.  This is chance agreement: beyond the four sampled matches each of n <= 112 candidates
lies within 4 px of a model with probability about (4 / 40)^2 = 1 %, so over the RANSAC's iterations a handful more do, never tens.
A true overlap on this data yields 247 matches per query at the median (K = 1).  (d) therefore runs with min_inliers = 30, between
the two by a wide margin on either side, and the run reports a query the gate kept nothing of as not accepted.  On the device,
K = 1 / 4: 8 / 15 of 24 accepted with min_inliers = 6 (the restatement's inlier counts, match for match), 0 / 0 with 30."""
import types

import numpy as np
import pytest

import desc_guided_util as gu
import reloc_prior_util as pu

pytestmark = pytest.mark.gpu

LM = dict(max_num_iterations=200)
TRIM = dict(trim_px=2.0, k_sigma=3.0, max_rounds=8, min_keep=8)
MATCH = dict(min_matches=8)
PRIOR = dict(radius_px=40.0, max_refs=8, min_overlap=8)
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
def data(pkg):
    out = {}
    for ft in (0, 1):
        rig = pkg.synth.make_scene(0, 20, 100).cam_gt.copy()
        if ft:
            rig[:, 10] = np.random.default_rng(100).uniform(-0.05, 0.05, len(rig))
        sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=24, n_feat=600, visible_share=0.5, noise_px=0.5, factor_type=ft, seed=0)
        refs, tests = pkg.synth_reloc.make_reloc_descriptors(sc, D=128, noise=12, n_distractors=50, seed=0, repeat_share=0.7, repeat_group=4,
                                                             repeat_noise=6)
        out[ft] = types.SimpleNamespace(rig=rig, sc=sc, refs=refs, tests=tests, prior=pkg.synth_reloc.perturb_cameras(sc.cam_gt, 0.3, 0.02, seed=0))
    return out


def _pair_list(pp):
    """the pair list and H of every pair from reloc_prior_pairs' lists: query-major, a query's references ascending"""
    ia, ib, H, qptr = [], [], [], [0]
    for q in range(len(pp["n_short"])):
        for s in range(int(pp["n_short"][q])):
            ia.append(int(pp["shortlist"][q, s])); ib.append(q); H.append(pp["H_slot"][q, s])
        qptr.append(len(ia))
    return np.asarray(ia, dtype=np.int32), np.asarray(ib, dtype=np.int32), np.asarray(H, dtype=np.float64).reshape(-1, 9), np.asarray(qptr, dtype=np.int64)


@pytest.fixture(scope="module")
def tracked(pkg, data):
    """the tracked runs (a), (c) and (e) share, by (factor type, K, variant)"""
    cache = {}

    def run(ft, K, variant):
        key = (ft, K, variant)
        if key not in cache:
            d = data[ft]
            kw = dict(trim=TRIM, uncertainty=True) if variant == "trim_cov" else {}
            with pkg.api.DescSet(*d.refs) as refs, pkg.api.DescSet(*d.tests) as tests, pkg.api.Relocalizer(refs, d.rig) as rl:
                got = rl.run(tests, d.sc.query_wh, max_refs=K, factor_type=ft, match=MATCH, prior=dict(PRIOR, cams=d.prior), **kw, **LM)
                got["asm"], got["pairs"] = rl.matches(), rl.pairs()
            cache[key] = got
        return cache[key]

    return run


@pytest.mark.parametrize("variant", ["plain", "trim_cov"])
@pytest.mark.parametrize("ft", [0, 1])
@pytest.mark.parametrize("K", [1, 4])
def test_a_tracked_run_is_the_composition_of_the_public_calls(pkg, data, tracked, K, ft, variant):
    """reloc_prior_pairs -> match_descriptors_guided with the H gathered here -> reloc_assemble -> the prior camera rule in numpy ->
    krt_solve_batch_gated / _trimmed / krt_covariance_batch: every per-query output, bit for bit."""
    api, d = pkg.api, data[ft]
    got = tracked(ft, K, variant)
    pp = api.reloc_prior_pairs(d.rig, d.prior, d.sc.query_wh, factor_type=ft, **PRIOR)
    ia, ib, H, qptr = _pair_list(pp)
    with api.DescSet(*d.refs) as refs, api.DescSet(*d.tests) as tests:
        g = api.match_descriptors_guided(refs, tests, ia, ib, H, None, PRIOR["radius_px"], **MATCH)
    asm = api.reloc_assemble(g["match_ptr"], g["uv_a"], g["uv_b"], ia, qptr, d.rig, d.sc.query_wh, factor_type=ft, max_refs=K)
    b = types.SimpleNamespace(n_query=24, match_ptr=asm["match_ptr"], uv_ref=asm["uv_ref"], uv_cur=asm["uv_cur"], cam_ref=asm["cam_ref"],
                              cam_init=pu.prior_camera(asm["cam_init"], d.prior, ft), factor_type=ft)
    cam, summ, acc, ninl, gmask, _, _ = api.krt_solve_batch_gated(b, ransac_thresh=4.0, min_inliers=6, **LM)
    want = dict(cam=cam, summaries=summ, accepted=acc * (ninl > 0), n_inliers=ninl, trim_report=None, cov=None, sigma0=None, cov_status=None)
    if variant == "trim_cov":
        cam, summ, acc, kept, rep, _ = api.krt_solve_batch_trimmed(b, match_mask=gmask, **TRIM, **LM)
        acc = acc * (ninl > 0)
        cov, s0, status = api.krt_covariance_batch(b, cam, match_mask=kept, accepted=acc)[:3]
        want.update(cam=cam, summaries=summ, accepted=acc, trim_report=rep, cov_status=status)
        ok = status == api.COV_OK
        assert ok.sum() >= 20 and np.array_equal(got["cov"][ok], cov[ok]) and np.array_equal(got["sigma0"][ok], s0[ok])
    want["n_matches"] = np.diff(asm["match_ptr"]).astype(np.int32)
    want["n_sel"] = asm["n_sel"]
    want["sel_ref"] = np.where(asm["sel_pair"] < 0, -1, ia[np.maximum(asm["sel_pair"], 0)])
    for key in PER_QUERY:
        if key not in ("cov", "sigma0"):
            assert _same(got[key], want[key]), (K, ft, variant, key)
    for key in ("shortlist", "n_short", "overlap"):
        assert np.array_equal(got[key], pp[key]), key
    for key in ("match_ptr", "uv_ref", "uv_cur", "src"):
        assert np.array_equal(got["asm"][key], asm[key]), key
    assert np.array_equal(got["pairs"]["pair_ref"], ia) and np.array_equal(got["pairs"]["query_ptr"], qptr)
    assert want["accepted"].all() and (ninl > 0).all()


def test_b_the_table_is_the_numpy_restatements(pkg, data):
    """The first six queries alone (a query's pairs depend on its own prior and image only): the tracked run's match table against
    desc_guided_util.match_pairs_guided under the numpy restatement's lists and H."""
    d = data[0]
    (rp, rd, rk), (qp, qd, qk) = d.refs, d.tests
    n = 6
    cut = int(qp[n])
    Rr, Rq = pkg.api.reloc_ref_rotations(d.rig), pkg.api.reloc_ref_rotations(d.prior[:n])
    pp = pu.prior_pairs(d.rig, Rr, d.prior[:n], Rq, d.sc.query_wh[:n], 0, PRIOR["max_refs"], PRIOR["min_overlap"])
    ia, ib, H, qptr = _pair_list(pp)
    want = gu.match_pairs_guided(rd, rp, rk, qd, qp, qk, ia, ib, H, None, PRIOR["radius_px"], **MATCH)
    with pkg.api.DescSet(rp, rd, rk) as refs, pkg.api.DescSet(qp[:n + 1], qd[:cut], qk[:cut]) as tests, pkg.api.Relocalizer(refs, d.rig) as rl:
        got = rl.run(tests, d.sc.query_wh[:n], max_refs=4, match=MATCH, prior=dict(PRIOR, cams=d.prior[:n]), **LM)
        table, pairs = rl.table(), rl.pairs()
    assert np.array_equal(pairs["pair_ref"], ia) and np.array_equal(pairs["query_ptr"], qptr)
    for key in ("shortlist", "n_short", "overlap"):
        assert np.array_equal(got[key], pp[key]), key
    gu.assert_equal(table, want)
    assert want["match_ptr"][-1] > 1000 and got["accepted"].all()


@pytest.mark.parametrize("ft", [0, 1])
@pytest.mark.parametrize("K", [1, 4])
def test_c_a_prior_beats_the_all_pairs_run_on_repeated_texture(pkg, data, tracked, K, ft):
    """THE test that needs the feature.  Same data, same K: 24 of 24 accepted, the median match count per query at least twice the
    all-pairs run's, the median relative focal error (FDist: the median k1 error) at most the all-pairs run's.  Figures of the CPU
    experiment in the module's docstring; seed 0 is the one of six for which all four (K, factor) cases hold."""
    d = data[ft]
    got = tracked(ft, K, "plain")
    with pkg.api.DescSet(*d.refs) as refs, pkg.api.DescSet(*d.tests) as tests, pkg.api.Relocalizer(refs, d.rig) as rl:
        dense = rl.run(tests, d.sc.query_wh, max_refs=K, factor_type=ft, match=MATCH, **LM)
    gt = d.sc.cam_gt
    err = lambda r, col: float(np.median(np.abs(r["cam"][r["accepted"] == 1, col] - gt[r["accepted"] == 1, col]) /
                                         (gt[r["accepted"] == 1, col] if col == 0 else 1.0)))
    n_t, n_d = np.median(got["n_matches"]), np.median(dense["n_matches"])
    print(f"factor {ft}, K = {K}: accepted {int(got['accepted'].sum())} / {int(dense['accepted'].sum())}, matches {n_d:.1f} -> {n_t:.1f}, "
          f"focal {err(dense, 0):.3e} -> {err(got, 0):.3e}, k1 {err(dense, 10):.3e} -> {err(got, 10):.3e}")
    assert got["accepted"].sum() == 24
    assert n_t >= 2 * n_d, (n_t, n_d)
    if ft == 0:
        assert err(got, 0) <= err(dense, 0), (err(got, 0), err(dense, 0))
    else:
        assert err(got, 10) <= err(dense, 10), (err(got, 10), err(dense, 10))


def test_d_priors_thirty_degrees_off_lose_every_query(pkg, data):
    """min_inliers = 30: the reasoning and the figures with the default are in the module's docstring"""
    d = data[0]
    far = pkg.synth_reloc.perturb_cameras(d.sc.cam_gt, 30.0, 0.02, seed=0)
    with pkg.api.DescSet(*d.refs) as refs, pkg.api.DescSet(*d.tests) as tests, pkg.api.Relocalizer(refs, d.rig) as rl:
        got = rl.run(tests, d.sc.query_wh, max_refs=4, min_inliers=30, match=MATCH, prior=dict(PRIOR, cams=far), **LM)
    print("n_short", got["n_short"], "n_matches", got["n_matches"], "n_inliers", got["n_inliers"], "accepted", got["accepted"])
    assert not got["accepted"].any() and np.isfinite(got["cam"]).all()


def test_e_no_dense_stage_and_at_most_r_pairs_per_query(tracked):
    for K in (1, 4):
        got = tracked(0, K, "plain")
        assert got["stage_ms"][0] == 0 and got["stage_ms"][1] > 0 and got["stage_ms"][3] > 0 and got["prior_ms"] > 0
        per = np.diff(got["pairs"]["query_ptr"])
        assert (per <= PRIOR["max_refs"]).all() and np.array_equal(per, got["n_short"]) and per.max() == 8


def test_f_the_other_runs_keep_their_bits_around_a_tracked_run(pkg, data):
    d = data[0]
    n = 6
    cut = int(d.tests[0][n])
    kw = dict(max_refs=4, match=MATCH, **LM)
    with pkg.api.DescSet(*d.refs) as refs, pkg.api.DescSet(d.tests[0][:n + 1], d.tests[1][:cut], d.tests[2][:cut]) as tests, \
            pkg.api.Relocalizer(refs, d.rig) as rl:
        wh = d.sc.query_wh[:n]
        a0 = rl.run(tests, wh, **kw)
        s0 = rl.run(tests, wh, shortlist=dict(max_refs=8, n_probes=256), **kw)
        t0 = rl.run(tests, wh, prior=dict(PRIOR, cams=d.prior[:n]), **kw)
        a1 = rl.run(tests, wh, **kw)
        s1 = rl.run(tests, wh, shortlist=dict(max_refs=8, n_probes=256), **kw)
        t1 = rl.run(tests, wh, prior=dict(PRIOR, cams=d.prior[:n]), **kw)
        with pytest.raises(ValueError):
            rl.run(tests, wh, shortlist={}, prior=dict(cams=d.prior[:n]), **kw)
        bad = d.prior[:n].copy()
        bad[2, 4] = np.nan
        with pytest.raises(pkg.api.PtzError) as e:
            rl.run(tests, wh, prior=dict(cams=bad), **kw)
        assert e.value.code == -1
    for x, y in ((a0, a1), (s0, s1), (t0, t1)):
        for key in PER_QUERY:
            assert _same(x[key], y[key]), key
    for key in ("shortlist", "n_short", "votes"):
        assert np.array_equal(s0[key], s1[key])
    assert a0["accepted"].all() and t0["accepted"].all()
