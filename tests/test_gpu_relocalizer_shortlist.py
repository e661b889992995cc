"""GPU tests of ptz_relocalizer_run_shortlisted (api.Relocalizer.run(..., shortlist=...)) on the data set of
test_four_references_beat_one_on_the_same_data: the 20-view rig make_scene(0, 20, 100), make_reloc_scene(n_query=24, n_feat=600,
visible_share=0.5, noise_px=0.5, seed=0), factor F, make_reloc_descriptors(D=128, noise=12, n_distractors=50, seed=0); the matcher
runs with min_matches = 8 as in test_gpu_relocalizer.py.

A pair's matches depend on its two images only and the assembly ranks a query's pairs by (match count, position), so whenever a
query's shortlist holds the K references the all-pairs run selects, every per-query output is that run's bits.  Whether it does is a
property of the DATA, derived with the numpy restatements alone (desc_match_util.match_pairs for the all-pairs counts,
desc_shortlist_util for the votes; CPU, ratio 0.8, ties by index) before the first device run.  Over the 24 queries, 0-based vote
ranks:

    M     worst rank of the all-pairs anchor   worst rank of any of the four best   matched references without a vote
    64                    3                                   10                                   9
    128                   3                                    7                                   2
    256                   1                                    6                                   1
    384                   1                                    6                                   0
    650 (every feature)   0                                    3                                   0

(5 to 16 of the 20 references share matches with a query: a dense rig.)  So with M = 256 the anchor is inside R = 4 and
the four best inside R = 8 for all 24 queries -- tests (a) and (b).  For (c), the whole run with R = 20, M = 256 leaves ONE
(reference, query) pair with matches but no vote, so the restatement alone does not satisfy it; the probe budget is raised until
it does.  (c) runs with M = 650 >= n: every feature is a probe, and a match of the mutual test under the ratio test is a probe
whose nearest neighbour passes the ratio test, so every matched reference has a vote by construction.
The device's shortlist is asserted array-equal to the restatement's, so the device adds no uncertainty of its own."""
import numpy as np
import pytest

import desc_shortlist_util as su

pytestmark = pytest.mark.gpu

LM = dict(max_num_iterations=200)
TRIM = dict(trim_px=2.0, k_sigma=3.0, max_rounds=8, min_keep=8)
MATCH = dict(min_matches=8)
PER_QUERY = ("cam", "accepted", "summaries", "sel_ref", "n_sel", "n_matches", "n_inliers", "trim_report", "cov", "sigma0", "cov_status")
VARIANTS = {"plain": {}, "guided": dict(guided_radius=4.0), "gated": dict(inlier_matches=True), "trimmed": dict(trim=TRIM),
            "uncertainty": dict(uncertainty=True)}


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
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt.copy()
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=24, n_feat=600, visible_share=0.5, noise_px=0.5, factor_type=0, seed=0)
    refs, tests = pkg.synth_reloc.make_reloc_descriptors(sc, D=128, noise=12, n_distractors=50, seed=0)
    return rig, sc, refs, tests


@pytest.fixture(scope="module")
def restated(data):
    """the restatement's votes per probe budget, computed once"""
    _, _, (rp, rd, _), (qp, qd, _) = data
    cache = {}
    return {M: su.shortlist(rd, rp, qd, qp, max_refs=20, n_probes=M, cache=cache)["votes"] for M in (256, 650)}


@pytest.fixture(scope="module")
def runner(pkg, data):
    """the resident objects, and the all-pairs runs computed once per option set"""
    rig, sc, (rp, rd, rk), (qp, qd, qk) = data
    api = pkg.api
    with api.DescSet(rp, rd, rk) as refs, api.DescSet(qp, qd, qk) as tests, api.Relocalizer(refs, rig) as rl:
        done = {}

        def run(shortlist=None, tables=False, **kw):
            key = repr(sorted(kw.items()))
            if shortlist is None and not tables and key in done:
                return done[key]
            out = rl.run(tests, sc.query_wh, match=MATCH, shortlist=shortlist, **kw, **LM)
            if tables:
                out["table"], out["pairs"], out["assembled"] = rl.table(), rl.pairs(), rl.matches()
            elif shortlist is None:
                done[key] = out
            return out

        yield run


def _assert_lists(got, votes, R):
    rows = [su.select(v, R, 1) for v in votes]
    assert np.array_equal(got["votes"], votes)
    assert np.array_equal(got["shortlist"], np.stack([r[0] for r in rows])) and np.array_equal(got["n_short"], [r[1] for r in rows])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_four_listed_one_selected(runner, restated, variant):
    """(a) R = 4, max_refs = 1, M = 256: every per-query output of all 24 queries is ptz_relocalizer_run's, with the guided pass, the
    gate, the trimming loop and the covariance as well"""
    kw = dict(max_refs=1, **VARIANTS[variant])
    want = runner(**kw)
    got = runner(shortlist=dict(max_refs=4, n_probes=256), **kw)
    _assert_lists(got, restated[256], 4)
    for q in range(24):  # the data's condition, from the restatement and the all-pairs run: the anchor is on the list
        assert want["sel_ref"][q, 0] in got["shortlist"][q], q
    for key in PER_QUERY:
        assert _same(got[key], want[key]), (variant, key)
    assert want["accepted"].sum() >= 20 and (got["n_short"] <= 4).all() and got["shortlist_ms"] > 0


def test_b_eight_listed_four_selected(runner, restated):
    """(b) R = 8, max_refs = 4, M = 256 against the all-pairs K = 4 run"""
    want = runner(max_refs=4)
    got = runner(shortlist=dict(max_refs=8, n_probes=256), max_refs=4)
    _assert_lists(got, restated[256], 8)
    for q in range(24):
        assert set(want["sel_ref"][q, :want["n_sel"][q]]) <= set(got["shortlist"][q]), q
    for key in PER_QUERY:
        assert _same(got[key], want[key]), key
    assert (want["n_sel"] == 4).sum() >= 20 and want["accepted"].all()


def test_c_every_reference_listed_is_the_whole_run(runner, restated):
    """(c) R = 20 with every feature a probe (M = 650, see the module's docstring): the whole run is the all-pairs run bit for bit --
    per-query outputs, the assembled matches, and the match table once the empty pairs of either run are dropped"""
    want = runner(tables=True, max_refs=4)
    got = runner(shortlist=dict(max_refs=20, n_probes=650), tables=True, max_refs=4)
    _assert_lists(got, restated[650], 20)
    for key in PER_QUERY:
        assert _same(got[key], want[key]), key
    for key in ("match_ptr", "uv_ref", "uv_cur"):
        assert np.array_equal(got["assembled"][key], want["assembled"][key]), key
    tabs = []
    for out in (want, got):
        t, p = out["table"], out["pairs"]
        n = np.diff(t["match_ptr"])
        query = np.repeat(np.arange(24), np.diff(p["query_ptr"]))
        keep = n > 0
        tabs.append(dict(ref=p["pair_ref"][keep], query=query[keep], n=n[keep], **{k: t[k] for k in ("idx_a", "idx_b", "dist2", "uv_a", "uv_b")}))
    assert len(want["pairs"]["pair_ref"]) == 24 * 20 and len(got["pairs"]["pair_ref"]) == got["n_short"].sum() < 24 * 20
    for key in tabs[0]:
        assert np.array_equal(tabs[0][key], tabs[1][key]), key
    assert tabs[0]["n"].sum() > 0


def test_a_query_without_a_list_goes_on_unselected(runner):
    """min_votes above every count: no pairs at all, every query as a query with n_sel = 0"""
    got = runner(shortlist=dict(max_refs=4, n_probes=16, min_votes=17), tables=True, max_refs=1)
    assert (got["n_short"] == 0).all() and (got["shortlist"] == -1).all() and (got["n_sel"] == 0).all() and (got["n_matches"] == 0).all()
    assert (got["sel_ref"] == -1).all() and len(got["pairs"]["pair_ref"]) == 0 and (got["pairs"]["query_ptr"] == 0).all()
