"""GPU tests of the landmark view (ptz-calib_amd/csrc/ptz_landmark_prior.hip): the device-pointer form on raw rays and the host form
on maps built by landmark_util, array-equal to the host instantiation of the shared header
(tests/cpu_harness/landmark_prior_harness.cc), which test_cpu_landmark_prior.py holds to the numpy restatement; the gathered
descriptor set against numpy distances and against a set packed from the same rows by ptz_desc_set_create, through both guided
kernels; the limits and the argument errors.
The rotation matrices are an input of the contract: the harness gets the library's own (api.reloc_ref_rotations)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import desc_match_util as du
import landmark_prior_util as lp
import landmark_util as lu

pytestmark = pytest.mark.gpu

N_FEAT = 80
I9 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.float64)


def test_device_form_on_raw_rays():
    """ptz_landmark_visible_device on raw rays (m_z <= 0, NaN, infinite and huge components among them), stale workspace and
    outputs, n_lm in {0, 1, 63, 64, 65, 255, 256, 257, 1025, 2049} x n_query in {0, 1, 5, 257}, and a capacity that cuts.  Own
    process with torch initialised first (as test_gpu_landmark_map.py::test_device_form_on_the_cases)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "run_landmark_visible_device.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "landmark visible device ok: 44 cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def maps(pkg):
    """landmark_util's rig, features and tracks as device maps, F and FDist"""
    out = {}
    for ft in (0, 1):
        cams = lu.make_rig(ft & 1, seed=5 + ft)
        feats = lu.make_features(len(cams), 64, N_FEAT, seed=6 + ft)
        tp, ti, tf, _ = lu.make_tracks(len(cams), N_FEAT, seed=7 + ft)
        refs = pkg.api.DescSet(*feats)
        m = pkg.api.LandmarkMap(refs, cams, tp, ti, tf, factor_type=ft)
        out[ft] = (cams, m, m.arrays(), refs)
    yield out
    for v in out.values():
        v[1].close()
        v[3].close()


def _priors(cams, seed):
    """the references themselves as priors, turned a little, with sizes of their own and fy != fx; reference 5 once more, looking
    straight up through a very long lens: it sees nothing"""
    rng = np.random.default_rng(seed)
    pri = np.insert(cams, 5, cams[5], axis=0)
    pri[:, 4:7] += rng.uniform(-0.02, 0.02, (len(pri), 3))
    pri[5, 0], pri[5, 4:7] = 1e7, (0.5 * np.pi, 0.0, 0.0)
    cams = pri
    pri[:, 1] = pri[:, 0] * rng.uniform(0.9, 1.1, len(cams))
    wh = np.stack([rng.integers(600, 4000, len(cams)), rng.integers(400, 2200, len(cams))], axis=1).astype(np.int32)
    return pri, wh


@pytest.mark.parametrize("ft", [0, 1, 2, 3])
def test_host_form_equals_harness(pkg, maps, ft):
    cams, m, lm, _ = maps[ft & 1]
    pri, wh = _priors(cams, 30 + ft)
    R = pkg.api.reloc_ref_rotations(pri)
    for radius in (40.0, 7.5):
        want = lp.harness_visible(lm["lm_ray"], pri, wh, ft, radius, prior_R=R)
        with pkg.api.landmark_visible(m, pri, wh, factor_type=ft, radius_px=radius) as v:
            got = v.arrays()
            assert v.n_visible == len(want["vis_lm"]) and v.device_ms > 0 and all(v.device_ptrs())
        lp.assert_equal(got, want, (ft, radius))
        n = np.diff(got["vis_ptr"])
        assert n.max() > 20 and n[5] == 0, n  # the empty view in the middle of the batch
    # a query's bits alone, reversed, and no query at all
    for qs in ([3], list(range(len(pri)))[::-1], []):
        with pkg.api.landmark_visible(m, pri[qs], wh[qs], factor_type=ft) as v:
            part = v.arrays()
        lp.assert_equal(part, lp.harness_visible(lm["lm_ray"], pri[qs], wh[qs], ft, 40.0, prior_R=R[qs]), (ft, qs))
    assert part["vis_ptr"].tolist() == [0] and len(part["vis_lm"]) == 0


# ---- the gathered set -------------------------------------------------------------------------------------------------------------
F, W, H = 2000.0, 200, 200
STEP_DEG = 8.0  # 2000 tan(8 degrees) = 281 px between the clusters: a query of 200 x 200 px and radius 10 sees its own only


def _cluster_map(pkg, D, sizes, seed):
    """One reference per cluster, panned STEP_DEG apart, with sizes[k] features within 60 px of its centre, every feature a track of
    its own: a prior equal to reference k with a 200 x 200 image sees exactly cluster k, predicted at (dx + 100, dy + 100)."""
    rng = np.random.default_rng(seed)
    n = len(sizes)
    cams = np.zeros((n, 15))
    cams[:, 0] = cams[:, 1] = F
    cams[:, 2], cams[:, 3] = 960.0, 540.0
    cams[:, 5] = np.radians(STEP_DEG) * np.arange(n)
    fp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    nf = int(fp[-1])
    desc = rng.integers(0, 256, (nf, D), dtype=np.uint8)
    kp = (np.array([960.0, 540.0]) + rng.uniform(-60, 60, (nf, 2))).astype(np.float32)
    tp = np.arange(nf + 1, dtype=np.int64)
    ti = np.repeat(np.arange(n), sizes).astype(np.int32)
    tf = (np.arange(nf) - fp[ti]).astype(np.int32)
    refs = pkg.api.DescSet(fp, desc, kp)
    m = pkg.api.LandmarkMap(refs, cams, tp, ti, tf)
    pri = cams.copy()
    wh = np.tile(np.array([W, H], dtype=np.int32), (n, 1))
    return refs, m, pri, wh


def _queries(lm_desc, view, seed, noise=6, n_distractors=20):
    """per query: a noisy copy of seven in ten of its visible landmarks within 3 px of the prediction, and distractors"""
    rng = np.random.default_rng(seed)
    ptr, desc, kp = [0], [], []
    D = lm_desc.shape[1]
    for q in range(len(view["vis_ptr"]) - 1):
        pq = lp.per_query(view, q)
        take = np.nonzero(rng.random(len(pq["vis_lm"])) < 0.7)[0]
        d = np.clip(lm_desc[pq["vis_lm"][take]].astype(np.int64) + rng.integers(-noise, noise + 1, (len(take), D)), 0, 255).astype(np.uint8)
        desc += [d, rng.integers(0, 256, (n_distractors, D), dtype=np.uint8)]
        kp += [pq["vis_uv"][take] + rng.uniform(-3, 3, (len(take), 2)).astype(np.float32),
               rng.uniform([0, 0], [W, H], (n_distractors, 2)).astype(np.float32)]
        ptr.append(ptr[-1] + len(take) + n_distractors)
    return np.asarray(ptr, dtype=np.int64), np.concatenate(desc), np.concatenate(kp).astype(np.float32)


def _check_gathered_set(pkg, D, sizes, seed, dist2_of=None):
    api = pkg.api
    refs, m, pri, wh = _cluster_map(pkg, D, sizes, seed)
    try:
        lm = m.arrays()
        nq = len(sizes)
        with api.landmark_visible(m, pri, wh, radius_px=10.0) as v:
            view = v.arrays()
            lp.assert_equal(view, lp.harness_visible(lm["lm_ray"], pri, wh, 0, 10.0, prior_R=api.reloc_ref_rotations(pri)), (D, sizes))
            assert np.diff(view["vis_ptr"]).tolist() == list(sizes)
            qp, qd, qk = _queries(lm["lm_desc"], view, seed + 1)
            vset = v.desc_set()
            rows = lm["lm_desc"][view["vis_lm"]]
            with api.DescSet(qp, qd, qk) as tests, api.DescSet(view["vis_ptr"], rows, view["vis_uv"]) as packed:
                for q in (range(nq) if dist2_of is None else dist2_of):
                    want = du.dist2(rows[view["vis_ptr"][q]:view["vis_ptr"][q + 1]], qd[qp[q]:qp[q + 1]])
                    assert np.array_equal(api.desc_dist2(vset, q, tests, q), want), (D, q)
                ia = np.arange(nq, dtype=np.int32)
                n_match = 0
                for grid in (False, True):
                    got = api.match_descriptors_guided(vset, tests, ia, ia, np.tile(I9, (nq, 1)), None, 10.0, grid=grid)
                    want = api.match_descriptors_guided(packed, tests, ia, ia, np.tile(I9, (nq, 1)), None, 10.0, grid=grid)
                    for key in ("match_ptr", "idx_a", "idx_b", "dist2", "uv_a", "uv_b"):
                        assert np.array_equal(got[key], want[key]), (D, grid, key)
                    n_match = len(got["idx_a"])
                    per = np.diff(got["match_ptr"])
                    assert all((per[q] > 0) == (sizes[q] >= 3) for q in range(nq) if sizes[q] == 0 or sizes[q] >= 63), (per, sizes)
        return n_match
    finally:
        m.close()
        refs.close()


@pytest.mark.parametrize("D", [1, 64, 128, 130, 512])
def test_gathered_set_is_the_packed_rows(pkg, D):
    """Views of 0, 1, 63, 64, 65 and 130 visible landmarks, the empty view first, in the middle and last: the matcher's own distances
    through the view's set are numpy's on lm_desc[vis_lm], and both guided kernels return through it what they return through a set
    ptz_desc_set_create packs from the same rows and pixels."""
    n = _check_gathered_set(pkg, D, (0, 1, 63, 0, 64, 65, 130, 0), 40 + D)
    assert n > 100 or D == 1


def test_gathered_set_above_2048_rows(pkg):
    """a view of 2100 landmarks: the grid kernel's second slab of 2048 rows runs on the gathered set"""
    n = _check_gathered_set(pkg, 64, (2100, 0, 5), 90, dist2_of=(0, 2))
    assert n > 1000


def test_limits_and_argument_errors(pkg, maps):
    api = pkg.api
    cams, m, lm, _ = maps[0]
    pri, wh = _priors(cams, 3)

    def code(fn):
        with pytest.raises(api.PtzError) as e:
            fn()
        return e.value.code

    assert code(lambda: api.landmark_visible(m, pri, wh, max_view_bytes=4096)) == -5      # PTZ_ELIMIT: the caller splits the batch
    assert code(lambda: api.landmark_visible(m, pri, wh, max_view_bytes=0)) == -1
    for r in (0.0, -1.0, float("nan"), float("inf")):
        assert code(lambda: api.landmark_visible(m, pri, wh, radius_px=r)) == -1
    assert code(lambda: api.landmark_visible(m, pri, wh, factor_type=4)) == -4
    assert code(lambda: api.landmark_visible(m, pri, wh * 0)) == -1
    for col, val in ((3, np.nan), (12, np.inf), (0, 0.0), (1, -5.0)):
        bad = pri.copy()
        bad[2, col] = val
        assert code(lambda: api.landmark_visible(m, bad, wh)) == -1
    R = api.reloc_ref_rotations(pri)
    R[1, 4] = np.nan
    assert code(lambda: api.landmark_visible(m, pri, wh, prior_R=R)) == -1
    with pytest.raises(ValueError):
        api.landmark_visible(m, pri, wh[:3])
    with api.landmark_visible(m, pri, wh) as v:  # and the same call with nothing wrong
        assert v.n_visible > 0
