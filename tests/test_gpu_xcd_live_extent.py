"""GPU tests of the live-extent XCD mapping (ptz_xcd_map.h): in a compacted LM pass the (camera, slot) and (tile, slot) launches
deal their workgroups over the XCDs by the device's own count of live slots, not by the grid the host sized from an older count.
Which workgroup takes which item is a speed matter only, so a batch must reproduce the bits of its scenes solved alone with the
mapping on (the default) and off (PTZ_BA_XCD_LIVE=0), whatever the extent of its passes.

The batch is that of test_gpu_launch_shapes.py: the 48 scenes make_scene(seed, 20, 100), seeds 0..47, whose active count per pass
runs 48 ... 43, 12, 7, 4 ... 1.  The host's count is up to three passes old, so compacted passes with more slots than live scenes
occur with exact-fit extents (e.g. 43 slots for 12 live scenes), far more with the ladder's extents (PTZ_BA_EXACT_FIT=0), and in
passes replayed from graphs (a second solve without the Cholesky look-ahead), whose grids are the ladder's.

The library reads its PTZ_BA_* switches when a batch is created, so a setting is an environment variable set around the batch's
construction."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEEDS = range(48)
FIELDS = 12  # fields of ptz_lm_summary
K1_SEEDS = range(24)  # the batch of a factor type with a distortion column (k_schur instead of k_schur_f)


@pytest.fixture(scope="module")
def scenes(pkg):
    return [pkg.synth.make_scene(s, 20, 100) for s in SEEDS]


@pytest.fixture(scope="module")
def solo(pkg, scenes):
    """every scene solved alone: (cams, rays, summaries); computed once, shared, never modified"""
    out = [pkg.api.ba_solve(sc) for sc in scenes]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def _solve_batch(pkg, scenes, monkeypatch, env=(), solves=1):
    for k, v in env:
        monkeypatch.setenv(k, v)
    try:
        b = pkg.api.BaBatch(scenes)
        for _ in range(solves):
            b.set_state()
            summ = b.solve()
        cams, rays = b.get_state()
        b.close()
    finally:
        for k, _ in env:
            monkeypatch.delenv(k)
    return cams, rays, summ


def _assert_same(got, want, what):
    cams, rays, summ = got
    wc, wr, ws = want
    assert len(summ) == len(ws)
    for i, (s, w) in enumerate(zip(summ, ws)):
        assert len(s) == FIELDS and s == w, (what, i, s, w)  # all twelve fields, num_lm_steps among them
        assert np.array_equal(cams[i], wc[i]) and np.array_equal(rays[i], wr[i]), (what, i)


def _stale_passes(summaries, ahead=3):
    """passes whose grid, sized by the count of `ahead` passes before, has more slots than scenes are live (an upper bound on the
    host's knowledge: it may be more recent)"""
    steps = np.array([s["num_lm_steps"] for s in summaries])
    counts = [int((steps > p).sum()) for p in range(int(steps.max()))]
    return sum(1 for p in range(ahead, len(counts)) if counts[p] < counts[p - ahead] and counts[p - ahead] < len(steps))


def test_compacted_passes_with_more_slots_than_live_scenes_occur(solo):
    assert _stale_passes(solo[2]) >= 3


EXTENTS = [("default", (), 1),
           ("one group", (("PTZ_BA_STREAMS", "1"),), 1),
           ("ladder extents", (("PTZ_BA_EXACT_FIT", "0"), ("PTZ_BA_STREAMS", "1")), 1),
           ("replayed graphs", (("PTZ_BA_LOOKAHEAD", "0"),), 2)]
MAPPINGS = [("live", ()), ("grid", (("PTZ_BA_XCD_LIVE", "0"),))]


@pytest.mark.parametrize("mapping,menv", MAPPINGS, ids=[m[0] for m in MAPPINGS])
@pytest.mark.parametrize("name,env,solves", EXTENTS, ids=[v[0].replace(" ", "_") for v in EXTENTS])
def test_batch_reproduces_solo_solves(pkg, scenes, solo, monkeypatch, name, env, solves, mapping, menv):
    _assert_same(_solve_batch(pkg, scenes, monkeypatch, tuple(env) + tuple(menv), solves), solo, (name, mapping))


def test_all_but_one_retire_in_one_pass(pkg, scenes, solo, monkeypatch):
    """The device's count drops from 48 to 1 while the host still sizes grids for 48: one live row in a launch of 48, every XCD
    takes its share of that row's cameras and tiles, and the 47 other rows' workgroups return."""
    steps = [s["num_lm_steps"] for s in solo[2]]
    assert steps[42] > steps[0] + 8
    order = [0] * 20 + [42] + [0] * 27
    want = ([solo[0][i] for i in order], [solo[1][i] for i in order], [solo[2][i] for i in order])
    _assert_same(_solve_batch(pkg, [scenes[i] for i in order], monkeypatch), want, "all but one retire together")


@pytest.fixture(scope="module")
def dist_batch(pkg):
    """24 PTZRayDist scenes and their solo solves; computed once, shared, never modified"""
    sc = [pkg.synth.make_scene(s, 20, 100, factor_type=1) for s in K1_SEEDS]
    out = [pkg.api.ba_solve(x) for x in sc]
    return sc, ([o[0] for o in out], [o[1] for o in out], [o[2] for o in out])


@pytest.mark.parametrize("mapping,menv", MAPPINGS, ids=[m[0] for m in MAPPINGS])
def test_factor_type_with_distortion_takes_k_schur(pkg, dist_batch, monkeypatch, mapping, menv):
    """PTZRayDist scenes are linearised by k_schur (k_schur_f is PTZRay's): the same mapping at that kernel's top.  One group of
    24 scenes (a batch of up to 32 runs two passes ahead), so that the group's passes are compacted as soon as a scene retires."""
    sc, want = dist_batch
    assert _stale_passes(want[2], ahead=2) >= 1
    _assert_same(_solve_batch(pkg, sc, monkeypatch, (("PTZ_BA_STREAMS", "1"),) + tuple(menv)), want, ("PTZRayDist", mapping))
