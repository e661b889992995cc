"""GPU tests of the launch extents of the batch LM passes: a batch whose active count falls through every variant threshold
reproduces the bits of its scenes solved alone, whatever extent the host gives a pass (exact fit or the ladder's), whichever way
the device's compacted list is split over scene groups, and when passes are replayed from graphs, which keep the ladder.

The batch: the 48 scenes make_scene(seed, 20, 100), seeds 0..47.  44 of them take 4 to 7 LM steps, seeds 18, 29, 19 and 42 take
22, 23, 25 and 29, so the active count per pass runs 48, 48, 48, 48, 43, 12, 7, 4 ... 3, 2, 2, 1: one solve crosses the ranges
in which the ladder's shapes differ (> 32, 9-32, 5-8, 3-4, <= 2 active scenes).  The counts are taken from the device's own solo
solves, and the test fails if they do not visit all five ranges.

The library reads its PTZ_BA_* switches when a batch is created, so a setting is an environment variable set around the batch's
construction (the pattern of the cross-variant tests in test_gpu_parity.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEEDS = range(48)
FIELDS = 12  # fields of ptz_lm_summary


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


def test_active_counts_cross_every_variant_threshold(solo):
    steps = np.array([s["num_lm_steps"] for s in solo[2]])
    counts = [int((steps > p).sum()) for p in range(int(steps.max()))]
    print("LM steps per scene:", steps.tolist())
    print("active scenes per pass:", counts)
    assert counts[0] == 48
    ranges = {"> 32": lambda c: c > 32, "9-32": lambda c: 9 <= c <= 32, "5-8": lambda c: 5 <= c <= 8, "3-4": lambda c: 3 <= c <= 4,
              "<= 2": lambda c: 1 <= c <= 2}
    missing = [k for k, f in ranges.items() if not any(f(c) for c in counts)]
    assert not missing, (missing, counts)


# (i) the batch as the library runs it: two groups of 24, each with its own count and list -- and as one group of 48, the only way the
# batch reaches the shapes of more than 32 active scenes; (ii) the ladder's extents; (iv) k_schur_f's table in global memory; (v) two
# scene groups, asked for by name; (vi) a second solve without the Cholesky look-ahead: passes replayed from graphs, ladder extents
# (there is no (iii): the k_schur_f work loop and its PTZ_BA_SCHUR_LOOP switch were measured and left out, profiles/NOTES_r07.md)
VARIANTS = [("default", (), 1),
            ("one group", (("PTZ_BA_STREAMS", "1"),), 1),
            ("ladder extents", (("PTZ_BA_EXACT_FIT", "0"), ("PTZ_BA_STREAMS", "1")), 1),
            ("ladder extents, two groups", (("PTZ_BA_EXACT_FIT", "0"),), 1),
            ("global T rows", (("PTZ_BA_SCHUR_GLOBAL_T", "1"), ("PTZ_BA_STREAMS", "1")), 1),
            ("two groups", (("PTZ_BA_STREAMS", "2"),), 1),
            ("replayed graphs", (("PTZ_BA_LOOKAHEAD", "0"),), 2),
            ("replayed graphs, one group", (("PTZ_BA_LOOKAHEAD", "0"), ("PTZ_BA_STREAMS", "1")), 2)]


@pytest.mark.parametrize("name,env,solves", VARIANTS, ids=[v[0].replace(", ", "_").replace(" ", "_") for v in VARIANTS])
def test_batch_reproduces_solo_solves(pkg, scenes, solo, monkeypatch, name, env, solves):
    _assert_same(_solve_batch(pkg, scenes, monkeypatch, env, solves), solo, name)


@pytest.mark.parametrize("env", [(), (("PTZ_BA_STREAMS", "1"),), (("PTZ_BA_EXACT_FIT", "0"), ("PTZ_BA_STREAMS", "1"))],
                         ids=["default", "one_group", "ladder"])
def test_count_that_falls_from_all_to_one_between_two_host_reads(pkg, scenes, solo, monkeypatch, env):
    """The staleness case: every scene of the batch but one retires in the same pass, so the device's count drops from n to 1
    while the host, which runs several passes ahead, still sizes grids for n -- slots beyond the device's count must do nothing,
    and the survivor's later single-slot passes must find it through the list.  (The options of a batch are common to its scenes, so
    the scenes that stop together are 47 copies of one scene -- seed 0, 4 steps -- rather than scenes with a small
    max_num_iterations of their own; the survivor is seed 42, 29 steps.)"""
    steps = [s["num_lm_steps"] for s in solo[2]]
    assert steps[42] > steps[0] + 8
    order = [0] * 20 + [42] + [0] * 27
    want = ([solo[0][i] for i in order], [solo[1][i] for i in order], [solo[2][i] for i in order])
    _assert_same(_solve_batch(pkg, [scenes[i] for i in order], monkeypatch, env), want, "all but one retire together")
