"""k_schur_f reads each thread's run of camera-pair entries from global memory in register chunks of four, two chunks deep (one in use, the next on its way), and
fetches three trips of observation records into two rotating buffers.  These tests hold both to the long-double reduced system of
schur_ref_util.py and to their own bits, on scenes cut for the run lengths and observation counts at which those paths hand over.

Scenes (every ray of `runlens` has exactly two views, so a pair's entry count is the number of rays dealt to it):
  * `runlens`, 14 cameras.  Camera 12 shares 1, 2, 3, 4, 5, 7, 8, 9 rays with cameras 0..7 and 250 with each of 8..11: 1039
    entries, more than 256 x 4, cut with L = 5 into runs of 1, 2, 3, 4, 5 (a full chunk and one entry), 5 + 2, 5 + 3, 5 + 4.
    Camera 13 shares 15, 16, 17 rays with cameras 0..2 and 210 with each of 3..12: 2148 entries, L = 9 (two full chunks and one
    entry), remainders 6, 7, 8 and 3.  The test recomputes L and the cut with build_pairs' rule and asserts the lengths.
  * `trips`: cameras with 511, 513, 767, 768 and 1025 observations (and a sixth that gives rays 768..1024 their second view):
    with `edges` of test_gpu_schur_direct.py (255 .. 257, 512, 769, 800) every hand-over of the two record buffers -- one, two,
    three trips exactly full and one over, and the unprefetched tail behind the third.
  * `band` of schur_ref_util (40 cameras of ~60 observations): the only one whose LDS request is below a quarter of a compute
    unit's, where PTZ_BA_SCHUR_WG4 changes the residency.

Bounds: K and the yardstick of schur_ref_util.py, as in test_gpu_schur_direct.py."""
import numpy as np
import pytest

import schur_ref_util as su

pytestmark = pytest.mark.gpu

THREADS = 256
SCALE_SEED = 7
RUNLENS_12 = [1, 2, 3, 4, 5, 7, 8, 9, 250, 250, 250, 250]
RUNLENS_13 = [15, 16, 17] + [210] * 10
TRIP_COUNTS = [511, 513, 767, 768, 1025, 257]
_SC, _LIN, _REF, _SOLO = {}, {}, {}, {}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _scene(pkg, kind):
    if kind in ("edges", "band"):
        return su.scene(pkg, kind, 0)
    if kind not in _SC:
        if kind == "runlens":
            rig = pkg.synth.make_scene(911, 14, 30, factor_type=0, pan_range_deg=2.0)
            lists = [[] for _ in range(14)]
            nxt = 0
            for ci, counts in ((12, RUNLENS_12), (13, RUNLENS_13)):
                for cj, c in enumerate(counts):
                    rays = list(range(nxt, nxt + c))
                    lists[ci] += rays
                    lists[cj] += rays
                    nxt += c
            X, _ = su._pool(nxt, -6, 6, 5, 21)
            _SC[kind] = su._assemble(pkg, rig, X, [np.array(sorted(l)) for l in lists], 31)
        else:
            rig = pkg.synth.make_scene(912, 6, 30, factor_type=0, pan_range_deg=2.0)
            X, _ = su._pool(1025, -6, 6, 5, 22)
            lists = [np.arange(c) for c in TRIP_COUNTS[:5]] + [np.arange(1025 - TRIP_COUNTS[5], 1025)]
            _SC[kind] = su._assemble(pkg, rig, X, lists, 32)
    return _SC[kind]


def _pair_counts(sc):
    inc = np.zeros((sc.n_cam, sc.n_ray), dtype=np.int64)
    inc[sc.obs_cam, sc.obs_ray] = 1
    return inc @ inc.T


def _run_lengths(sc):
    """Per camera: (L, lengths of its runs), by build_pairs' rule: a camera's entries, its pairs (cj < ci, ascending) one after
    the other, are cut into pieces of one length L that never straddle two pairs, L the smallest in [1, longest pair] for which
    the camera has at most THREADS pieces (the longest pair's length if there is none)."""
    cnt = _pair_counts(sc)
    out = []
    for ci in range(sc.n_cam):
        pairs = [int(cnt[ci, cj]) for cj in range(ci) if cnt[ci, cj] > 0]
        if not pairs:
            out.append((0, []))
            continue
        pieces = lambda L: sum((p + L - 1) // L for p in pairs)
        L = next((L for L in range(1, max(pairs)) if pieces(L) <= THREADS), max(pairs))
        out.append((L, [min(L, p - e) for p in pairs for e in range(0, p, L)]))
    return out


def _lin(pkg, kind):
    if kind not in _LIN:
        sc = _scene(pkg, kind)
        b = pkg.api.BaBatch([sc])
        b.set_state()
        lin = b.linearize(0)
        b.close()
        _LIN[kind] = ({k: lin[k] for k in ("U", "g_c", "V", "g_r", "W")}, su.scales(sc, lin["nc"], SCALE_SEED))
    return _LIN[kind]


def _ref(pkg, kind, radius):
    if (kind, radius) not in _REF:
        sc = _scene(pkg, kind)
        lin, (s_c, s_r) = _lin(pkg, kind)
        S, b, Y, Yb, _, _ = su.system(lin, sc.obs_cam, sc.obs_ray, s_c, s_r, radius)
        _REF[(kind, radius)] = dict(S=S, b=b, Y=Y, Yb=Yb, zero=~su.shares_ray(sc, lin["U"].shape[1]))
    return _REF[(kind, radius)]


def _device(pkg, kinds, index, radius):
    """(S, b, diag_c, info) of scene `index` of a FRESH batch of the scenes `kinds`, the system's block poisoned."""
    _, (s_c, s_r) = _lin(pkg, kinds[index])
    b = pkg.api.BaBatch([_scene(pkg, k) for k in kinds], initial_trust_region_radius=radius)
    b.set_state()
    out = b.reduced_system(index, s_c, s_r, poison=True)
    b.close()
    return out


def _solo(pkg, kind, radius):
    """The scene alone under the default switches, once per process: what every bit-for-bit check compares with."""
    if (kind, radius) not in _SOLO:
        _SOLO[(kind, radius)] = _device(pkg, [kind], 0, radius)
    return _SOLO[(kind, radius)]


def _same(a, e, tag):
    for x, y, name in zip(a[:3], e[:3], ("S", "b", "diag_c")):
        assert np.array_equal(_bits(x), _bits(y)), (tag, name, float(np.abs(x - y).max()))


# ---- the scenes are what the kernel's paths need (CPU) ---------------------------------------------------------------------
def test_runlens_scene_has_the_run_lengths(pkg):
    sc = _scene(pkg, "runlens")
    assert sc.n_cam == 14 and (np.bincount(sc.obs_ray) == 2).all()
    cnt = _pair_counts(sc)
    assert cnt[12, :12].tolist() == RUNLENS_12 and cnt[13, :13].tolist() == RUNLENS_13
    off = cnt[np.tril_indices(14, -1)]
    assert set(off[off > 0].tolist()) >= {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17}
    runs = _run_lengths(sc)
    assert sum(RUNLENS_12) > THREADS * 4 and runs[12][0] == 5 and runs[13][0] == 9, [r[0] for r in runs]
    assert all(len(r[1]) <= THREADS for r in runs)
    assert runs[12][1][:11] == [1, 2, 3, 4, 5, 5, 2, 5, 3, 5, 4]
    lengths = set(l for r in runs for l in r[1])
    assert lengths >= {1, 3, 4, 5, 8, 9}, sorted(lengths)


def test_trips_scene_has_the_observation_counts(pkg):
    sc = _scene(pkg, "trips")
    assert np.bincount(sc.obs_cam, minlength=6).tolist() == TRIP_COUNTS and np.bincount(sc.obs_ray).min() >= 2
    assert all(len(r[1]) <= THREADS for r in _run_lengths(sc))


# ---- values: both scenes against the long-double system -------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1e-2, 1e4])
@pytest.mark.parametrize("kind", ["runlens", "trips"])
def test_values_against_the_reference(pkg, kind, radius):
    S, b, diag_c, info = _solo(pkg, kind, radius)
    ref = _ref(pkg, kind, radius)
    inf = dict(zip(pkg.api.BaBatch.REDUCED_INFO, (int(v) for v in info)))
    assert su.KERNELS[inf["kernel"]] == "k_schur_f" and inf["table_global"] == 0 and inf["threads"] == THREADS, inf
    assert inf["max_cam_obs"] == np.bincount(_scene(pkg, kind).obs_cam).max()
    # (the cut recomputed here is the library's: a change of build_pairs' rule must not quietly empty the run-length conditions)
    assert inf["max_cam_run"] == max(len(r[1]) for r in _run_lengths(_scene(pkg, kind))), inf
    assert np.isfinite(S).all() and np.isfinite(b).all() and np.array_equal(S, S.T)
    rS, rb = su.ratios(S, b, ref["S"], ref["b"], ref["Y"], ref["Yb"])
    print("SCHURF %s r=%g np=%d S=%.3f b=%.3f (units of 2^-52, bound %d)" % (kind, radius, inf["np"], rS, rb, su.K))
    assert (S[ref["zero"]] == 0.0).all(), int((S[ref["zero"]] != 0).sum())
    assert rS <= su.K and rb <= su.K, (rS, rb)


# ---- bits: the table's home, the residency switch, the scene's place in a batch ---------------------------------------------
@pytest.mark.parametrize("radius", [1e-2, 1e4])
@pytest.mark.parametrize("kind", ["runlens", "trips"])
def test_table_in_global_memory_has_the_same_bits(pkg, monkeypatch, kind, radius):
    monkeypatch.setenv("PTZ_BA_SCHUR_GLOBAL_T", "1")
    got = _device(pkg, [kind], 0, radius)
    assert int(got[3][0]) == 2 and int(got[3][1]) == 1, got[3]
    _same(got, _solo(pkg, kind, radius), "global table")


@pytest.mark.parametrize("kind", ["runlens", "trips", "band"])
def test_three_workgroups_per_compute_unit_have_the_same_bits(pkg, monkeypatch, kind):
    got = {}
    for v in ("0", "1"):
        monkeypatch.setenv("PTZ_BA_SCHUR_WG4", v)
        got[v] = _device(pkg, [kind], 0, 1e4)
        assert int(got[v][3][0]) == 2 and int(got[v][3][1]) == 0, got[v][3]
    _same(got["0"], got["1"], "wg4")
    _same(got["1"], _solo(pkg, kind, 1e4), "wg4 default")


@pytest.mark.parametrize("kind", ["runlens", "trips"])
def test_first_and_last_of_a_batch_have_the_bits_of_the_scene_alone(pkg, kind):
    """The last scene owns the final run of the batch's entry array: a chunk that read past its run would read past the array."""
    other = "trips" if kind == "runlens" else "runlens"
    solo = _solo(pkg, kind, 1e4)
    first = _device(pkg, [kind, other, "edges"], 0, 1e4)
    last = _device(pkg, ["edges", other, kind], 2, 1e4)
    assert int(first[3][0]) == 2 and int(last[3][0]) == 2
    _same(first, solo, "first of three")
    _same(last, solo, "last of three")


# ---- a whole solve ----------------------------------------------------------------------------------------------------------
def test_batch_solve_has_the_bits_of_the_solo_solves(pkg):
    kinds = ["runlens", "trips", "edges"]
    opt = dict(max_num_iterations=6)

    def solve(ks):
        b = pkg.api.BaBatch([_scene(pkg, k) for k in ks], **opt)
        b.set_state()
        summ = b.solve()
        cams, _ = b.get_state()
        b.close()
        return summ, cams

    summ, cams = solve(kinds)
    for i, k in enumerate(kinds):
        s1, c1 = solve([k])
        assert s1[0]["num_iterations"] > 0 and np.isfinite(c1[0]).all(), (k, s1[0])
        assert summ[i] == s1[0], (k, summ[i], s1[0])
        assert np.array_equal(_bits(cams[i]), _bits(c1[0])), (k, float(np.abs(cams[i] - c1[0]).max()))
