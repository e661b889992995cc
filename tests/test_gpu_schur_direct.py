"""The reduced camera system S y = b as k_ray_prep and the three Schur kernels (k_schur_f, k_schur, k_schur_w) leave it, read
through BaBatch.reduced_system / ptz_debug_batch_reduced_system -- the solver's own prologue and first-pass launches, shared code --
and held entrywise to the long-double system of schur_ref_util.py.

Every case reads the UNSCALED linearisation from one batch (linearize) and the system from a second, fresh batch of the same
scenes (no materialised W row can steer anything), with seeded Jacobi scales that differ per column (cameras [1e-3, 1], rays
[1e-2, 1]) and the system's block poisoned with 0xFF bytes.  It asserts: info names the expected kernel and configuration; no NaN;
|S - S_ref| <= K 2^-52 Y and the same for b (K and the yardstick Y: schur_ref_util.py, derived from float64 numpy, not from the
kernels); diag_c against the clamp of diag U'; EXACT 0.0 wherever two cameras share no ray, inside and outside the tile mask.

Measured on one MI355X, largest |S - S_ref| / Y, the same over the blocks OFF the diagonal alone, and |b - b_ref| / Yb, per path
over all its cases, in units of 2^-52 (the bound is K = 128; numpy: float64 on the oracle's linearisation of the same scenes,
test_cpu_schur_reference.py; the two table homes give the same figures, the three elimination orders the same bits):

    path                         r = 1e-2               r = 1e4                r = 1e8
    numpy float64                9.35 / 0.10 / 6.82     0.21 / 0.00 / 0.00     0.20 / 0.00 / 0.00
    k_schur_f  PTZRay            3.68 / 0.17 / 1.03     0.80 / 0.00 / 0.00     0.51 / 0.00 / 0.00
    k_schur    PTZRay            3.68 / 0.09 / 1.03     0.80 / 0.00 / 0.00     0.51 / 0.00 / 0.00
    k_schur    PTZRayDist        8.55 / 0.14 / 1.38     0.80 / 0.00 / 0.00     0.51 / 0.00 / 0.00
    k_schur    PTZRayFxfyDist    2.90 / 0.31 / 1.53     0.80 / 0.00 / 0.00     0.51 / 0.00 / 0.00
    k_schur_w  PTZRay            3.68 / 0.07 / 1.03     0.80 / 0.00 / 0.00     0.51 / 0.00 / 0.00
    k_schur_w  PTZRayDist        8.55 / 0.12 / 1.38     0.80 / 0.00 / 0.00     0.51 / 0.00 / 0.00

The largest figures sit on the diagonal blocks, where U' (k_lin_cam sums the scaled Jacobians, the reference scales the unscaled sum)
and D^2 = sqrt(d / r)^2 weigh as much as the kernels' own sums: hence one value for all kernels of a type.  0.80 and 0.51 are the
D^2 of the camera without observations (three roundings against the reference's one).  Off the diagonal the kernels stay a factor
400 and more inside the bound: kappa_j (median 50 .. 400, largest 1e5 .. 1e7 at r = 1e-2 with these ray scales; ~r above) makes the
yardstick generous there,
which is the price of a bound that float64 can meet at all; test_cpu_schur_reference.py shows what it still catches (one entry of
769 dropped from a pair's sum: 1e7 bounds).  At r = 1e8 kappa is 1e12 .. 1e14 and the bound is of the order of the terms: that rung
holds structure (NaN, zeros, diagonal, kernel), not values -- profiles/NOTES_schur_direct.md, where a build with the wrong camera's
scales in the pair blocks fails every k_schur / k_schur_f case at 1e-2 and 1e4 and none at 1e8.  Over a whole system no path needs more than numpy's own ratio; off the diagonal the kernels
are at up to three times numpy's 0.10, the factor their extra roundings per term predict.

Scenes (schur_ref_util.scene): `edges`, one camera each with 0, 1, 2, 63, 64, 65, 255, 256, 257, 512, 769 and 800 observations
(the kernels stride 256 threads over a camera's observations, k_schur_f with three prefetched trips); `band`, 40 cameras, whose
camera 12 (PTZRayDist, columns 60-64) and camera 10 (PTZRayFxfyDist, 60-65) straddle the first tile edge; `ring`, 128 / 104 / 86
cameras on a full circle -- the planner dissects a ring only from six free tiles on, which 40 cameras (three tiles at most) never
reach, so the non-identity order is asserted there and the 40-camera scene runs under the same three orders beside it; `rounds`,
258 cameras sharing six rays (more runs of one camera than the workgroup has threads); three scenes of different sizes in one batch.

Out of scope: annotation rows (k_schur_3d), the shared-intrinsics fold (k_group_diag, k_fold_system), PTZRayDistDisp -- their
reference terms are not among what linearize returns -- and compacted launch shapes (the entry launches shape 0)."""
import numpy as np
import pytest

import schur_ref_util as su

pytestmark = pytest.mark.gpu

_LIN, _REF = {}, {}
SCALE_SEED = 7


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _lin(pkg, kind, ftype):
    """The device's unscaled linearisation of the scene at its initial state, from a batch of its own, once per process."""
    key = (kind, ftype)
    if key not in _LIN:
        sc = su.scene(pkg, kind, ftype)
        b = pkg.api.BaBatch([sc])
        b.set_state()
        lin = b.linearize(0)
        b.close()
        assert lin["nc"] == lin["W"].shape[1]
        _LIN[key] = (sc, {k: lin[k] for k in ("U", "g_c", "V", "g_r", "W")}, su.scales(sc, lin["nc"], SCALE_SEED))
    return _LIN[key]


def _clamps(pkg, kind, ftype, clamps):
    sc, lin, (s_c, s_r) = _lin(pkg, kind, ftype)
    return su.lm_clamps(lin, s_c) if clamps == "inside" else (su.MIN_DIAG, su.MAX_DIAG)


def _ref(pkg, kind, ftype, radius, clamps=None):
    key = (kind, ftype, radius, clamps)
    if key not in _REF:
        sc, lin, (s_c, s_r) = _lin(pkg, kind, ftype)
        lo, hi = _clamps(pkg, kind, ftype, clamps)
        S, b, Y, Yb, diag_c, kappa = su.system(lin, sc.obs_cam, sc.obs_ray, s_c, s_r, radius, lo, hi)
        _REF[key] = dict(S=S, b=b, Y=Y, Yb=Yb, diag_c=diag_c, kappa=kappa, zero=~su.shares_ray(sc, lin["U"].shape[1]), lo=lo, hi=hi)
    return _REF[key]


def _device(pkg, kinds, ftype, index, radius, lo=su.MIN_DIAG, hi=su.MAX_DIAG, poison=True):
    """The system of scene `index` of a FRESH batch of the scenes `kinds`."""
    scenes = [su.scene(pkg, k, ftype) for k in kinds]
    _, _, (s_c, s_r) = _lin(pkg, kinds[index], ftype)
    b = pkg.api.BaBatch(scenes, initial_trust_region_radius=radius, min_lm_diagonal=lo, max_lm_diagonal=hi)
    b.set_state()
    out = b.reduced_system(index, s_c, s_r, poison=poison)
    b.close()
    return out


def _info(info):
    return dict(zip(("kernel", "table_global", "np", "n_tiles", "reordered", "max_cam_obs", "max_cam_run", "threads"), (int(v) for v in info)))


def _hold(pkg, tag, kind, ftype, radius, got, kernel, clamps=None):
    """The assertions every case makes of one system (S, b, diag_c, info)."""
    S, b, diag_c, info = got
    ref = _ref(pkg, kind, ftype, radius, clamps)
    sc, lin, (s_c, s_r) = _lin(pkg, kind, ftype)
    inf = _info(info)
    assert inf["kernel"] == kernel, (tag, inf)
    assert np.isfinite(S).all() and np.isfinite(b).all() and np.isfinite(diag_c).all(), tag
    assert np.array_equal(S, S.T)
    rS, rb = su.ratios(S, b, ref["S"], ref["b"], ref["Y"], ref["Yb"])
    # (the blocks off the diagonal apart: they are the Schur kernels' alone, the diagonal ones also carry U' and D^2 of k_lin_cam)
    off = ~np.kron(np.eye(sc.n_cam, dtype=bool), np.ones((lin["U"].shape[1],) * 2, dtype=bool))
    rO = su.ratios(S[off], b, ref["S"][off], ref["b"], ref["Y"][off], ref["Yb"])[0]
    print("SCHURSTAT %s %s %s type=%d r=%g n=%d np=%d tg=%d reordered=%d kappa_max=%.2e S=%.3f S_offdiag=%.3f b=%.3f" %
          (su.KERNELS[kernel], tag, kind, ftype, radius, len(b), inf["np"], inf["table_global"], inf["reordered"], ref["kappa"].max(), rS, rO, rb))
    assert (S[ref["zero"]] == 0.0).all(), (tag, int((S[ref["zero"]] != 0).sum()))
    # diag_c: the device sums the squares of the SCALED Jacobian's entries, the reference scales the unscaled sum.  Per term two
    # roundings more on one side (<= 1.5 ulp of the sum of positive terms); k_lin_cam sums m terms over 64 lanes and a six-level
    # butterfly, ceil(m / 64) + 6 additions deep, each within half an ulp of the total, on either side.  A clamped entry is exact.
    m = np.bincount(sc.obs_cam, minlength=sc.n_cam)
    ulps = (3 + np.ceil(m / 64.0) + 6)[:, None]
    want = ref["diag_c"].astype(np.float64)
    assert (np.abs(diag_c - want) <= ulps * np.spacing(want)).all(), (tag, float((np.abs(diag_c - want) / np.spacing(want)).max()))
    assert rS <= su.K and rb <= su.K, (tag, rS, rb)
    return inf


# ---- every kernel and both homes of the table, on the observation-count edges and on the straddling blocks ----------------
@pytest.mark.parametrize("radius", su.RADII)
@pytest.mark.parametrize("tg", [0, 1])
@pytest.mark.parametrize("path", su.PATHS, ids=lambda p: "type%d-%s" % (p[0], su.KERNELS[p[1]]))
@pytest.mark.parametrize("kind", ["edges", "band"])
def test_every_kernel_and_table_home(pkg, monkeypatch, kind, path, tg, radius):
    ftype, kernel, env = path
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PTZ_BA_SCHUR_GLOBAL_T", str(tg))
    sc = su.scene(pkg, kind, ftype)
    if kind == "edges":
        assert np.bincount(sc.obs_cam, minlength=12).tolist() == su.EDGE_COUNTS
        assert np.bincount(sc.obs_ray).min() >= 2
    else:
        assert sc.n_cam == 40 and np.bincount(sc.obs_cam, minlength=40).min() > 0
    inf = _hold(pkg, "tg%d" % tg, kind, ftype, radius, _device(pkg, [kind], ftype, 0, radius), kernel)
    assert inf["table_global"] == tg and inf["threads"] == 256
    assert inf["max_cam_obs"] == np.bincount(sc.obs_cam).max()
    assert inf["n_tiles"] * 64 == inf["np"] > sc.n_cam * [4, 5, 6][ftype]


# ---- blocks that straddle a tile under the planner's order, the natural order and the dense path ---------------------------
@pytest.mark.parametrize("ftype", [0, 1, 2])
@pytest.mark.parametrize("kind", ["band", "ring"])
def test_elimination_orders_leave_the_same_bits(pkg, monkeypatch, kind, ftype):
    sc = su.scene(pkg, kind, ftype)
    nc = [4, 5, 6][ftype]
    if ftype:  # a camera block across the first tile edge (type 0 is the tile-aligned control)
        cam = {1: 12, 2: 10}[ftype]
        assert cam * nc < 64 <= cam * nc + nc - 1
    kernel = 2 if ftype == 0 else 1
    got = {}
    for name, env in (("planner", {}), ("natural", {"PTZ_BA_ORDER": "natural"}), ("dense", {"PTZ_BA_DENSE_CHOL": "1"})):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            got[name] = _device(pkg, [kind], ftype, 0, 1e4)
        inf = _hold(pkg, name, kind, ftype, 1e4, got[name], kernel)
        if name == "planner" and kind == "ring":
            assert sc.n_cam == su.RING_CAMS[ftype] and inf["n_tiles"] >= 8
            assert inf["reordered"] == 1, inf
        if name != "planner":
            assert inf["reordered"] == 0, inf
    for name in ("natural", "dense"):
        assert np.array_equal(_bits(got[name][0]), _bits(got["planner"][0])), (name, np.abs(got[name][0] - got["planner"][0]).max())
        assert np.array_equal(_bits(got[name][1]), _bits(got["planner"][1])), name
        assert np.array_equal(_bits(got[name][2]), _bits(got["planner"][2])), name


# ---- more runs than threads -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", su.RADII)
@pytest.mark.parametrize("path", su.PATHS[:2], ids=lambda p: su.KERNELS[p[1]])
def test_more_runs_than_threads(pkg, monkeypatch, path, radius):
    """Camera 257 has 257 lower-numbered partners, one more than the workgroup has threads (runs never straddle two pairs): the
    kernel takes several rounds, with the table in global memory."""
    ftype, kernel, env = path
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = su.scene(pkg, "rounds", ftype)
    assert sc.n_cam == 258 and sc.n_ray == 6 and (np.bincount(sc.obs_ray) == 258).all()
    inf = _hold(pkg, "rounds", "rounds", ftype, radius, _device(pkg, ["rounds"], ftype, 0, radius), kernel)
    assert inf["threads"] == 256 and sc.n_cam - 1 == inf["threads"] + 1
    assert inf["max_cam_run"] > inf["threads"] and inf["table_global"] == 1, inf


# ---- clamps of the LM diagonal that bite ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ftype", [0, 1, 2])
def test_lm_diagonal_clamps_inside_the_range(pkg, ftype):
    sc, lin, (s_c, s_r) = _lin(pkg, "trio1", ftype)
    lo, hi = _clamps(pkg, "trio1", ftype, "inside")
    nc = lin["U"].shape[1]
    dg = s_c * s_c * lin["U"][:, np.arange(nc), np.arange(nc)]
    assert (dg < lo).any() and (dg > hi).any() and ((dg > lo) & (dg < hi)).any(), (lo, hi)
    got = _device(pkg, ["trio1"], ftype, 0, 1e4, lo, hi)
    _hold(pkg, "clamps", "trio1", ftype, 1e4, got, 2 if ftype == 0 else 1, "inside")
    assert (got[2][dg < lo * (1 - 1e-12)] == lo).all() and (got[2][dg > hi * (1 + 1e-12)] == hi).all()


# ---- a scene's system does not depend on the batch it is in ------------------------------------------------------------------
@pytest.mark.parametrize("ftype", [0, 1, 2])
def test_batch_of_three_has_the_bits_of_each_scene_alone(pkg, ftype):
    kinds = ["trio0", "trio1", "trio2"]
    kernel = 2 if ftype == 0 else 1
    sizes = [su.scene(pkg, k, ftype).n_cam for k in kinds]
    assert len(set(sizes)) == 3
    for i, kind in enumerate(kinds):
        solo = _device(pkg, [kind], ftype, 0, 1e4)
        both = _device(pkg, kinds, ftype, i, 1e4)
        _hold(pkg, "solo", kind, ftype, 1e4, solo, kernel)
        _hold(pkg, "batch", kind, ftype, 1e4, both, kernel)
        for a, e in zip(solo[:3], both[:3]):
            assert np.array_equal(_bits(a), _bits(e)), (kind, np.abs(a - e).max())
    # the last scene's camera 0 has no observation: U = 0, its diagonal block is D^2 alone, from the clamped minimum
    sc = su.scene(pkg, "trio2", ftype)
    assert (sc.obs_cam != 0).all()
    nc = [4, 5, 6][ftype]
    S, b, diag_c, _ = both
    assert (diag_c[0] == su.MIN_DIAG).all()
    want = su.MIN_DIAG / 1e4
    blk = S[:nc, :nc]
    assert (blk[~np.eye(nc, dtype=bool)] == 0).all() and (S[:nc, nc:] == 0).all() and (b[:nc] == 0).all()
    assert (np.abs(np.diag(blk) - want) <= 2 * np.spacing(want)).all(), np.diag(blk)  # (sqrt, square: two roundings on the quotient's)


def test_arguments(pkg):
    api = pkg.api
    sc = su.scene(pkg, "trio0", 0)
    b = api.BaBatch([sc])
    with pytest.raises(api.PtzError) as e:
        b.reduced_system(0)  # no state yet
    assert e.value.code == -1
    b.set_state()
    with pytest.raises(api.PtzError) as e:
        b.reduced_system(1)
    assert e.value.code == -1
    S0, b0, d0, i0 = b.reduced_system(0, poison=True)
    S1, b1, d1, i1 = b.reduced_system(0, poison=False)  # repeated, unpoisoned: unit scales, the same bits
    assert np.array_equal(_bits(S0), _bits(S1)) and np.array_equal(_bits(b0), _bits(b1)) and np.array_equal(i0, i1)
    summ = b.solve()  # the batch is still good for a solve, which starts over from the stored state
    ref = api.ba_solve(sc)[2]
    assert summ[0]["termination_type"] == 0 and summ[0]["final_cost"] == ref["final_cost"] and summ[0]["num_iterations"] == ref["num_iterations"]
    b.close()
    d3 = api.BaBatch([pkg.synth.make_scene(1, 6, 30, factor_type=3)])
    d3.set_state()
    with pytest.raises(api.PtzError) as e:
        d3.reduced_system(0)
    assert e.value.code == -4  # PTZ_EUNSUPPORTED
    d3.close()
