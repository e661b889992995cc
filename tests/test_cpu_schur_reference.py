"""The yardstick of test_gpu_schur_direct.py, checked without a GPU (schur_ref_util.py): the long-double reduced camera system is
exact to far below the bound, float64 numpy passes every case the GPU test runs with a factor 8 to spare -- the measurement the
bound's constant K is derived from -- and the reference reacts to the bugs the test exists for.  Inputs: the oracle's analytic
linearisation at the scenes' initial state (the GPU test takes the device's; the dummy fy column is dropped as in
test_linearize_vs_oracle)."""
import numpy as np
import pytest

import schur_ref_util as su

_LIN = {}


def _lin(pkg, orc, kind, ftype):
    key = (kind, ftype)
    if key not in _LIN:
        sc = su.scene(pkg, kind, ftype)
        _LIN[key] = (sc, su.drop_dummy_fy(orc.ba_linearize(sc, sc.cam_init, sc.ray_init), ftype))
    return _LIN[key]


def _inputs(pkg, orc, kind, ftype, clamps):
    sc, lin = _lin(pkg, orc, kind, ftype)
    s_c, s_r = su.scales(sc, lin["U"].shape[1], 7)
    lo, hi = su.lm_clamps(lin, s_c) if clamps == "inside" else (su.MIN_DIAG, su.MAX_DIAG)
    return sc, lin, s_c, s_r, lo, hi


@pytest.mark.parametrize("ftype", [0, 1, 2])
def test_long_double_reference_is_exact(pkg, orc, ftype):
    """5 cameras, 30 rays: long double against the same formula at 50 digits, to 1e-17 of the yardstick, on every rung."""
    sc, lin, s_c, s_r, lo, hi = _inputs(pkg, orc, "small5", ftype, None)
    assert sc.n_cam == 5 and sc.n_ray == 30
    for radius in su.RADII:
        S, b, Y, Yb, _, kappa = su.system(lin, sc.obs_cam, sc.obs_ray, s_c, s_r, radius)
        Sm, bm = su.mp_system(lin, sc.obs_cam, sc.obs_ray, s_c, s_r, radius)
        eS = float((np.abs(S - su.mp_to_ld(Sm)) / Y).max())
        eb = float((np.abs(b - su.mp_to_ld(bm)) / Yb).max())
        print("SCHURREF exact type=%d r=%g kappa_max=%.2e |S_ld - S_mp|/Y=%.2e |b_ld - b_mp|/Yb=%.2e" % (ftype, radius, kappa.max(), eS, eb))
        assert eS <= 1e-17 and eb <= 1e-17, (radius, eS, eb)


def test_float64_numpy_passes_every_gpu_case_with_a_factor_8_to_spare(pkg, orc):
    """|S_float64 - S_longdouble| / Y over every system of the GPU test: the worst is what K is 8 times of, rounded up to a power of
    two.  (The two scale LAPACKs apart: K may be up to twice tighter than the rule asks, never looser than a factor 8.)"""
    worst = 0.0
    for kind, ftype, radius, clamps in su.numeric_cases():
        sc, lin, s_c, s_r, lo, hi = _inputs(pkg, orc, kind, ftype, clamps)
        S, b, Y, Yb, _, kappa = su.system(lin, sc.obs_cam, sc.obs_ray, s_c, s_r, radius, lo, hi)
        S64, b64, _, _, _, _ = su.system(lin, sc.obs_cam, sc.obs_ray, s_c, s_r, radius, lo, hi, dtype=np.float64)
        rS, rb = su.ratios(S64, b64, S, b, Y, Yb)
        print("SCHURSTAT numpy %s type=%d r=%g clamps=%s n=%d kappa_max=%.2e S=%.3f b=%.3f" % (kind, ftype, radius, clamps, len(b), kappa.max(), rS, rb))
        assert max(rS, rb) <= su.K / 8.0, (kind, ftype, radius, rS, rb)
        worst = max(worst, rS, rb)
    print("SCHURSTAT numpy worst ratio %.4f (K = %d)" % (worst, su.K))
    assert su.K == 2 ** int(np.ceil(np.log2(8.0 * su.NUMPY_WORST_RATIO)))
    assert 0.5 * su.NUMPY_WORST_RATIO <= worst <= 2.0 * su.NUMPY_WORST_RATIO, worst


@pytest.mark.parametrize("ftype", [0, 1, 2])
def test_reference_reacts_to_the_bugs_the_test_is_for(pkg, orc, ftype):
    """The small-radius rung of the scene with the observation-count edges, the pair with the MOST entries (cameras 10 and 11, 769
    common rays): one entry dropped from its sum, the two cameras' Jacobi scales swapped, E without the LM term -- each must move
    some entry by at least 1000 times the bound."""
    sc, lin, s_c, s_r, lo, hi = _inputs(pkg, orc, "edges", ftype, None)
    radius = su.RADII[0]
    S, b, Y, Yb, _, _ = su.system(lin, sc.obs_cam, sc.obs_ray, s_c, s_r, radius)
    bound = su.K * su.EPS * Y
    a = int(np.nonzero((sc.obs_cam == 10) & (sc.obs_ray == 400))[0][0])
    e = int(np.nonzero((sc.obs_cam == 11) & (sc.obs_ray == 400))[0][0])
    for name, kw in (("drop", dict(drop=(a, e))), ("swap", dict(swap=(10, 11))), ("no_lm", dict(no_lm=True))):
        Sp = su.system(lin, sc.obs_cam, sc.obs_ray, s_c, s_r, radius, **kw)[0]
        live = bound > 0  # (a non-finite entry, as a singular V' without its LM term may give, counts as moved)
        worst = float(np.where(np.isfinite(Sp[live]), np.abs(Sp[live] - S[live]) / bound[live], np.inf).max())
        print("SCHURREF sensitivity type=%d %s: largest move %.3e bounds" % (ftype, name, worst))
        assert worst >= 1000.0, (name, worst)
