"""The rotation-and-focal gate's contract without a GPU: the host instantiation of ptz_rotfocal.h against the numpy restatement, the
degenerate inputs, recovery on generated queries, the query the homography estimator's iteration bound loses, and the header under the
sanitizers as a stand-alone program."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rotfocal_util as ru

SIZES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 2049, 5000)
ITERS = (1, 2, 128, 129)
ANCHORS = {"virtual": ru.VIRTUAL, "real": ru.REAL}


def same(h, r, n):
    """every output of the harness equals the restatement's: flag, count, and under a model the model, H and mask, bit for bit"""
    assert h["found"] == r["found"] and h["best_count"] == r["best_count"], (h["found"], r["found"], h["best_count"], r["best_count"])
    if r["found"]:
        assert np.array_equal(h["model"], r["model"]) and np.array_equal(h["H"], r["H"], equal_nan=True)
        assert np.array_equal(h["mask"], r["mask"]) and int(h["mask"].sum()) == h["best_count"] and len(h["mask"]) == n


def valid(h):
    """no NaN in an output flagged valid: the model always; H is finite or nine NaN as a whole"""
    if h["found"]:
        assert np.isfinite(h["model"]).all() and h["best_count"] >= 3
        assert np.isfinite(h["H"]).all() or np.isnan(h["H"]).all()
        if np.isfinite(h["H"]).all():
            assert h["H"][8] == 1.0


@pytest.mark.parametrize("anchor", sorted(ANCHORS))
@pytest.mark.parametrize("n", SIZES)
def test_harness_equals_restatement(n, anchor):
    cam = ANCHORS[anchor]
    q = ru.make_query(n, 0.3, seed=5, cam_a=cam)
    for iters in ITERS:
        h = ru.harness_find(q["uv_a"], q["uv_b"], cam, q["cxq"], q["cyq"], 4.0, iters)
        r = ru.find(q["uv_a"], q["uv_b"], cam, q["cxq"], q["cyq"], 4.0, iters)
        same(h, r, n)
        valid(h)
        assert h["found"] == (1 if n >= 3 and r["best_count"] >= 3 else 0)
    if n >= 63:
        assert h["found"] == 1


def test_sample_is_a_function_of_iteration_and_size():
    ij = np.zeros(2, dtype=np.int32)
    for n in (2, 3, 64, 1000, 2 ** 31 - 1):
        for it in (0, 1, 127, 4095):
            ru.harness().h_rotfocal_sample(it, n, ij.ctypes.data_as(C.c_void_p))
            assert tuple(ij) == ru.sample(it, n) and ij[0] != ij[1] and 0 <= ij.min() and ij.max() < n


def degenerate_cases():
    out = {}
    for name, cam in ANCHORS.items():
        q = ru.make_query(64, 0.0, seed=9, cam_a=cam)
        a, b = q["uv_a"], q["uv_b"]
        out["same-pixel-" + name] = (np.tile(a[:1], (64, 1)), np.tile(b[:1], (64, 1)), cam)
        out["two-identical-" + name] = (np.tile(a[:1], (2, 1)), np.tile(b[:1], (2, 1)), cam)
        out["equal-query-pixels-" + name] = (a, np.tile(b[:1], (64, 1)), cam)
        out["parallel-rays-" + name] = (np.tile(a[:1], (64, 1)), b, cam)
        a1, b1 = a.copy(), b.copy()
        a1[3, 0] = np.nan; b1[10, 1] = np.inf; a1[20, 0] = -np.inf
        out["nan-inf-pixels-" + name] = (a1, b1, cam)
        a2 = a.copy()
        a2[:, 0] = (cam[2] + 1e7 * (np.random.default_rng(4).random(64) - 0.5)).astype(np.float32)
        out["near-image-plane-" + name] = (a2, b, cam)
    return out


DEGENERATE = degenerate_cases()


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_inputs(name):
    a, b, cam = DEGENERATE[name]
    for iters in (1, 128):
        h = ru.harness_find(a, b, cam, 960.0, 540.0, 4.0, iters)
        r = ru.find(a, b, cam, 960.0, 540.0, 4.0, iters)
        same(h, r, len(a))
        valid(h)
    if name.startswith(("same-pixel", "two-identical", "parallel-rays")):
        assert h["found"] == 0 and h["best_count"] == -1  # X = 0 in every sample: no hypothesis at all
    if name.startswith("nan-inf"):
        assert h["found"] == 1 and 3 <= h["best_count"] <= 61 and not h["mask"][[3, 10, 20]].any()


def test_matches_behind_the_camera_are_no_inliers():
    """a model that maps a match to m_z <= 0 does not count it, whatever its pixel error: the query's matches mirrored through the
    anchor's centre satisfy the pixel equation of the true model with m_z < 0"""
    cam = ru.VIRTUAL
    q = ru.make_query(64, 0.0, seed=2, cam_a=cam, noise=0.0)
    r = ru.find(q["uv_a"], q["uv_b"], cam, q["cxq"], q["cyq"])
    assert r["found"] and r["best_count"] == 64
    L = ru.lift(q["uv_a"], q["uv_b"], cam, q["cxq"], q["cyq"])
    h = ru.harness_find(q["uv_a"], q["uv_b"], cam, q["cxq"], q["cyq"])
    assert h["found"] and np.array_equal(h["model"], r["model"])
    m = h["model"].copy()
    m[1:] = -m[1:]  # R a -> -R a: the same pixel, behind the camera
    hm = ru.harness_inliers(m, q["uv_a"], q["uv_b"], cam, q["cxq"], q["cyq"])  # the header's host instantiation
    assert not hm.any() and np.array_equal(hm, ru.inliers(m, L, 4.0))
    m[1:] = -m[1:]
    hp = ru.harness_inliers(m, q["uv_a"], q["uv_b"], cam, q["cxq"], q["cyq"])
    assert hp.all() and np.array_equal(hp, ru.inliers(m, L, 4.0))


def test_two_positive_roots_tie_goes_to_the_lower_number():
    """Four matches and one iteration.  The two sample matches lie nearly on a line through the query's centre, on the same side of it, so
    the quadratic has two positive roots (c > 0, b < 0) and both pass the sign test (q_i . q_j > 0); either model reproduces its two sample matches, the
    third match copies the first sample match and the fourth is wrong.  Both hypotheses count 3: number 0 must win."""
    cam = ru.VIRTUAL
    i, j = ru.sample(0, 4)
    rest = [k for k in range(4) if k not in (i, j)]
    q = ru.make_query(4, 0.0, seed=1, cam_a=cam, noise=0.0)
    ub = np.zeros((4, 2))
    ub[i], ub[j] = [960.0 + 300.0, 540.0 + 100.0], [960.0 + 600.0, 540.0 + 210.0]
    ub[rest[0]] = ub[i]
    ub[rest[1]] = [100.0, 1000.0]
    ua = ru.to_anchor(ub, q["f_true"], q["R_true"], cam, 960.0, 540.0)
    ua[rest[1]] += [700.0, -300.0]
    ua, ub = ua.astype(np.float32), ub.astype(np.float32)
    L = ru.lift(ua, ub, cam, 960.0, 540.0)
    m0, m1 = ru.hypothesis(L[i], L[j], 0), ru.hypothesis(L[i], L[j], 1)
    assert m0 is not None and m1 is not None and m0[0] != m1[0]
    assert int(ru.inliers(m0, L, 4.0).sum()) == 3 and int(ru.inliers(m1, L, 4.0).sum()) == 3
    h = ru.harness_find(ua, ub, cam, 960.0, 540.0, 4.0, 1)
    r = ru.find(ua, ub, cam, 960.0, 540.0, 4.0, 1)
    same(h, r, 4)
    assert h["found"] == 1 and h["best_count"] == 3 and r["best_h"] == 0 and np.array_equal(h["model"], m0)


RECOVERY = [(n, w, s) for n in (128, 1000) for w in (0.0, 0.3, 0.5) for s in range(4)]


@pytest.mark.parametrize("n,wrong,seed", RECOVERY, ids=lambda v: str(v))
def test_recovery(n, wrong, seed):
    """the prototype's generator: 1920 x 1080 query, virtual anchor fa = 1500, S = 8192, 0.5 px noise in both images, threshold 4 px"""
    q = ru.make_query(n, wrong, seed)
    h = ru.harness_find(q["uv_a"], q["uv_b"], ru.VIRTUAL, q["cxq"], q["cyq"], 4.0, 128)
    assert h["found"] == 1
    good = ~q["wrong"]
    kept_good, kept_wrong = int(h["mask"][good].sum()), int(h["mask"][q["wrong"]].sum())
    ferr = abs(h["model"][0] - q["f_true"]) / q["f_true"]
    print("n %d wrong %.1f seed %d: %d / %d true inliers, %d wrong kept, focal error %.2e" % (n, wrong, seed, kept_good, int(good.sum()), kept_wrong, ferr))
    assert kept_good >= 0.98 * int(good.sum())
    assert kept_wrong <= max(2, n // 100)
    assert ferr < 1e-2


# seed of make_query(1000, 0, seed) on which the 4-point homography estimator's adaptive bound overflows after a first model of 1 to 7
# inliers and the estimator ends with fewer than 6 inliers of 1000 true matches (a search over seeds 0 .. 399 finds two: 250 and 305, both with 4 inliers)
OVERFLOW_SEED = 250


def test_query_the_homography_bound_loses():
    q = ru.make_query(1000, 0.0, OVERFLOW_SEED)
    hh = C.CDLL(os.path.join(ru.ROOT, "tests", "cpu_harness", "libhomography_harness.so"))
    H, mask = np.zeros(9), np.zeros(1000, dtype=np.uint8)
    found = hh.h_find_homography(1000, ru._p(q["uv_a"]), ru._p(q["uv_b"]), C.c_double(4.0), ru._p(H), ru._p(mask))
    assert (int(mask.sum()) if found else 0) < 6
    h = ru.harness_find(q["uv_a"], q["uv_b"], ru.VIRTUAL, q["cxq"], q["cyq"], 4.0, 128)
    assert h["found"] == 1 and int(h["mask"].sum()) >= 980


def test_header_under_sanitizers(tmp_path):
    """the header's host instantiation as a stand-alone program built with the address and undefined-behaviour sanitizers"""
    exe = str(tmp_path / "rotfocal_harness_main")
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DROTFOCAL_HARNESS_MAIN", "-o", exe, ru.HARNESS_SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout
