"""CPU tests of the guided matcher's contract: the guided part of the shared header (ptz-calib_amd/csrc/ptz_desc_match.h)
instantiated on the host by tests/cpu_harness/desc_guided_harness.cc against the numpy restatement (desc_guided_util.py), the
generator of repeated descriptors, the argument errors of the C-ABI that need no device, and the guard of the chain tests: on the
rig with repeated descriptors the first pass loses and invents matches, the two-pass flow does neither."""
import ctypes as C
import os

import numpy as np
import pytest

import desc_guided_util as gu
import desc_match_util as du
import host_util as hu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_h = None

IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.float64)
_c, _s = 1.1 * np.cos(0.05), 1.1 * np.sin(0.05)
ROT_ZOOM = np.array([_c, -_s, 7.25, _s, _c, -3.5, 0, 0, 1], dtype=np.float64)
BEHIND = np.array([1, 0, 0, 0, 1, 0, -1.0 / 32, 0, 1], dtype=np.float64)  # Z = 1 - x / 32: <= 0 from x = 32 on
NAN_H = np.array([1, 0, 0, 0, np.nan, 0, 0, 0, 1], dtype=np.float64)


def harness():
    global _h
    if _h is None:
        _h = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "libdesc_guided_harness.so"))
        _h.h_desc_match_pair_guided.restype = C.c_int64
        _h.h_desc_guide_warp.restype = None
        _h.h_desc_guide_admissible.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, C.c_double]
    return _h


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness_warp(H, xy):
    xy = np.ascontiguousarray(xy, dtype=np.float32)
    H = np.ascontiguousarray(H, dtype=np.float64)
    n = len(xy)
    wx, wy, ok = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    harness().h_desc_guide_warp(_p(H), n, _p(xy), _p(wx), _p(wy), _p(ok))
    return wx, wy, ok.astype(bool)


def harness_pair(a, b, kp_a, kp_b, H, radius, ratio=0.8, max_dist2=0, cross_check=True, min_matches=0):
    a = np.ascontiguousarray(a, dtype=np.uint8); b = np.ascontiguousarray(b, dtype=np.uint8)
    kp_a = np.ascontiguousarray(kp_a, dtype=np.float32); kp_b = np.ascontiguousarray(kp_b, dtype=np.float32)
    H = np.ascontiguousarray(H, dtype=np.float64)
    na, nb, D = len(a), len(b), a.shape[1]
    ta = np.zeros((max(na, 1), 3), dtype=np.int32); tb = np.zeros((max(nb, 1), 3), dtype=np.int32)
    ia, ib, dd = (np.zeros(max(na, 1), dtype=np.int32) for _ in range(3))
    n = harness().h_desc_match_pair_guided(_p(a), na, _p(b), nb, D, _p(kp_a), _p(kp_b), _p(H), C.c_double(radius), C.c_double(ratio),
                                           int(max_dist2), int(cross_check), int(min_matches), _p(ta), _p(tb), _p(ia), _p(ib), _p(dd))
    return ta[:na], tb[:nb], ia[:n], ib[:n], dd[:n]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------- the header
@pytest.mark.parametrize("name,H", [("identity", IDENTITY), ("rot_zoom", ROT_ZOOM), ("behind", BEHIND), ("nan", NAN_H)])
def test_warp_on_host_equals_numpy(name, H):
    rng = np.random.default_rng(5)
    xy = np.concatenate([rng.uniform(0, 64, (300, 2)), np.stack(np.meshgrid(np.arange(28, 37), np.arange(3)), -1).reshape(-1, 2)]).astype(np.float32)
    wx, wy, ok = harness_warp(H, xy)
    nx, ny, nok = gu.warp(H, xy)
    assert np.array_equal(ok, nok)
    # where the warp is ok the quotients are numbers and must agree bit for bit; elsewhere both sides hold the same inf / NaN class
    assert np.array_equal(_bits(wx)[ok], _bits(nx)[ok]) and np.array_equal(_bits(wy)[ok], _bits(ny)[ok])
    assert np.array_equal(wx, nx, equal_nan=True) and np.array_equal(wy, ny, equal_nan=True)
    if name in ("identity", "rot_zoom"):
        assert ok.all()
    if name == "behind":
        assert np.array_equal(ok, xy[:, 0] < 32) and ok.any() and not ok.all()
    if name == "nan":
        assert not ok.any()


def test_inclusive_bound_on_integer_pixels():
    """identity H, offset (3, 4): e2 = 25 exactly; radius 5 admits it, the double just below 5 does not, a NaN never"""
    adm = harness().h_desc_guide_admissible
    below = float(np.nextafter(np.float32(5.0), np.float32(0.0)))  # r2f of it is the float32 below 25
    assert gu.r2f_of(5.0) == np.float32(25.0) and gu.r2f_of(below) < np.float32(25.0)
    wx, wy, ok = harness_warp(IDENTITY, np.array([[10, 20]], dtype=np.float32))
    assert ok[0] and wx[0] == 10 and wy[0] == 20
    assert adm(wx[0], wy[0], 13.0, 24.0, 5.0) == 1 and adm(wx[0], wy[0], 13.0, 24.0, below) == 0
    assert adm(float("nan"), wy[0], 13.0, 24.0, 1e9) == 0 and adm(wx[0], wy[0], 13.0, float("nan"), 1e9) == 0
    a = np.array([[10, 20]], dtype=np.float32); b = np.array([[13, 24]], dtype=np.float32)
    assert gu.admissible(IDENTITY, a, b, 5.0)[0, 0] and not gu.admissible(IDENTITY, a, b, below)[0, 0]
    d = np.zeros((1, 8), dtype=np.uint8)
    assert harness_pair(d, d, a, b, IDENTITY, 5.0, ratio=0.0)[2].tolist() == [0]
    assert harness_pair(d, d, a, b, IDENTITY, below, ratio=0.0)[2].tolist() == []


def _points(rng, na, nb, H):
    """A's key points on integer pixels of a small window; B's: the warped point of one of A's plus an integer offset of a few
    pixels (so that under the identity distances hit the bound exactly and repeat), a few far away."""
    kp_a = rng.integers(0, 40, (na, 2)).astype(np.float32)
    wx, wy, ok = gu.warp(H, kp_a)
    src = rng.integers(0, na, nb)
    base = np.where(ok[src, None], np.stack([wx, wy], 1)[src], kp_a[src])
    kp_b = (base + rng.integers(-4, 5, (nb, 2))).astype(np.float32)
    far = rng.random(nb) < 0.1
    kp_b[far] += 500
    return kp_a, kp_b


@pytest.mark.parametrize("D", (1, 128, 130))
def test_guided_header_on_host_equals_numpy(D):
    """top-2 over the admissible candidates and the accepted matches, every size, radius and option set; at the open radius the
    result is the unguided restatement's (ties at D = 1, where values repeat)"""
    rng = np.random.default_rng(100 + D)
    hs = (IDENTITY, ROT_ZOOM, BEHIND)
    for na in gu.SIZES:
        for nb in gu.SIZES:
            a = rng.integers(0, 4 if D == 1 else 256, (na, D), dtype=np.uint8)
            b = rng.integers(0, 4 if D == 1 else 256, (nb, D), dtype=np.uint8)
            k = min(na, nb) // 2
            if k and D > 1:
                b[rng.permutation(nb)[:k]] = np.clip(a[rng.permutation(na)[:k]].astype(np.int64) + rng.integers(-5, 6, (k, D)), 0, 255)
            H = hs[(na + nb) % 3]
            kp_a, kp_b = _points(rng, na, nb, H)
            for radius in (0.5, 4.0, 1e9):
                want_top = gu.pair_top2(a, b, kp_a, kp_b, H, radius)
                for o in (dict(ratio=0.8), dict(ratio=0.0), dict(ratio=1.0), dict(ratio=0.8, cross_check=False), dict(ratio=0.0, cross_check=False),
                          dict(ratio=0.0, max_dist2=int(np.median(want_top[0][want_top[0] != gu.INT32_MAX])) + 1 if (want_top[0] != gu.INT32_MAX).any() else 1),
                          dict(ratio=0.0, min_matches=max(na, nb))):
                    ta, tb, ia, ib, dd = harness_pair(a, b, kp_a, kp_b, H, radius, **o)
                    assert np.array_equal(ta, np.stack(want_top[:3], 1)) and np.array_equal(tb, np.stack(want_top[3:], 1)), (D, na, nb, radius)
                    wi, wj, wd = gu.accept(want_top, **o)
                    assert np.array_equal(ia, wi) and np.array_equal(ib, wj) and np.array_equal(dd, wd), (D, na, nb, radius, o)
                    if radius == 1e9 and gu.warp(H, kp_a)[2].all():  # open radius: the unguided restatement
                        ui, uj, ud = du.match_pair(a, b, **o)
                        assert np.array_equal(ia, ui) and np.array_equal(ib, uj) and np.array_equal(dd, ud), (D, na, nb, o)
                if radius == 0.5 and nb == 1:
                    assert (ta[:, 2] == gu.INT32_MAX).all()  # fewer than two admissible candidates: no second


def test_open_radius_is_the_unguided_restatement():
    desc_a, ptr_a, desc_b, ptr_b = du.mixed_sets(11, 64, sizes=(17, 65, 130, 0, 1))
    rng = np.random.default_rng(2)
    kp_a = rng.uniform(0, 1920, (ptr_a[-1], 2)).astype(np.float32)
    kp_b = rng.uniform(0, 1920, (ptr_b[-1], 2)).astype(np.float32)
    ia, ib = (x.ravel() for x in np.meshgrid(np.arange(5), np.arange(5)))
    H = np.tile(ROT_ZOOM, (len(ia), 1))
    for o in (dict(ratio=0.8), dict(ratio=0.0, cross_check=False), dict(ratio=1.0, min_matches=5)):
        got = gu.match_pairs_guided(desc_a, ptr_a, kp_a, desc_b, ptr_b, kp_b, ia, ib, H, None, 1e9, **o)
        want = du.match_pairs(desc_a, ptr_a, desc_b, ptr_b, ia, ib, **o)
        for k in ("match_ptr", "idx_a", "idx_b", "dist2"):
            assert np.array_equal(got[k], want[k]), (k, o)
        assert len(got["idx_a"]) > 0


# ------------------------------------------------------------------------------------------------------------ the generator
def test_make_repeated_descriptors(pkg, scene_c1):
    tb = pkg.synth.make_match_table(scene_c1, min_pair_matches=8)
    kw = dict(D=128, noise=12, n_distractors=50, repeat_share=0.7, repeat_group=4, repeat_noise=6)
    ptr, desc, kp = pkg.synth.make_repeated_descriptors(scene_c1, seed=1, **kw)
    p2, d2, k2 = pkg.synth.make_repeated_descriptors(scene_c1, seed=1, **kw)
    assert np.array_equal(ptr, p2) and np.array_equal(desc, d2) and np.array_equal(kp, k2)             # deterministic in its seed
    assert not np.array_equal(desc, pkg.synth.make_repeated_descriptors(scene_c1, seed=2, **kw)[1])
    # the table's feature indices stay valid: the layout of make_descriptors, tracked features first with the table's key points
    p0, d0, k0 = pkg.synth.make_descriptors(scene_c1, D=128, noise=12, n_distractors=50, seed=1)
    assert desc.dtype == np.uint8 and np.array_equal(ptr, p0) and desc.shape == d0.shape and kp.shape == k0.shape
    assert np.array_equal(np.diff(ptr), np.diff(tb.kp_ptr) + 50)
    for i in (0, 7):
        assert np.array_equal(kp[ptr[i]:ptr[i] + tb.kp_ptr[i + 1] - tb.kp_ptr[i]], tb.kp_xy[tb.kp_ptr[i]:tb.kp_ptr[i + 1]])
    s, d, ms = tb.pairs()[0]
    q, t = ms[0]
    assert np.abs(desc[ptr[s] + q].astype(int) - desc[ptr[d] + t].astype(int)).max() <= 24  # two ends of a match: one descriptor
    # texture repeats: tracked features of an image have look-alikes in the SAME image (within the two noises), none without
    n0 = int(tb.kp_ptr[1] - tb.kp_ptr[0])
    x = desc[ptr[0]:ptr[0] + n0].astype(int)
    near = (np.abs(x[:, None, :] - x[None, :, :]).max(-1) <= 2 * (12 + 6)).sum(1) - 1
    assert (near > 0).sum() >= 2 and (near == 0).any()
    y = d0[ptr[0]:ptr[0] + n0].astype(int)
    assert ((np.abs(y[:, None, :] - y[None, :, :]).max(-1) <= 36).sum(1) == 1).all()
    pt, dt, kt = pkg.synth.make_repeated_descriptors(tb, seed=1, **kw)
    assert np.array_equal(pt, ptr) and dt.shape == desc.shape


# ------------------------------------------------------------------------------------------- C-ABI errors that need no device
def test_abi_argument_errors(pkg):
    L = pkg.api.lib()
    EINVAL = -1
    h = C.c_void_p()
    ia = np.zeros(1, dtype=np.int32)
    H = IDENTITY.copy()
    for f in (L.ptz_desc_match_pairs_guided, L.ptz_desc_match_pairs_guided_device):
        assert f(None, None, 1, _p(ia), _p(ia), _p(H), None, C.c_double(4.0), None, C.byref(h)) == EINVAL
        assert f(None, None, 0, None, None, None, None, C.c_double(4.0), None, C.byref(h)) == EINVAL
        assert f(None, None, 0, None, None, None, None, C.c_double(4.0), None, None) == EINVAL
    assert not h.value
    assert "ptz_desc_match_pairs_guided" in pkg.api.EXPORTS and "ptz_desc_match_pairs_guided_device" in pkg.api.EXPORTS


# ------------------------------------------------------------------------------------------------------- the guard on the rig
def test_guard_first_pass_fails_and_two_passes_recover(pkg):
    """Conditions on the INPUT of the chain tests, with the restatement and the project's host homography estimator: repeated
    descriptors must break the first pass (at most 60 % of the table, at least 10 % of its output wrong) and the two-pass flow must
    mend it (at least 90 % of the table, at most 0.5 % wrong)."""
    sc, tb, ptr, desc, kp, _ = gu.repeated_rig(pkg)
    ia, ib = (x.astype(np.int32) for x in np.triu_indices(tb.n_img, 1))
    table = {(s, d): set(ms) for s, d, ms in tb.pairs()}
    first, H, found, second = gu.two_pass(hu.lib(), desc, ptr, kp, desc, ptr, kp, ia, ib, radius_px=4.0, ransac_thresh=4.0, min_inliers=6,
                                          ratio=0.8, cross_check=True, min_matches=8)
    n1, hit1, tot = gu.table_score(first, ia, ib, table)
    n2, hit2, _ = gu.table_score(second, ia, ib, table)
    print(f"table {tot}; first pass {n1} matches, {hit1} in the table ({hit1 / tot:.3f}), {n1 - hit1} not ({(n1 - hit1) / n1:.4f}); "
          f"two passes {n2}, {hit2} in the table ({hit2 / tot:.3f}), {n2 - hit2} not ({(n2 - hit2) / n2:.4f}); {int(found.sum())} models")
    assert hit1 <= 0.60 * tot and n1 - hit1 >= 0.10 * n1
    assert hit2 >= 0.90 * tot and n2 - hit2 <= 0.005 * n2
    assert (second["match_ptr"][1:] - second["match_ptr"][:-1])[found == 0].sum() == 0  # a pair without a model keeps none
