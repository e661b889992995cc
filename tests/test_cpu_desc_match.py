"""CPU tests of the descriptor matcher's contract and of its host plumbing: the shared header (ptz-calib_amd/csrc/ptz_desc_match.h)
instantiated on the host by tests/cpu_harness/desc_match_harness.cc against the numpy restatement (desc_match_util.py), the loader
of descriptors, the writer of match files, the generator of descriptors and the argument errors of the C-ABI that need no device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import desc_match_util as du
import host_util as hu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_h = None


def harness():
    global _h
    if _h is None:
        _h = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "libdesc_match_harness.so"))
        _h.h_desc_match_pair.restype = C.c_int64
    return _h


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness_pair(a, b, ratio=0.8, max_dist2=0, cross_check=True, min_matches=0, seed=1, parts=5):
    a = np.ascontiguousarray(a, dtype=np.uint8); b = np.ascontiguousarray(b, dtype=np.uint8)
    na, nb, D = len(a), len(b), a.shape[1]
    ta = np.zeros((max(na, 1), 3), dtype=np.int32); tb = np.zeros((max(nb, 1), 3), dtype=np.int32)
    ia, ib, dd = (np.zeros(max(na, 1), dtype=np.int32) for _ in range(3))
    n = harness().h_desc_match_pair(_p(a), na, _p(b), nb, D, C.c_double(ratio), int(max_dist2), int(cross_check), int(min_matches),
                                    C.c_uint64(seed), int(parts), _p(ta), _p(tb), _p(ia), _p(ib), _p(dd))
    return ta[:na], tb[:nb], ia[:n], ib[:n], dd[:n]


def _probe(cmd, a="", b=""):
    lib = hu.lib()
    lib.ptzh_io_probe.restype = C.c_void_p
    p = lib.ptzh_io_probe(cmd.encode(), a.encode(), b.encode())
    txt = C.string_at(p).decode()
    lib.ptzh_free(C.c_void_p(p))
    return json.loads(txt)


# ----------------------------------------------------------------------------------------------------------------- the header
@pytest.mark.parametrize("D", du.DIMS)
def test_header_on_host_equals_numpy(D):
    """top-2 by merging in a scrambled order, then the rule, on every size of the list (ties at D = 1, where values repeat; a
    one-feature image has its second at INT32_MAX)"""
    rng = np.random.default_rng(D)
    sizes = du.SIZES
    for na in sizes:
        for nb in sizes:
            a = rng.integers(0, 4 if D == 1 else 256, (na, D), dtype=np.uint8)
            b = rng.integers(0, 4 if D == 1 else 256, (nb, D), dtype=np.uint8)
            k = min(na, nb) // 2
            if k and D > 1:
                b[rng.permutation(nb)[:k]] = np.clip(a[rng.permutation(na)[:k]].astype(np.int64) + rng.integers(-5, 6, (k, D)), 0, 255)
            want_top = du.pair_top2(a, b)
            for o in (dict(ratio=0.8), dict(ratio=0.0), dict(ratio=1.0), dict(ratio=0.8, cross_check=False), dict(ratio=0.0, cross_check=False),
                      dict(ratio=0.0, max_dist2=int(np.median(want_top[0])) + 1), dict(ratio=0.0, min_matches=max(na, nb))):
                ta, tb, ia, ib, dd = harness_pair(a, b, seed=na * 1000 + nb, parts=1 + (na + nb) % 6, **o)
                assert np.array_equal(ta, np.stack(want_top[:3], 1)) and np.array_equal(tb, np.stack(want_top[3:], 1)), (D, na, nb)
                wi, wj, wd = du.accept(want_top, **o)
                assert np.array_equal(ia, wi) and np.array_equal(ib, wj) and np.array_equal(dd, wd), (D, na, nb, o)
            if nb == 1:
                assert (ta[:, 2] == du.INT32_MAX).all()


def test_header_ties_and_extremes():
    rng = np.random.default_rng(3)
    a = du.random_desc(rng, 40, 128)
    b = du.random_desc(rng, 257, 128)
    b[3] = a[7]; b[200] = a[7]; a[21] = a[20]; b[100] = a[20]
    for seed in range(5):
        ta, tb, ia, ib, dd = harness_pair(a, b, ratio=0.0, seed=seed, parts=7)
        assert ta[7].tolist() == [0, 3, 0] and tb[100].tolist()[:2] == [0, 20] and tb[100, 2] == 0
        m = dict(zip(ia.tolist(), ib.tolist()))
        assert m[7] == 3 and m[20] == 100 and 21 not in m
        _, _, ia, ib, _ = harness_pair(a, b, ratio=0.8, seed=seed, parts=3)
        assert 7 not in ia and 20 not in ia and 21 not in ia
    # the largest distance there is
    x = np.full((3, 512), 255, np.uint8); y = np.zeros((2, 512), np.uint8)
    ta, tb, ia, ib, dd = harness_pair(x, y, ratio=0.0, cross_check=False)
    assert (ta[:, 0] == 512 * 255 * 255).all() and (ta[:, 1] == 0).all() and dd.tolist() == [512 * 255 * 255] * 3 and ib.tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------------ host plumbing
def test_descriptor_loader_and_quantiser(pkg, tmp_path):
    rng = np.random.default_rng(0)
    kp = rng.uniform(0, 1000, (7, 2)).astype(np.float32)
    desc = du.random_desc(rng, 7, 33)
    pkg.dataset_io.write_features(str(tmp_path), ["a.png"], [0, 7], kp, desc=desc)
    r = _probe("descriptors", str(tmp_path / "a.png.txt"))
    assert r["ok"] and r["dim"] == 33 and np.array_equal(np.array(r["desc"], dtype=np.uint8).reshape(7, 33), desc)
    assert _probe("descriptors", str(tmp_path / "a.png.txt"), "33")["ok"]
    assert not _probe("descriptors", str(tmp_path / "a.png.txt"), "32")["ok"]       # another dimension than the images before it
    assert not _probe("descriptors", str(tmp_path / "missing.txt"))["ok"]
    # the default writer (zeros) still reads as before, and as integer descriptors
    pkg.dataset_io.write_features(str(tmp_path), ["z.png"], [0, 7], kp, desc_dim=4)
    r = _probe("descriptors", str(tmp_path / "z.png.txt"))
    assert r["ok"] and r["dim"] == 4 and not any(r["desc"])
    # a float file goes through the quantiser
    v = rng.normal(size=(5, 8)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    with open(tmp_path / "f.png.txt", "w") as f:
        f.write("5 8\n")
        for row in v:
            f.write("1 2 1 0 " + " ".join(repr(float(x)) for x in row) + "\n")
    r = _probe("descriptors", str(tmp_path / "f.png.txt"))
    assert r["ok"] and np.array_equal(np.array(r["desc"]).reshape(5, 8), np.clip(np.rint(128 + 127 * v), 0, 255).astype(np.int64))
    # an image without features fits any dimension and leaves it as it is
    with open(tmp_path / "e.png.txt", "w") as f:
        f.write("0 0\n")
    r = _probe("descriptors", str(tmp_path / "e.png.txt"), "33")
    assert r["ok"] and r["dim"] == 33 and r["desc"] == []
    # a short file is a load error
    with open(tmp_path / "s.png.txt", "w") as f:
        f.write("3 4\n1 2 1 0 1 2 3 4\n1 2 1 0 1 2\n")
    assert not _probe("descriptors", str(tmp_path / "s.png.txt"))["ok"]


def test_matches_writer_round_trip(pkg, tmp_path):
    pairs = [("a.png", "b.png", [(0, 5), (3, 1), (7, 7)]), ("b.png", "c.jpg", [(2, 2)]), ("c.jpg", "a.png", [(9, 0), (10, 4)])]
    src = str(tmp_path / "in.txt"); dst = str(tmp_path / "out.txt"); again = str(tmp_path / "again.txt")
    pkg.dataset_io.write_matches(src, pairs)
    r = _probe("rewrite_matches", src, dst)
    assert r["ok"] and r["blocks"] == 3
    assert open(dst).read() == open(src).read() and open(dst).read().endswith("\n\n")
    assert _probe("rewrite_matches", dst, again)["blocks"] == 3 and open(again).read() == open(src).read()


def test_make_descriptors(pkg, scene_c1):
    tb = pkg.synth.make_match_table(scene_c1, min_pair_matches=8)
    ptr, desc, kp = pkg.synth.make_descriptors(scene_c1, D=128, noise=12, n_distractors=50, seed=1)
    assert desc.dtype == np.uint8 and desc.shape == (ptr[-1], 128) and kp.shape == (ptr[-1], 2)
    assert np.array_equal(np.diff(ptr), np.diff(tb.kp_ptr) + 50)
    for i in (0, 7):  # the tracked features come first, with the table's key points
        assert np.array_equal(kp[ptr[i]:ptr[i] + tb.kp_ptr[i + 1] - tb.kp_ptr[i]], tb.kp_xy[tb.kp_ptr[i]:tb.kp_ptr[i + 1]])
    # the two ends of a match are noisy copies of one descriptor
    s, d, ms = tb.pairs()[0]
    q, t = ms[0]
    assert np.abs(desc[ptr[s] + q].astype(int) - desc[ptr[d] + t].astype(int)).max() <= 24
    p2, d2, k2 = pkg.synth.make_descriptors(tb, D=128, noise=12, n_distractors=50, seed=1)
    assert np.array_equal(p2, ptr) and d2.shape == desc.shape


# ------------------------------------------------------------------------------------------- C-ABI errors that need no device
def test_abi_argument_errors(pkg):
    L = pkg.api.lib()
    EINVAL, ELIMIT = -1, -5
    h = C.c_void_p()
    ptr = np.array([0, 4], dtype=np.int64)
    desc = np.zeros((4, 8), dtype=np.uint8)
    args = lambda n_img, p, d, D, dev=0: (n_img, _p(p) if p is not None else None, _p(d) if d is not None else None, D, None, dev, C.byref(h))
    assert L.ptz_desc_set_create(*args(-1, ptr, desc, 8)) == EINVAL
    assert L.ptz_desc_set_create(*args(1, None, desc, 8)) == EINVAL
    assert L.ptz_desc_set_create(*args(1, ptr, desc, 0)) == EINVAL
    assert L.ptz_desc_set_create(*args(1, ptr, desc, 513)) == EINVAL
    assert L.ptz_desc_set_create(*args(1, ptr, None, 8)) == EINVAL
    assert L.ptz_desc_set_create(*args(1, ptr, desc, 8, -1)) == EINVAL
    assert L.ptz_desc_set_create(*args(2, np.array([0, 4, 3], dtype=np.int64), desc, 8)) == EINVAL   # decreasing
    assert L.ptz_desc_set_create(*args(1, np.array([1, 4], dtype=np.int64), desc, 8)) == EINVAL
    assert L.ptz_desc_set_create(*args(1, np.array([0, 2**31], dtype=np.int64), desc, 8)) == ELIMIT
    assert L.ptz_desc_set_create(1, _p(ptr), _p(desc), 8, None, 0, None) == EINVAL
    assert not h.value
    ia = np.zeros(1, dtype=np.int32)
    assert L.ptz_desc_match_pairs(None, None, 1, _p(ia), _p(ia), None, C.byref(h)) == EINVAL
    assert L.ptz_desc_match_pairs(None, None, 0, None, None, None, None) == EINVAL
    assert L.ptz_debug_desc_dist2(None, 0, None, 0, None) == EINVAL
    assert L.ptz_desc_matches_download(None, None, None, None, None, None, None) == EINVAL
    L.ptz_desc_matches_n_matches.restype = C.c_int64
    assert L.ptz_desc_matches_n_matches(None) == 0
    o = pkg.api.desc_options()
    assert (o.ratio, o.max_dist2, o.cross_check, o.min_matches, o.device_id, o.workspace_bytes) == (0.8, 0, 1, 0, 0, 256 << 20)
