"""CPU tests of the batched RANSAC homography estimator (ptz-calib_amd/csrc/ptz_homography.h, ptz_homography_ransac_batch):
the header's math instantiated on the host equals the host estimator (host/homography.cc) bit for bit, the adaptive bound
table the kernel reads is the host's formula, and the C-ABI validates before it looks for a device and has no CPU fallback."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import homography_corpus as hc
import host_util as hu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEVICE = -1, -2


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(ROOT, "tests", "cpu_harness", "libhomography_harness.so")
    src = os.path.join(ROOT, "tests", "cpu_harness", "homography_harness.cc")
    srcs = [src, os.path.join(ROOT, "ptz-calib_amd", "csrc", "ptz_homography.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    return C.CDLL(so)


def test_host_instantiation_matches_host_estimator(harness):
    """2 000+ pairs (0-3 000 matches, 0-80 % outliers, degenerate / duplicated points, NaN pixels, the INT_MIN bound): found
    flag, the nine doubles of H and the inlier mask of the header's sequential composition equal ptzh_find_homography's."""
    ptr, src, dst = hc.corpus(seed=0, n_pairs=2000)
    n = np.diff(ptr)
    assert len(n) >= 2000 and n.min() == 0 and n.max() >= 2900 and (n == 4).sum() >= 3 and (n == 5).sum() >= 3
    Hh, fh, mh = hc.run_per_pair(hu.lib().ptzh_find_homography, ptr, src, dst)
    Hd, fd, md = hc.run_per_pair(harness.h_find_homography, ptr, src, dst)
    assert np.array_equal(fh, fd)
    assert np.array_equal(Hh.view(np.uint64), Hd.view(np.uint64))
    assert np.array_equal(mh, md)
    assert 0 < (fh == 0).sum() < 20 and (fh == 1).sum() > 1900  # both outcomes exercised


def test_bound_table_is_the_host_formula(pkg, harness):
    """ptz_debug_homography_bounds (the table the kernel reads) for every n <= 4096 and every count equals the host
    formula, INT_MIN where ceil(need) overflows int (4 inliers of 1000 matches)."""
    lib = pkg.api.lib()
    a = np.zeros(4097, dtype=np.int32); b = np.zeros(4097, dtype=np.int32)
    for n in range(0, 4097):
        assert lib.ptz_debug_homography_bounds(n, hc._p(a)) == 0
        harness.h_adaptive_bounds(n, hc._p(b))
        assert np.array_equal(a[:n + 1], b[:n + 1]), n
    lib.ptz_debug_homography_bounds(1000, hc._p(a))
    assert a[4] == -2**31 and 0 < a[1000 // 2] < 2000 and a[1000] == 0
    assert lib.ptz_debug_homography_bounds(-1, hc._p(a)) == EINVAL and lib.ptz_debug_homography_bounds(4, None) == EINVAL


def _call(lib, n_pair, ptr, src, dst, thresh=4.0, H=None, found=None, mask=None, device_id=0):
    ms = C.c_double()
    return lib.ptz_homography_ransac_batch(n_pair, hc._p(ptr), hc._p(src), hc._p(dst), C.c_double(thresh), device_id, hc._p(H),
                                           hc._p(found), hc._p(mask), C.byref(ms))


def test_validation_precedes_device_and_no_cpu_fallback(pkg):
    lib = pkg.api.lib()
    ptr, src, dst = hc.corpus(seed=1, n_pairs=40)
    n = len(ptr) - 1
    H = np.zeros(9 * n); found = np.zeros(n, np.int32); mask = np.zeros(int(ptr[-1]), np.uint8)
    # malformed calls are PTZ_EINVAL whether or not a GPU exists
    assert _call(lib, -1, ptr, src, dst, H=H, found=found) == EINVAL
    bad = ptr.copy(); bad[0] = 1
    assert _call(lib, n, bad, src, dst, H=H, found=found) == EINVAL
    bad = ptr.copy(); bad[5] = bad[4] - 1
    assert _call(lib, n, bad, src, dst, H=H, found=found) == EINVAL
    for t in (0.0, -4.0, float("nan"), float("inf")):
        assert _call(lib, n, ptr, src, dst, thresh=t, H=H, found=found) == EINVAL
    assert _call(lib, n, None, src, dst, H=H, found=found) == EINVAL
    assert _call(lib, n, ptr, None, dst, H=H, found=found) == EINVAL
    assert _call(lib, n, ptr, src, None, H=H, found=found) == EINVAL
    assert _call(lib, n, ptr, src, dst, H=None, found=found) == EINVAL
    assert _call(lib, n, ptr, src, dst, H=H, found=None) == EINVAL
    with pytest.raises(pkg.api.PtzError) as e:
        pkg.api.find_homographies(bad, src, dst)
    assert e.value.code == EINVAL
    # empty extents: no pair, or pairs without matches, need no point arrays
    assert _call(lib, 0, np.zeros(1, np.int64), None, None) == 0
    assert _call(lib, 0, None, None, None) == 0
    if pkg.api.device_count() == 0:
        # no GPU: the call fails loudly, never computes on the CPU
        found[:] = 7
        assert _call(lib, n, ptr, src, dst, H=H, found=found, mask=mask) == ENODEVICE
        assert (found == 7).all() and (H == 0).all()
        with pytest.raises(pkg.api.PtzError) as e:
            pkg.api.find_homographies(ptr, src, dst)
        assert e.value.code == ENODEVICE
        assert _call(lib, 2, np.zeros(3, np.int64), None, None, H=np.zeros(18), found=np.zeros(2, np.int32)) == ENODEVICE
