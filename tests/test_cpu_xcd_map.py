"""CPU tests of the index arithmetic that deals the workgroups of an (item, slot) launch over the 8 XCDs by the live slot count
(ptz-calib_amd/csrc/ptz_xcd_map.h, what xcd_remap calls in k_schur, k_schur_w, k_schur_f and the tile kernels of the batch
Cholesky), through tests/cpu_harness/xcd_map_harness.cc.

A launch of gx x rows workgroups of which only rows 0 .. live-1 have work: the workgroup with linear id L belongs to XCD L % 8 and
is that XCD's (L // 8)-th; the XCD owns one contiguous range of the gx x live items, the eight ranges follow one another in XCD
order and differ in length by at most one, and the ids beyond a range's length have nothing to do.  With live == rows the mapping
is the one the kernels had before there was a live count, restated in the harness."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_harness", "xcd_map_harness.cc")
HDR = os.path.join(ROOT, "ptz-calib_amd", "csrc", "ptz_xcd_map.h")

GX = [1, 3, 13, 200]
ROWS = [1, 2, 7, 8, 9, 48, 512]


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(ROOT, "tests", "cpu_harness", "libxcd_map_harness.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, SRC])
    return C.CDLL(so)


def _live_map(h, gx, rows, live):
    out = np.zeros((gx * rows, 3), np.int32)
    h.h_xcd_live_map(gx, rows, live, out.ctypes.data_as(C.c_void_p))
    return out[:, 0] != 0, out[:, 1].astype(np.int64), out[:, 2].astype(np.int64)


def _full_map(h, gx, rows):
    out = np.zeros((gx * rows, 2), np.int32)
    h.h_xcd_full_map(gx, rows, out.ctypes.data_as(C.c_void_p))
    return out[:, 0].astype(np.int64), out[:, 1].astype(np.int64)


@pytest.mark.parametrize("gx", GX)
@pytest.mark.parametrize("rows", ROWS)
def test_accepted_ids_cover_the_live_items_once_in_balanced_ranges(harness, gx, rows):
    L = np.arange(gx * rows)
    for live in range(rows + 1):
        work, bx, by = _live_map(harness, gx, rows, live)
        items = gx * live
        assert (bx[work] < gx).all() and (by[work] < live).all(), live
        item = by * gx + bx
        # one-to-one onto [0, gx * live)
        assert np.array_equal(np.sort(item[work]), np.arange(items)), live
        lens, nxt = [], 0
        for x in range(8):
            sel = work & (L % 8 == x)
            got = item[sel]  # in ascending id
            lens.append(len(got))
            # one contiguous range per residue, walked in id order, the ranges in XCD order; the accepted ids are the XCD's first
            assert np.array_equal(got, np.arange(nxt, nxt + len(got))), (live, x)
            assert np.array_equal(L[sel] // 8, np.arange(len(got))), (live, x)
            nxt += len(got)
        assert nxt == items and max(lens) - min(lens) <= 1, (live, lens)


@pytest.mark.parametrize("gx", GX)
@pytest.mark.parametrize("rows", ROWS)
def test_a_launch_without_idle_rows_keeps_the_former_mapping(harness, gx, rows):
    work, bx, by = _live_map(harness, gx, rows, rows)
    fx, fy = _full_map(harness, gx, rows)
    assert work.all() and np.array_equal(bx, fx) and np.array_equal(by, fy)


@pytest.mark.parametrize("gx", GX)
@pytest.mark.parametrize("rows", ROWS)
def test_no_live_row_accepts_nothing(harness, gx, rows):
    work, _, _ = _live_map(harness, gx, rows, 0)
    assert not work.any()


def test_stand_alone_harness_passes():
    """The same sweep as a program of its own (the form a sanitizer build uses)."""
    exe = os.path.join(ROOT, "tests", "cpu_harness", "xcd_map_harness_main")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-DXCD_MAP_MAIN", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "xcd_map_harness: ok" in r.stdout, r.stdout[-2000:]
