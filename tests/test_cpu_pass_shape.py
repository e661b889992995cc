"""CPU tests of the grid extent of an LM pass (ptz-calib_amd/csrc/ptz_pass_shape.h, the function solve_impl calls for every pass
it enqueues), through tests/cpu_harness/pass_shape_harness.cc.

The ladder of a batch of n scenes is restated here as the library builds it: full size, then compacted shapes of 2 slots (8 for a
batch of up to eight) times four while below n.  The covering shape -- the one whose kernel variants and factorisation path a pass
gets -- is the smallest compacted shape that holds the reported count and is smaller than the group, else the full-size shape."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_harness", "pass_shape_harness.cc")
HDR = os.path.join(ROOT, "ptz-calib_amd", "csrc", "ptz_pass_shape.h")

# (batch, group): group sizes 1, 8, 33, 500 and 1000.  A group of 8 that keeps a compacted list is half of a batch of 16; the
# batch of 8 itself (one shape, no list on the device) is CASES_NO_LIST below
CASES = [(1, 1), (16, 8), (33, 33), (1000, 500), (1000, 1000)]
COUNTS = range(1, 1101)


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(ROOT, "tests", "cpu_harness", "libpass_shape_harness.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, SRC])
    return C.CDLL(so)


def _ladder(n):
    lad, sl = [n], (2 if n > 8 else 8)
    while sl < n:
        lad.append(sl)
        sl *= 4
    return lad


def _covering(count, group_n, lad):
    for k in range(1, len(lad)):
        if lad[k] >= count and lad[k] < group_n:
            return k
    return 0


def _extent(h, count, group_n, lad, graph, exact_fit):
    a = np.asarray(lad, dtype=np.int32)
    out = np.zeros(3, np.int32)
    h.h_pass_extent(count, group_n, a.ctypes.data_as(C.c_void_p), len(lad), int(graph), int(exact_fit), out.ctypes.data_as(C.c_void_p))
    return int(out[0]), int(out[1]), bool(out[2])


@pytest.mark.parametrize("batch,group", CASES)
def test_replayed_passes_keep_the_ladder_shape(harness, batch, group):
    """A pass replayed from a captured graph has the frozen grid of its ladder shape, exact fit or not -- and so has every pass
    when exact fit is switched off."""
    lad = _ladder(batch)
    for count in COUNTS:
        k = _covering(count, group, lad)
        want = (k, lad[k] if k else group, k != 0)
        assert _extent(harness, count, group, lad, True, True) == want, count
        assert _extent(harness, count, group, lad, True, False) == want, count
        assert _extent(harness, count, group, lad, False, False) == want, count


@pytest.mark.parametrize("batch,group", CASES)
def test_eager_passes_fit_the_count(harness, batch, group):
    """Enqueued launch by launch: the count clamped to [1, group size], compacted iff that is below the group size, variants
    (the shape index) those of the covering ladder shape."""
    lad = _ladder(batch)
    for count in COUNTS:
        shape, slots, compact = _extent(harness, count, group, lad, False, True)
        assert slots == min(max(count, 1), group), count
        assert compact == (slots < group), count
        assert shape == _covering(count, group, lad), count
    for count in (0, -3):  # the last scene retired between the host's look and the enqueue: one (empty) slot, never a zero grid
        shape, slots, compact = _extent(harness, count, group, lad, False, True)
        assert slots == 1 and compact == (group > 1) and shape == _covering(count, group, lad)


@pytest.mark.parametrize("n", [1, 5, 8])
def test_batches_without_a_compacted_list_stay_full_size(harness, n):
    """A batch of up to eight scenes keeps one shape and runs no k_compact, so there is no list a compacted grid could index: its
    passes stay full size whatever the count (the same holds with PTZ_BA_COMPACT=0, which hands the function a ladder of one)."""
    assert _ladder(n) == [n]
    for count in range(0, n + 3):
        for graph in (False, True):
            assert _extent(harness, count, n, [n], graph, True) == (0, n, False)


def test_stand_alone_harness_passes():
    """The same sweep as a program of its own (the form a sanitizer build uses)."""
    exe = os.path.join(ROOT, "tests", "cpu_harness", "pass_shape_harness_main")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-DPASS_SHAPE_MAIN", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "pass_shape_harness: ok" in r.stdout, r.stdout[-2000:]
