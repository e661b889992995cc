"""GPU tests of the rotation-and-focal gate (ptz_rotfocal_gate): every output of ptz_rotfocal_gate_run and _run_device is ARRAY-EQUAL to
the host instantiation of ptz_rotfocal.h (tests/cpu_harness/rotfocal_harness.cc, held to the numpy restatement by test_cpu_rotfocal.py)
and to the integer compaction numpy builds from its mask.  No tolerance anywhere."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import rotfocal_util as ru

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 3, 63, 64, 65, 257, 2048, 2049, 5000)  # below, at and above the wave and the 1024-match tile; one beyond the homography gate's 4096
ANCHORS = {"virtual": ru.VIRTUAL, "real": ru.REAL}
FILL = 0xAB


@functools.lru_cache(maxsize=None)
def batch(anchor):
    return ru.make_batch(SIZES, seed=3, cam_a=ANCHORS[anchor])


@functools.lru_cache(maxsize=None)
def reference(anchor, iters):
    ptr, a, b, cr, cc, _ = batch(anchor)
    return ru.harness_batch(ptr, a, b, cr, cc, 4.0, iters, fill=FILL)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def equal_to_reference(g, want, ptr, a, b, min_inliers):
    assert np.array_equal(g["found"], want["found"])
    assert same_bits(g["model"], want["model"]) and same_bits(g["H"].reshape(-1, 9), want["H"]) and np.array_equal(g["mask"], want["mask"])
    out_ptr, oa, ob, oi = ru.compact(ptr, want["found"], want["mask"], a, b, min_inliers)
    assert np.array_equal(g["out_ptr"], out_ptr) and np.array_equal(g["out_index"], oi)
    assert same_bits(g["out_uv_a"], oa) and same_bits(g["out_uv_b"], ob)
    return out_ptr


@pytest.mark.parametrize("min_inliers", [0, 6, 600])
@pytest.mark.parametrize("iters", [1, 128, 300])
@pytest.mark.parametrize("anchor", sorted(ANCHORS))
def test_run_equals_the_host_harness(pkg, anchor, iters, min_inliers):
    """the mixed batch; iters = 300 makes a thread take three rounds of hypotheses.  model, H and mask of a query without a model keep
    the pattern they were filled with."""
    ptr, a, b, cr, cc, _ = batch(anchor)
    want = reference(anchor, iters)
    with pkg.api.RotFocalGate(len(SIZES), len(a)) as gate:
        g = gate.run(ptr, a, b, cr, cc, thresh=4.0, min_inliers=min_inliers, iters=iters, fill=FILL)
    out_ptr = equal_to_reference(g, want, ptr, a, b, min_inliers)
    assert g["device_ms"] > 0
    assert (want["found"][:3] == 0).all() and (g["model"][:3] == float(FILL)).all() and (g["mask"][:ptr[3]] == FILL).all()
    if iters >= 128:
        assert (want["found"][4:] == 1).all()
        kept = np.diff(out_ptr)
        if min_inliers == 600:
            assert (kept[:8] == 0).all() and (kept[8:] >= 600).all()
        else:
            assert (kept[4:] > 0).all()


def test_the_5000_match_query_is_served(pkg):
    """the homography gate answers found = -1 for a query beyond its table; the new gate has no such limit"""
    ptr, a, b, cr, cc, wrong = batch("virtual")
    old = pkg.api.gate_matches(ptr, a, b, max_pair_matches=4096)
    assert old["found"][-1] == -1 and old["out_ptr"][-1] == old["out_ptr"][-2]
    with pkg.api.RotFocalGate(len(SIZES), len(a)) as gate:
        g = gate.run(ptr, a, b, cr, cc)
    s = slice(int(ptr[-2]), int(ptr[-1]))
    assert g["found"][-1] == 1 and int(np.diff(g["out_ptr"])[-1]) == int(g["mask"][s].sum())
    good = ~wrong[s]
    assert int(g["mask"][s][good].sum()) >= 0.98 * int(good.sum()) and int(g["mask"][s][wrong[s]].sum()) <= 50


@pytest.mark.parametrize("iters", [128, 300])
def test_a_query_alone_reversed_and_split_gives_the_same_bits(pkg, iters):
    ptr, a, b, cr, cc, _ = batch("virtual")
    want = reference("virtual", iters)
    nq = len(SIZES)

    def sub(order):
        sizes = [SIZES[q] for q in order]
        p2 = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        idx = np.concatenate([np.arange(ptr[q], ptr[q + 1]) for q in order]).astype(np.int64) if order else np.zeros(0, np.int64)
        with pkg.api.RotFocalGate(max(len(order), 1), len(idx)) as gate:
            g = gate.run(p2, a[idx], b[idx], cr[list(order)], cc[list(order)], iters=iters, fill=FILL)
        for k, q in enumerate(order):
            assert g["found"][k] == want["found"][q]
            assert same_bits(g["model"][k], want["model"][q]) and same_bits(g["H"][k].reshape(9), want["H"][q])
            assert np.array_equal(g["mask"][p2[k]:p2[k + 1]], want["mask"][ptr[q]:ptr[q + 1]])

    sub(list(range(nq))[::-1])
    sub(list(range(0, 5)))
    sub(list(range(5, nq)))
    for q in (3, 7, 10):
        sub([q])


def test_errors_return_before_device_work(pkg):
    import ctypes as C
    api = pkg.api
    ptr, a, b, cr, cc, _ = ru.make_batch((8, 8), seed=1)
    L = api.lib()
    h = C.c_void_p()
    assert L.ptz_rotfocal_gate_create(0, C.c_int64(16), 0, C.byref(h)) == -1
    assert L.ptz_rotfocal_gate_create(2, C.c_int64(-1), 0, C.byref(h)) == -1
    assert L.ptz_rotfocal_gate_create(2, C.c_int64(16), -1, C.byref(h)) == -1
    assert L.ptz_rotfocal_gate_create(2, C.c_int64(16), 0, None) == -1
    assert L.ptz_rotfocal_gate_create(2, C.c_int64(2 ** 31), 0, C.byref(h)) == -5
    with api.RotFocalGate(2, 16) as gate:
        for kw in (dict(thresh=0.0), dict(thresh=-1.0), dict(thresh=float("nan")), dict(thresh=float("inf")), dict(min_inliers=-1),
                   dict(iters=0), dict(iters=4097), dict(iters=-5)):
            with pytest.raises(api.PtzError, match="PTZ_EINVAL"):
                gate.run(ptr, a, b, cr, cc, **kw)
        bad = ptr.copy(); bad[0] = 1
        with pytest.raises(api.PtzError, match="PTZ_EINVAL"):
            gate.run(bad, a, b, cr, cc)
        bad = ptr.copy(); bad[1] = 20
        with pytest.raises(api.PtzError, match="PTZ_EINVAL"):
            gate.run(bad, a, b, cr, cc)
        p3, a3, b3, cr3, cc3, _ = ru.make_batch((4, 4, 4), seed=1)
        with pytest.raises(api.PtzError, match="PTZ_ELIMIT"):
            gate.run(p3, a3, b3, cr3, cc3)
        p4, a4, b4, cr4, cc4, _ = ru.make_batch((9, 9), seed=1)
        with pytest.raises(api.PtzError, match="PTZ_ELIMIT"):
            gate.run(p4, a4, b4, cr4, cc4)
        # the device entry: NULL required arrays, a negative count, too many queries -- all answered before anything is enqueued
        one = C.c_void_p(256)  # never dereferenced: every call below returns at its checks
        def dev(n_pair=2, ptr_=one, found=one, out_ptr=one, cref=one, thresh=4.0, min_inl=0, iters=128, uv=one, g=gate.handle):
            return L.ptz_rotfocal_gate_run_device(g, n_pair, ptr_, uv, uv, cref, one, C.c_double(thresh), min_inl, iters, None, None, found, None, out_ptr,
                                                  one, one, None, None)
        assert dev(g=None) == -1 and dev(n_pair=-1) == -1 and dev(ptr_=None) == -1 and dev(found=None) == -1 and dev(out_ptr=None) == -1
        assert dev(cref=None) == -1 and dev(uv=None) == -1 and dev(thresh=0.0) == -1 and dev(min_inl=-1) == -1 and dev(iters=0) == -1
        assert dev(iters=4097) == -1 and dev(n_pair=3) == -5
        g0 = gate.run(np.zeros(1, np.int64), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros((0, 15)), np.zeros((0, 15)))
        assert g0["out_ptr"].tolist() == [0] and len(g0["found"]) == 0


def test_device_entry_equals_the_host_harness_and_writes_only_its_ranges():
    """RotFocalGate.run_device on torch tensors pre-filled with a pattern, own process with torch initialised first (see
    test_device_resident_chain_gate_then_solve)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "run_rotfocal_gate_device.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.count("rotfocal device entry ok") == 3, r.stdout[-2000:] + r.stderr[-2000:]
