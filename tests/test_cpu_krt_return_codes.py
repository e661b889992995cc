"""What the eight relocalization entry points (plain solve, covariance, residual report, trimmed solve; host form and _device form)
answer to malformed calls, pinned: the four host forms do not validate alike (the table beside check_host_batch in
ptz-calib_amd/csrc/ptz_krt_device.h), and a change of their shared plumbing must not change one answer.

The expected codes are not derived: tests/golden/krt_return_codes.json holds what the library returned for record(lib) below BEFORE the
entry points were moved onto the shared path, on a machine without a GPU.  There every call returns before it touches a device; a call
whose arguments pass every check gets as far as hipGetDeviceCount and is answered PTZ_ENODEVICE -- those rows are marked
"reaches_device" in the fixture: what they return depends on the machine (with a GPU they would go on to run on the arrays of this
file, host memory also for the _device forms), so they are compared only where there is no device.  The same fixture pins
ptz_krt_trim_workspace_bytes, by which a caller of ptz_krt_solve_batch_trimmed_device sizes a buffer."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import krt_trim_util as tu

_p = tu._p
GOLDEN = os.path.join(tu.ROOT, "tests", "golden", "krt_return_codes.json")
ENODEVICE = -2
WORKSPACE_SHAPES = [(1, 0), (1, 1), (3, 384), (24, 3072), (257, 1), (100000, 12800000)]
N, NM = 3, 12


def _workspace_bytes(lib, n_query, n_match):
    f = lib.ptz_krt_trim_workspace_bytes
    f.restype, f.argtypes = C.c_int64, [C.c_int32, C.c_int64]
    return int(f(n_query, n_match))


def _aligned_bytes(nbytes):
    raw = np.full(nbytes + 256, 0xA5, dtype=np.uint8)
    at = (-raw.ctypes.data) % 256
    return raw[at:at + nbytes]


def _args(lib):
    """a well-formed batch of 3 queries of 4 matches, no 2D-3D points, and every output poisoned; by argument name"""
    rng = np.random.default_rng(0)
    f8 = lambda *shape: np.full(shape, -7.0)
    return dict(n=N, ptr=np.arange(0, NM + 1, 4, dtype=np.int64), uvr=rng.uniform(0, 1000, (NM, 2)).astype(np.float32),
                uvc=rng.uniform(0, 1000, (NM, 2)).astype(np.float32), pptr=None, p2=None, p3=None, cref=np.ones((N, 15)), ccur=f8(N, 15), ft=0,
                summ=np.full(N * 256, 0xA5, np.uint8), acc=np.full(N, -7, np.int32), ms=f8(1), cov=f8(N, 36), s0=f8(N), st=np.full(N, -7, np.int32),
                err=f8(NM), rms=f8(N), mx=f8(N), med=f8(N), cnt=np.full(N, -7, np.int32), rms3=f8(N), kept=np.full(NM, 0xA5, np.uint8),
                rep=np.full(N * 256, 0xA5, np.uint8), work=_aligned_bytes(_workspace_bytes(lib, N, NM)))


OUTPUTS = ("ccur", "summ", "acc", "ms", "cov", "s0", "st", "err", "rms", "mx", "med", "cnt", "rms3", "kept", "rep", "work")
D0, D100 = C.c_double(0.0), C.c_double(100.0)


def _batch(a):
    return [_p(a[k]) for k in ("ptr", "uvr", "uvc", "pptr", "p2", "p3", "cref", "ccur")]


# entry point -> (the call on the arguments of _args(), its required pointers)
ENTRIES = {
    "ptz_krt_solve_batch_2d3d": (lambda lib, a: lib.ptz_krt_solve_batch_2d3d(a["n"], *_batch(a), a["ft"], D100, None, _p(a["summ"]), _p(a["acc"]), _p(a["ms"])),
                                 ("ptr", "uvr", "uvc", "cref", "ccur", "summ", "acc")),
    "ptz_krt_solve_batch_device": (lambda lib, a: lib.ptz_krt_solve_batch_device(a["n"], *_batch(a), a["ft"], D100, None, _p(a["summ"]), _p(a["acc"]), None),
                                   ("ptr", "uvr", "uvc", "cref", "ccur", "summ", "acc")),
    "ptz_krt_covariance_batch": (lambda lib, a: lib.ptz_krt_covariance_batch(a["n"], *_batch(a), a["ft"], None, None, D0, 0, _p(a["cov"]), _p(a["s0"]),
                                                                             _p(a["st"]), _p(a["ms"])),
                                 ("ptr", "uvr", "uvc", "cref", "ccur", "cov", "s0", "st")),
    "ptz_krt_covariance_batch_device": (lambda lib, a: lib.ptz_krt_covariance_batch_device(a["n"], *_batch(a), a["ft"], None, None, D0, _p(a["cov"]),
                                                                                           _p(a["s0"]), _p(a["st"]), None),
                                        ("ptr", "uvr", "uvc", "cref", "ccur", "cov", "s0", "st")),
    "ptz_krt_residuals_batch": (lambda lib, a: lib.ptz_krt_residuals_batch(a["n"], *_batch(a), a["ft"], None, None, 0, 0, _p(a["err"]), None, _p(a["rms"]),
                                                                           _p(a["mx"]), _p(a["med"]), _p(a["cnt"]), _p(a["rms3"]), _p(a["ms"])),
                                ("ptr", "uvr", "uvc", "cref", "ccur")),
    "ptz_krt_residuals_batch_device": (lambda lib, a: lib.ptz_krt_residuals_batch_device(a["n"], *_batch(a), a["ft"], None, None, 0, _p(a["err"]), None,
                                                                                         _p(a["rms"]), _p(a["mx"]), _p(a["med"]), _p(a["cnt"]), _p(a["rms3"]),
                                                                                         None),
                                       ("ptr", "uvr", "uvc", "cref", "ccur")),
    "ptz_krt_solve_batch_trimmed": (lambda lib, a: lib.ptz_krt_solve_batch_trimmed(a["n"], *_batch(a), a["ft"], D100, None, None, None, _p(a["summ"]),
                                                                                   _p(a["acc"]), _p(a["kept"]), _p(a["rep"]), _p(a["ms"])),
                                    ("ptr", "uvr", "uvc", "cref", "ccur", "summ", "acc")),
    "ptz_krt_solve_batch_trimmed_device": (lambda lib, a: lib.ptz_krt_solve_batch_trimmed_device(
        a["n"], C.c_int64(NM), *_batch(a), a["ft"], D100, None, None, None, _p(a["summ"]), _p(a["acc"]), _p(a["kept"]), _p(a["rep"]), _p(a["work"]),
        C.c_int64(0 if a["work"] is None else a["work"].nbytes), None), ("ptr", "uvr", "uvc", "cref", "ccur", "summ", "acc", "work")),
}


def _points(a, pptr=(0, 1, 2, 3), p2=True, p3=True):
    a["pptr"] = np.array(pptr, dtype=np.int64)
    a["p2"] = np.zeros((3, 2), np.float32) if p2 else None
    a["p3"] = np.ones((3, 3)) if p3 else None


def _decreasing(a):
    a["ptr"][2] = a["ptr"][1] - 1


def _cases(required):
    """the malformed calls of one entry point: name -> what it does to the arguments"""
    c = {"n_query=-1": lambda a: a.update(n=-1), "n_query=0": lambda a: a.update(n=0), "match_ptr decreasing": _decreasing,
         "match_ptr[0]=1": lambda a: a["ptr"].__setitem__(0, 1), "point_ptr decreasing": lambda a: _points(a, pptr=(0, 2, 1, 3)),
         "point_ptr with pts2d null": lambda a: _points(a, p2=False), "point_ptr with pts3d null": lambda a: _points(a, p3=False),
         "factor_type=4": lambda a: a.update(ft=4), "factor_type=-1": lambda a: a.update(ft=-1)}
    for k in required:
        c[k + " null"] = lambda a, k=k: a.update({k: None})
    return c


def run_case(lib, entry, case):
    """(return code, every output still as it was poisoned)"""
    call, required = ENTRIES[entry]
    a = _args(lib)
    _cases(required)[case](a)
    before = {k: a[k].copy() for k in OUTPUTS if a[k] is not None}
    rc = int(call(lib, a))
    return rc, all(np.array_equal(a[k], v) for k, v in before.items())


def record(lib):
    """the fixture's content from a library (run once on the commit before the change, on a machine without a GPU)"""
    rows = {}
    for entry, (_, required) in ENTRIES.items():
        rows[entry] = {}
        for case in _cases(required):
            rc, untouched = run_case(lib, entry, case)
            assert untouched, (entry, case)
            rows[entry][case] = {"rc": rc, "reaches_device": rc == ENODEVICE}
    return {"return_codes": rows, "trim_workspace_bytes": {"%d,%d" % s: _workspace_bytes(lib, *s) for s in WORKSPACE_SHAPES}}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_malformed_calls_are_answered_as_before_and_touch_no_output(golden, entry):
    api = tu.pkg().api
    lib, want = api.lib(), golden["return_codes"][entry]
    assert sorted(want) == sorted(_cases(ENTRIES[entry][1]))  # the fixture and the table list the same calls
    have_device = api.device_count() > 0
    for case, row in want.items():
        assert row["reaches_device"] == (row["rc"] == ENODEVICE), (entry, case)
        if row["reaches_device"] and have_device:
            continue  # machine-dependent (see the head of the file)
        rc, untouched = run_case(lib, entry, case)
        assert rc == row["rc"] and untouched, (entry, case, rc, row["rc"], untouched)


def test_trim_workspace_bytes_are_what_callers_sized_their_buffers_by(golden):
    lib = tu.pkg().api.lib()
    assert sorted(golden["trim_workspace_bytes"]) == sorted("%d,%d" % s for s in WORKSPACE_SHAPES)
    for s in WORKSPACE_SHAPES:
        assert _workspace_bytes(lib, *s) == golden["trim_workspace_bytes"]["%d,%d" % s], s
