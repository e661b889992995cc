"""The host harness of the prior's contract (tests/cpu_harness/reloc_prior_harness.cc) behind ctypes, and the cameras the prior
tests share: references and priors as rotation vectors [tilt, pan, roll] on one centre, so that a prior near a reference in pan and
tilt overlaps it, one 180 degrees in pan has the rig behind it and one tilted 90 degrees looks away from every reference."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

import reloc_assemble_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_h = None


def harness():
    global _h
    if _h is None:
        _h = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "libreloc_prior_harness.so"))
        for f in (_h.h_prior_homography, _h.h_prior_query_K, _h.h_reloc_prior, _h.h_reloc_prior_camera):
            f.restype = None
    return _h


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness_homography(cam_from, R_from, cam_to, R_to):
    a, b = np.ascontiguousarray(cam_from, dtype=np.float64), np.ascontiguousarray(cam_to, dtype=np.float64)
    Ra, Rb = np.ascontiguousarray(R_from, dtype=np.float64).reshape(9), np.ascontiguousarray(R_to, dtype=np.float64).reshape(9)
    H = np.zeros(9)
    harness().h_prior_homography(_p(a), _p(Ra), _p(b), _p(Rb), _p(H))
    return H


def harness_query_K(prior, w, h, factor_type):
    p = np.ascontiguousarray(prior, dtype=np.float64)
    K = np.zeros(4)
    harness().h_prior_query_K(_p(p), int(w), int(h), int(factor_type), _p(K))
    return K


def harness_prior_pairs(ref_cams, ref_R, prior_cams, prior_R, query_wh, factor_type=0, max_refs=8, min_overlap=8):
    cams = np.ascontiguousarray(ref_cams, dtype=np.float64).reshape(-1, 15)
    pri = np.ascontiguousarray(prior_cams, dtype=np.float64).reshape(-1, 15)
    Rr = np.ascontiguousarray(ref_R, dtype=np.float64).reshape(-1, 9)
    Rq = np.ascontiguousarray(prior_R, dtype=np.float64).reshape(-1, 9)
    wh = np.ascontiguousarray(query_wh, dtype=np.int32).reshape(-1, 2)
    nq, n_ref, R = len(pri), len(cams), int(max_refs)
    sl = np.full((nq, R), -1, dtype=np.int32)
    ns = np.zeros(nq, dtype=np.int32)
    ov = np.zeros((nq, n_ref), dtype=np.int32)
    Hs = np.zeros((nq, R, 9))
    harness().h_reloc_prior(n_ref, _p(cams), _p(Rr), nq, _p(pri), _p(Rq), _p(wh), int(factor_type), R, int(min_overlap), _p(sl), _p(ns), _p(ov),
                            _p(Hs))
    return dict(shortlist=sl, n_short=ns, overlap=ov, H_slot=Hs)


def harness_prior_camera(cam_cur, prior_cams, factor_type):
    out = np.array(cam_cur, dtype=np.float64).reshape(-1, 15).copy()
    pri = np.ascontiguousarray(prior_cams, dtype=np.float64).reshape(-1, 15)
    harness().h_reloc_prior_camera(len(out), _p(out), _p(pri), int(factor_type))
    return out


rotations = ru.harness_rotations  # (the one host function both the references' and the priors' matrices come from, in the tests)


def make_cams(n, seed, pan=(-60.0, 60.0), tilt=(-15.0, 15.0), f=(1500.0, 4000.0), dist=False):
    """n cameras [n, 15] on one centre with rotation vector [tilt, pan, roll], fy within 2 % of fx, image centres of three frame sizes."""
    rng = np.random.default_rng(seed)
    cams = np.zeros((n, 15))
    sizes = [(960.0, 540.0), (640.0, 360.0), (1024.0, 768.0)]
    for i in range(n):
        cams[i, 0] = rng.uniform(*f)
        cams[i, 1] = cams[i, 0] * rng.uniform(0.98, 1.02)
        cams[i, 2], cams[i, 3] = sizes[i % 3]
        cams[i, 4:7] = [math.radians(rng.uniform(*tilt)), math.radians(rng.uniform(*pan)), math.radians(rng.uniform(-1, 1))]
        cams[i, 7:10] = rng.uniform(-1, 1, 3)
        if dist:
            cams[i, 10] = rng.uniform(-0.05, 0.05)
            cams[i, 11:15] = rng.uniform(-1e-3, 1e-3, 4)
    return cams


def make_priors(n, seed, behind=(), away=(), **kw):
    """(prior cameras [n, 15], query_wh int32 [n, 2]); the queries of `behind` pan 180 degrees on (the rig is behind them), those of
    `away` tilt 90 degrees up (no reference in sight)."""
    cams = make_cams(n, seed, **kw)
    rng = np.random.default_rng(seed + 1000)
    wh = np.stack([rng.integers(600, 4000, n), rng.integers(400, 2200, n)], axis=1).astype(np.int32)
    for q in behind:
        cams[q, 4:7] = [0.0, cams[q, 5] + math.pi, 0.0]
    for q in away:
        cams[q, 4:7] = [math.pi / 2, 0.0, 0.0]
    return cams, wh
