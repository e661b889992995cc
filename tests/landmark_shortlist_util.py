"""The landmark shortlist's contract (ptz-calib_amd/csrc/ptz_landmark_shortlist.h) restated in numpy: the home groups by a stable
sort, the votes and lists by desc_shortlist_util over the grouped rows, the view by a plain np.isin.  The yardstick of the CPU
harness (tests/cpu_harness/landmark_shortlist_harness.cc) and of the device kernels; nothing here is shared with either."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import desc_shortlist_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_h = None


def home_groups(lm_home, n_ref):
    """dict(home_ptr [n_ref + 1] int64, home_lm [n_lm] int32): the landmarks of home r in ascending landmark index."""
    home = np.asarray(lm_home, dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(home, minlength=int(n_ref))[:int(n_ref)])]).astype(np.int64)
    return dict(home_ptr=ptr, home_lm=np.argsort(home, kind="stable").astype(np.int32))


def home_images(lm_desc, lm_home, n_ref):
    """The home set's images: a list of n_ref uint8 arrays [*, D]."""
    g = home_groups(lm_home, n_ref)
    return su.images(np.asarray(lm_desc)[g["home_lm"]], g["home_ptr"])


def shortlist(lm_desc, lm_home, n_ref, q_desc, q_ptr, query_img=None, cache=None, **opt):
    """desc_shortlist_util.shortlist over the grouped rows: dict(shortlist [n_query, R], n_short, votes [n_query, n_ref])."""
    g = home_groups(lm_home, n_ref)
    return su.shortlist(np.asarray(lm_desc)[g["home_lm"]], g["home_ptr"], q_desc, q_ptr, query_img=query_img, cache=cache, **opt)


def view(lm_home, lists):
    """dict(vis_ptr [n_query + 1] int64, vis_lm [n_vis] int32) of lists [n_query, R] (-1: unused slot)."""
    home = np.asarray(lm_home)
    lists = np.asarray(lists)
    lists = lists.reshape(len(lists), lists.shape[1] if lists.ndim == 2 else 1)
    rows = [np.nonzero(np.isin(home, row[row >= 0]))[0] for row in lists]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    lm = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, dtype=np.int32)
    return dict(vis_ptr=ptr, vis_lm=lm)


def lift(view_, table):
    """The landmark index of every match of a table over the pairs (view image q, query q), pair q = query q."""
    pair_of = np.repeat(np.arange(len(table["match_ptr"]) - 1), np.diff(table["match_ptr"]))
    return view_["vis_lm"][view_["vis_ptr"][pair_of] + table["idx_a"]].astype(np.int32)


def all_homes(lm_home, n_ref, n_query):
    """The list [n_query, n_ref] that names every non-empty home (ascending, -1 behind)."""
    used = np.unique(np.asarray(lm_home))
    row = np.full(int(n_ref), -1, dtype=np.int32)
    row[:len(used)] = used
    return np.tile(row, (int(n_query), 1))


# ------------------------------------------------------------------------------------------------------------- the host harness
def harness():
    global _h
    if _h is None:
        _h = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "liblandmark_shortlist_harness.so"))
        for f in (_h.h_lm_home_groups, _h.h_lm_shortlist, _h.h_lm_view):
            f.restype = C.c_int32
    return _h


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness_groups(lm_home, n_ref):
    home = np.ascontiguousarray(lm_home, dtype=np.int32)
    ptr, lm = np.zeros(int(n_ref) + 1, dtype=np.int64), np.zeros(max(len(home), 1), dtype=np.int32)
    rc = harness().h_lm_home_groups(_p(home) if len(home) else None, len(home), int(n_ref), _p(ptr), _p(lm))
    return rc, dict(home_ptr=ptr, home_lm=lm[:len(home)])


def harness_shortlist(lm_desc, lm_home, n_ref, q, M, R, min_votes=1, ratio=0.8, max_dist2=0, seed=1, parts=3):
    """(votes [n_ref], row [R], n_short) of one query image q [n, D] against the home set of the map"""
    desc = np.ascontiguousarray(lm_desc, dtype=np.uint8)
    D = desc.shape[1]
    home = np.ascontiguousarray(lm_home, dtype=np.int32)
    qq = np.ascontiguousarray(q, dtype=np.uint8)
    votes, row = np.zeros(max(int(n_ref), 1), dtype=np.int32), np.zeros(int(R), dtype=np.int32)
    n = harness().h_lm_shortlist(_p(desc) if desc.size else None, _p(home) if len(home) else None, len(home), int(n_ref), _p(qq) if qq.size else None,
                                 len(q), D, int(M), int(R), int(min_votes), C.c_double(ratio), int(max_dist2), C.c_uint64(seed), int(parts),
                                 _p(votes), _p(row))
    return votes[:int(n_ref)], row, n


def harness_view(lm_home, n_ref, lists, device_form=False):
    """(rc, view): the host form checks the entries (rc = -1: PTZ_EINVAL), the device form ignores what is out of range"""
    home = np.ascontiguousarray(lm_home, dtype=np.int32)
    lists = np.ascontiguousarray(lists, dtype=np.int32)
    lists = lists.reshape(len(lists), lists.shape[1] if lists.ndim == 2 else 1)
    nq, R = lists.shape
    ptr, lm = np.zeros(nq + 1, dtype=np.int64), np.zeros(max(nq * len(home), 1), dtype=np.int32)
    rc = harness().h_lm_view(_p(home) if len(home) else None, len(home), int(n_ref), nq, R, _p(lists) if lists.size else None, int(device_form),
                             _p(ptr), _p(lm))
    return rc, dict(vis_ptr=ptr, vis_lm=lm[:int(ptr[-1])] if rc == 0 else lm[:0])


def assert_equal(got, want, what="", keys=("vis_ptr", "vis_lm")):
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


# ------------------------------------------------------------------------------------------------------------------ generated cases
def make_map(n_lm, n_ref, D, seed=0, empty=()):
    """(lm_desc [n_lm, D] uint8, lm_home [n_lm] int32): random rows, homes drawn from the references not in `empty`"""
    rng = np.random.default_rng(seed)
    hi = 4 if D == 1 else 256
    homes = np.array([r for r in range(n_ref) if r not in set(empty)], dtype=np.int32)
    return rng.integers(0, hi, (n_lm, D), dtype=np.uint8), (homes[rng.integers(0, len(homes), n_lm)] if n_lm else np.zeros(0, dtype=np.int32))


def make_query(lm_desc, n, seed=0, noise=6):
    """A query image [n, D]: random rows, a third of them noisy copies of landmarks (so that votes are neither 0 nor all)"""
    rng = np.random.default_rng(seed)
    D = lm_desc.shape[1]
    hi = 4 if D == 1 else 256
    q = rng.integers(0, hi, (n, D), dtype=np.uint8)
    k = min(len(lm_desc), n) // 3
    if k:
        src = lm_desc[rng.permutation(len(lm_desc))[:k]].astype(np.int64)
        q[rng.permutation(n)[:k]] = np.clip(src + rng.integers(-noise, noise + 1, (k, D)), 0, hi - 1)
    return q
