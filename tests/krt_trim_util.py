"""Shared by test_cpu_krt_trim.py, test_gpu_krt_residuals.py and test_gpu_krt_trim.py: the contaminated relocalization batches, the
numpy restatement of the rule of ptz-calib_amd/csrc/ptz_krt_trim.h, the host instantiation of that header
(tests/cpu_harness/krt_trim_harness.cc), the trimmed loop written on the CPU oracle alone, and the manual loop over the library's
public calls that ptz_krt_solve_batch_trimmed must equal bit for bit.

The oracle loop shares no code with the library: solves are oracle_py.krt_solve_batch with the open bound, residuals the oracle's
functors as krt_cov_util.Restatement takes them.  Every oracle loop is computed once per process and shared (lru_cache)."""
import ctypes as C
import functools
import os
import subprocess
import types

import numpy as np

import __graft_entry__ as ge
import krt_cov_util as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYLEIGH_MEDIAN = 1.1774
OPEN_BOUND = 1e300
CONTINUE, DONE, MAX_ROUNDS, MIN_KEEP, REJECTED = -1, 0, 2, 4, 8
DEFAULTS = dict(trim_px=4.0, k_sigma=3.0, max_rounds=8, min_keep=8)
SEED_ID = 7
# (factor type, contaminated fraction of each query's matches, mode): 'displaced' by 20..80 px in a random direction, 'random' =
# replaced by a uniform pixel of the frame
CASES = [(ft, frac, mode) for ft in (0, 1) for frac in (0.1, 0.3) for mode in ("displaced", "random")]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def orc():
    o = ge.load_oracle()
    o.build()
    return o


@functools.lru_cache(maxsize=None)
def pkg():
    return ge.load_package()


@functools.lru_cache(maxsize=None)
def restatement():
    return cu.Restatement()


HARNESS_SRC = os.path.join(ROOT, "tests", "cpu_harness", "krt_trim_harness.cc")


@functools.lru_cache(maxsize=None)
def harness():
    so = os.path.join(ROOT, "tests", "cpu_harness", "libkrt_trim_harness.so")
    srcs = [HARNESS_SRC] + [os.path.join(ROOT, "ptz-calib_amd", "csrc", h) for h in ("ptz_krt_trim.h", "ptz_ba_trim.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, HARNESS_SRC])
    return C.CDLL(so)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def round_restated(err, in_u, in_k, rounds_run, trim_px=4.0, k_sigma=3.0, max_rounds=8, min_keep=8):
    """numpy restatement of one round of one query: (decision, new_k [n] bool, t, median)"""
    err = np.asarray(err, dtype=np.float64)
    in_u = np.ones(len(err), dtype=bool) if in_u is None else np.asarray(in_u) != 0
    in_k = np.asarray(in_k) != 0
    skipped = err < 0
    counted = np.sort(err[in_k & ~skipped])
    median = counted[(len(counted) - 1) // 2] if len(counted) else np.nan
    t = trim_px
    if k_sigma > 0 and len(counted):
        t = max(trim_px, k_sigma * median / RAYLEIGH_MEDIAN)
    new_k = in_u & (skipped | (err <= t))
    if (new_k == in_k).all():
        d = DONE
    elif int((new_k & ~skipped).sum()) < min_keep:
        d = MIN_KEEP
    elif rounds_run >= max_rounds:
        d = MAX_ROUNDS
    else:
        d = CONTINUE
    return d, new_k, t, median


def round_header(err, in_u, in_k, rounds_run, trim_px=4.0, k_sigma=3.0, max_rounds=8, min_keep=8):
    """the header's rule on the host (krt_trim_harness.cc): the same tuple as round_restated"""
    err = np.ascontiguousarray(err, dtype=np.float64)
    u = None if in_u is None else np.ascontiguousarray(np.asarray(in_u) != 0, dtype=np.uint8)
    k = np.ascontiguousarray(np.asarray(in_k) != 0, dtype=np.uint8)
    new_k = np.full(len(err), 7, dtype=np.uint8)
    t, med = C.c_double(), C.c_double()
    d = harness().h_krt_trim_round(C.c_double(trim_px), C.c_double(k_sigma), C.c_int(max_rounds), C.c_int(min_keep), C.c_int64(len(err)),
                                   _p(err), _p(u), _p(k), C.c_int(rounds_run), _p(new_k), C.byref(t), C.byref(med))
    return d, new_k != 0, t.value, med.value


# ---- batches ----------------------------------------------------------------------------------------------------------------------
def as_batch(**kw):
    b = types.SimpleNamespace(point_ptr=None, pts2d=None, pts3d=None)
    b.__dict__.update(kw)
    return b


@functools.lru_cache(maxsize=None)
def clean_batch(ft, n_query=24, n_match=128):
    return pkg().synth.make_reloc_batch(n_query, n_match, seed_id=SEED_ID, factor_type=ft)


@functools.lru_cache(maxsize=None)
def contaminated_batch(ft, frac, mode, n_query=24, n_match=128, seed=1):
    """(batch, wrong [n_match_total] bool): round(frac n_match) matches of EACH query, chosen without replacement, get a wrong
    current-image pixel (float32)"""
    rb = clean_batch(ft, n_query, n_match)
    rng = np.random.default_rng(seed)
    uvc = np.array(rb.uv_cur, dtype=np.float32).copy()
    wrong = np.zeros(len(uvc), dtype=bool)
    k = int(round(frac * n_match))
    for q in range(n_query):
        idx = q * n_match + rng.choice(n_match, size=k, replace=False)
        if mode == "displaced":
            ang = rng.uniform(0.0, 2.0 * np.pi, k)
            mag = rng.uniform(20.0, 80.0, k)
            uvc[idx] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1).astype(np.float32)
        else:
            uvc[idx] = rng.uniform([0, 0], [1920, 1080], (k, 2)).astype(np.float32)
        wrong[idx] = True
    b = as_batch(n_query=rb.n_query, match_ptr=np.asarray(rb.match_ptr, dtype=np.int64), uv_ref=np.asarray(rb.uv_ref, dtype=np.float32),
                 uv_cur=uvc, cam_ref=rb.cam_ref, cam_init=rb.cam_init, cam_gt=rb.cam_gt, factor_type=ft)
    return b, wrong


def sub_batch(b, queries, sel=None, cam_init=None):
    """the queries `queries` of b with the matches whose sel byte is non-zero (all if None), order kept; points as they are"""
    ptr = np.asarray(b.match_ptr, dtype=np.int64)
    uvr, uvc, new_ptr = [], [], [0]
    for q in queries:
        a, e = int(ptr[q]), int(ptr[q + 1])
        s = np.ones(e - a, dtype=bool) if sel is None else np.asarray(sel[a:e]) != 0
        uvr.append(np.asarray(b.uv_ref)[a:e][s]); uvc.append(np.asarray(b.uv_cur)[a:e][s])
        new_ptr.append(new_ptr[-1] + int(s.sum()))
    cat = lambda xs, w, dt: np.ascontiguousarray(np.concatenate(xs).reshape(-1, w), dtype=dt) if xs else np.zeros((0, w), dtype=dt)
    o = as_batch(n_query=len(queries), match_ptr=np.array(new_ptr, dtype=np.int64), uv_ref=cat(uvr, 2, np.float32), uv_cur=cat(uvc, 2, np.float32),
                 cam_ref=np.ascontiguousarray(np.asarray(b.cam_ref)[queries]),
                 cam_init=np.ascontiguousarray((np.asarray(b.cam_init) if cam_init is None else cam_init)[queries]), factor_type=b.factor_type)
    if getattr(b, "point_ptr", None) is not None:
        pp = np.asarray(b.point_ptr, dtype=np.int64)
        p2, p3, new_pp = [], [], [0]
        for q in queries:
            a, e = int(pp[q]), int(pp[q + 1])
            p2.append(np.asarray(b.pts2d)[a:e]); p3.append(np.asarray(b.pts3d)[a:e])
            new_pp.append(new_pp[-1] + e - a)
        o.point_ptr, o.pts2d, o.pts3d = np.array(new_pp, dtype=np.int64), cat(p2, 2, np.float32), cat(p3, 3, np.float64)
    return o


# ---- residuals through the oracle's functors ----------------------------------------------------------------------------------------
def oracle_errors(ft, ref, cur_world, uv_ref, uv_cur):
    """|e_m| [n] of one query at the world-frame camera cur_world, -1 where the restatement's border guard skips"""
    rs = restatement()
    uv_ref = np.ascontiguousarray(uv_ref, dtype=np.float32).reshape(-1, 2)
    uv_cur = np.ascontiguousarray(uv_cur, dtype=np.float32).reshape(-1, 2)
    cam = rs.orc.krt_world_to_local(ref, cur_world)
    res = rs._residuals(ft, ref, cam, uv_ref, uv_cur, np.zeros((0, 2), np.float32), np.zeros((0, 3)))
    err = np.sqrt(res[:, 0] ** 2 + res[:, 1] ** 2)
    if ft & 1:
        err[rs._skip(ref, uv_ref)] = -1.0
    return err


def oracle_point_errors(ft, ref, cur_world, pts2d, pts3d):
    rs = restatement()
    pts2d = np.ascontiguousarray(pts2d, dtype=np.float32).reshape(-1, 2)
    cam = rs.orc.krt_world_to_local(ref, cur_world)
    Xl = rs.orc.krt_point_to_local(ref, pts3d) if len(pts2d) else np.zeros((0, 3))
    res = rs._residuals(ft, ref, cam, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), pts2d, Xl)
    return np.sqrt(res[:, 0] ** 2 + res[:, 1] ** 2)


# ---- the loop ---------------------------------------------------------------------------------------------------------------------
def _final_reproj(s):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(2.0) * np.sqrt(np.float64(2 * s["final_cost"]) / np.float64(s["num_residuals"]))


def run_loop(b, solve, errors, rule, mask=None, max_reproj_error=100.0, trim=None):
    """The trimmed loop of include/ptz_calib_amd.h over a batch, with the pieces handed in:
      solve(sub_batch) -> (cam_world [k, 15], summaries, accepted)   -- run with the OPEN bound by the caller's closure
      errors(queries, cams [n, 15], kept, accepted_round [n]) -> (err [n_match_total], rms [n] or None): only the entries of
                                                                 `queries` are read; rms = None: taken from err with numpy
      rule(err, in_u, in_k, rounds_run, **trim) -> (decision, new_k, t, median).
    Returns dict(cam [n, 15], summaries, accepted [n], kept [n_match], reports (list of dicts), margin): margin = the smallest
    |e_m - t| over every round, query and match of the universe that is not skipped."""
    trim = dict(DEFAULTS, **(trim or {}))
    n = b.n_query
    ptr = np.asarray(b.match_ptr, dtype=np.int64)
    nm = int(ptr[-1])
    U = np.ones(nm, dtype=bool) if mask is None else np.asarray(mask) != 0
    K = U.copy()
    cam = np.array(b.cam_init, dtype=np.float64).copy()
    summ = [None] * n
    acc_round = np.zeros(n, dtype=np.int32)
    rep = [dict(rounds=0, flags=0, n_removed=0, n_kept=0, threshold=np.nan, rms_first=np.nan, rms_last=np.nan, median_last=np.nan)
           for _ in range(n)]
    active = list(range(n))
    margin = np.inf
    for r in range(trim["max_rounds"]):
        if not active:
            break
        sb = sub_batch(b, active, K, cam_init=cam)
        c, s, a = solve(sb)
        for i, q in enumerate(active):
            summ[q] = s[i]
            acc_round[q] = a[i]
            if a[i]:
                cam[q] = c[i]
        err, rms_all = errors(active, cam, K, acc_round)
        go_on = []
        for q in active:
            lo, hi = int(ptr[q]), int(ptr[q + 1])
            rq = rep[q]
            rq["rounds"] = r + 1
            if not acc_round[q]:
                rq["flags"] = REJECTED
                rq["n_kept"] = int(K[lo:hi].sum()); rq["n_removed"] = int(U[lo:hi].sum()) - rq["n_kept"]
                continue
            e = err[lo:hi]
            d, new_k, t, med = rule(e, U[lo:hi], K[lo:hi], r + 1, **trim)
            judged = U[lo:hi] & (e >= 0)
            if judged.any():
                margin = min(margin, float(np.abs(e[judged] - t).min()))
            cnt = K[lo:hi] & (e >= 0)
            rms = float(rms_all[q]) if rms_all is not None else (float(np.sqrt(np.mean(e[cnt] ** 2))) if cnt.any() else np.nan)
            if d == CONTINUE:
                K[lo:hi] = new_k
                go_on.append(q)
            rq["flags"] = 0 if d == CONTINUE else d
            rq["n_kept"] = int(K[lo:hi].sum()); rq["n_removed"] = int(U[lo:hi].sum()) - rq["n_kept"]
            rq["threshold"] = t
            if r == 0:
                rq["rms_first"] = rms
            rq["rms_last"] = rms
            rq["median_last"] = med
        active = go_on
    accepted = np.array([1 if (acc_round[q] and _final_reproj(summ[q]) < max_reproj_error) else 0 for q in range(n)], dtype=np.int32)
    out = np.array(b.cam_init, dtype=np.float64).copy()
    out[accepted != 0] = cam[accepted != 0]
    return dict(cam=out, summaries=summ, accepted=accepted, kept=K.astype(np.uint8), reports=rep, margin=margin)


@functools.lru_cache(maxsize=None)
def oracle_loop(ft, frac, mode, max_rounds=8):
    """the loop on the CPU oracle alone over contaminated_batch(ft, frac, mode) (frac = 0: the clean batch)"""
    b = contaminated_batch(ft, frac, mode)[0] if frac > 0 else clean_as_batch(ft)
    return oracle_loop_on(b, trim=dict(max_rounds=max_rounds))


def clean_as_batch(ft):
    rb = clean_batch(ft)
    return as_batch(n_query=rb.n_query, match_ptr=np.asarray(rb.match_ptr, dtype=np.int64), uv_ref=np.asarray(rb.uv_ref, dtype=np.float32),
                    uv_cur=np.asarray(rb.uv_cur, dtype=np.float32), cam_ref=rb.cam_ref, cam_init=rb.cam_init, cam_gt=rb.cam_gt, factor_type=ft)


def oracle_loop_on(b, mask=None, max_reproj_error=100.0, trim=None, **opt):
    o = orc()
    ft = b.factor_type
    ptr = np.asarray(b.match_ptr, dtype=np.int64)

    def solve(sb):
        return o.krt_solve_batch(sb, max_reproj_error=OPEN_BOUND, **opt)

    def errors(queries, cams, kept, acc_round):
        err = np.full(int(ptr[-1]), np.nan)
        for q in queries:
            if acc_round[q]:
                lo, hi = int(ptr[q]), int(ptr[q + 1])
                err[lo:hi] = oracle_errors(ft, b.cam_ref[q], cams[q], b.uv_ref[lo:hi], b.uv_cur[lo:hi])
        return err, None

    return run_loop(b, solve, errors, round_restated, mask, max_reproj_error, trim)


def manual_loop_on(b, mask=None, max_reproj_error=100.0, trim=None, **opt):
    """the loop over the library's public calls: ptz_krt_solve_batch[_2d3d] with the open bound, ptz_krt_residuals_batch, the rule
    header on the host, a compaction in numpy"""
    api = pkg().api

    def solve(sb):
        c, s, a, _ = api.krt_solve_batch(sb, max_reproj_error=OPEN_BOUND, **opt)
        return c, s, a

    def errors(queries, cams, kept, acc_round):
        r = api.krt_residuals_batch(b, cams, match_mask=kept.astype(np.uint8), accepted=acc_round,
                                    lanes_per_query=opt.get("krt_lanes_per_query", 0))
        return r["err_px"], r["rms"]

    return run_loop(b, solve, errors, round_header, mask, max_reproj_error, trim)
