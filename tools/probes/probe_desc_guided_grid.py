#!/usr/bin/env python3
"""Measurement of the grid-binned guided kernel beside the scan kernel (a probe, not a test; no threshold).

One process, both kernels warmed up, alternating turns, minima and medians.  Before anything is timed the two kernels' arrays
(match_ptr, idx_a, idx_b, dist2, uv_a, uv_b) are asserted equal at every shape.
  (a) offline   probe_desc_guided.py's shape: all pairs of 200 images x 2000 features, D = 128, ground-truth pair homographies,
                radius 4 px: device_ms of ptz_desc_match_pairs_guided and of ptz_desc_match_pairs_guided_grid.
  (b) tracked   probe_reloc_prior.py's shape: 1000 queries x 2000 features, 200 references, R = 8, radius 40 px.  The matcher alone
                on the run's own pairs and predicted homographies (api.reloc_prior_pairs), both kernels, and the dense matcher on
                the same pairs; then wall time of ptz_relocalizer_run_tracked with guided_grid 0 and 1 beside
                ptz_relocalizer_run_shortlisted.
  (c) one query the first query of (b) alone: the matcher's device time and the tracked run's wall time, both kernels.

usage: probe_desc_guided_grid.py [--images 200] [--features 2000] [--queries 1000] [--dim 128] [--turns 5] [--skip a|b|c ...]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as ge  # noqa: E402
from probe_desc_guided import views  # noqa: E402
from probe_reloc_shortlist import features  # noqa: E402

KEYS = ("match_ptr", "idx_a", "idx_b", "dist2", "uv_a", "uv_b")


def stats(v):
    return dict(min=float(np.min(v)), median=float(np.median(v)))


def matcher_ab(api, sa, sb, ia, ib, H, radius, turns, dense=False, **opt):
    """device_ms of the scan and the grid kernel on the same pairs, alternating, after the equality check (which warms both up)"""
    s = api.match_descriptors_guided(sa, sb, ia, ib, H, None, radius, **opt)
    g = api.match_descriptors_guided(sa, sb, ia, ib, H, None, radius, grid=True, **opt)
    for k in KEYS:
        assert np.array_equal(s[k], g[k]), k
    t = dict(scan=[], grid=[], dense=[])
    for _ in range(turns):
        for name, kw in (("scan", {}), ("grid", dict(grid=True))):
            m = api.match_descriptors_guided(sa, sb, ia, ib, H, None, radius, resident=True, **kw, **opt)
            t[name].append(m.device_ms)
            m.close()
        if dense:
            m = api.match_descriptors(sa, sb, ia, ib, resident=True, **opt)
            t["dense"].append(m.device_ms)
            m.close()
    out = dict(pairs=int(len(ia)), radius_px=radius, matches=int(len(s["idx_a"])), scan_ms=stats(t["scan"]), grid_ms=stats(t["grid"]),
               grid_over_scan=float(np.min(t["grid"]) / np.min(t["scan"])))
    if dense:
        out["dense_ms"] = stats(t["dense"])
    return out


def wall(f, turns_of):
    t0 = time.perf_counter()
    r = f()
    turns_of.append(1e3 * (time.perf_counter() - t0))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--turns", type=int, default=5)
    ap.add_argument("--refs", type=int, default=8)
    ap.add_argument("--skip", nargs="*", default=[])
    a = ap.parse_args()
    pkg = ge.load_package()
    api = pkg.api
    out = dict(lib=os.path.basename(api.LIB_PATH), D=a.dim, turns=a.turns)
    if "a" not in a.skip:
        rng = np.random.default_rng(0)
        ptr, desc, kp, Hw = views(rng, a.images, a.features, a.dim)
        ia, ib = (x.astype(np.int32) for x in np.triu_indices(a.images, k=1))
        Hp = np.stack([Hw[y] @ np.linalg.inv(Hw[x]) for x, y in zip(ia, ib)])
        Hp /= Hp[:, 2:3, 2:3]
        with api.DescSet(ptr, desc, kp) as s:
            out["a_offline"] = matcher_ab(api, s, s, ia, ib, Hp.reshape(-1, 9), 4.0, a.turns, min_matches=8)
        print(json.dumps(dict(a_offline=out["a_offline"])), file=sys.stderr, flush=True)
    if "b" not in a.skip or "c" not in a.skip:
        rng = np.random.default_rng(0)
        n_ref, nq = a.images, a.queries
        rig = pkg.synth.make_scene(0, n_ref, 20).cam_gt  # only the cameras matter
        base = rng.integers(0, 256, (4 * a.features, a.dim), dtype=np.uint8)
        base_xy = rng.uniform([100, 100], [1820, 980], (len(base), 2)).astype(np.float32)
        rd, rk, rp = features(rng, n_ref, a.features, a.dim, base, base_xy)
        qd, qk, qp = features(rng, nq, a.features, a.dim, base, base_xy)
        wh = np.tile(np.array([1920, 1080], dtype=np.int32), (nq, 1))
        priors = pkg.synth_reloc.perturb_cameras(rig[np.arange(nq) % n_ref], 0.3, 0.02, seed=0)
        match = dict(min_matches=8)

        def pair_list(n):
            pp = api.reloc_prior_pairs(rig, priors[:n], wh[:n], factor_type=0, radius_px=40.0, max_refs=a.refs)
            pa, pb, H = [], [], []
            for q in range(n):
                for k in range(int(pp["n_short"][q])):
                    pa.append(int(pp["shortlist"][q, k])); pb.append(q); H.append(pp["H_slot"][q, k])
            return np.asarray(pa, dtype=np.int32), np.asarray(pb, dtype=np.int32), np.asarray(H, dtype=np.float64).reshape(-1, 9)

        def runs(rl, tests, n, shortlisted):
            pr = dict(cams=priors[:n], radius_px=40.0, max_refs=a.refs)
            f = dict(scan=lambda: rl.run(tests, wh[:n], max_refs=1, match=match, prior=pr),
                     grid=lambda: rl.run(tests, wh[:n], max_refs=1, match=match, prior=pr, guided_grid=True))
            if shortlisted:
                f["shortlisted"] = lambda: rl.run(tests, wh[:n], max_refs=1, match=match, shortlist=dict(max_refs=a.refs, n_probes=256))
            first = {k: g() for k, g in f.items()}  # warm-up of every shape of the timed window
            for k in ("cam", "accepted", "n_matches", "n_inliers", "sel_ref"):
                assert np.array_equal(first["scan"][k], first["grid"][k], equal_nan=True), k
            t = {k: [] for k in f}
            stage = {k: [] for k in f}
            for _ in range(a.turns):
                for k, g in f.items():
                    stage[k].append(wall(g, t[k])["stage_ms"])
            res = {k + "_wall_ms": stats(v) for k, v in t.items()}
            res.update({k + "_stage_ms_min": [float(x) for x in np.min(np.array(v), axis=0)] for k, v in stage.items()})
            res["accepted"] = {k: int(v["accepted"].sum()) for k, v in first.items()}
            res["tracked_grid_over_tracked_scan"] = float(np.median(t["grid"]) / np.median(t["scan"]))
            if shortlisted:
                res["tracked_grid_over_shortlisted"] = float(np.median(t["grid"]) / np.median(t["shortlisted"]))
                res["tracked_scan_over_shortlisted"] = float(np.median(t["scan"]) / np.median(t["shortlisted"]))
            return res

        with api.DescSet(rp, rd, rk) as refs:
            if "b" not in a.skip:
                pa, pb, H = pair_list(nq)
                with api.DescSet(qp, qd, qk) as tests, api.Relocalizer(refs, rig) as rl:
                    out["b_tracked_matcher"] = matcher_ab(api, refs, tests, pa, pb, H, 40.0, a.turns, dense=True, **match)
                    out["b_tracked_runs"] = runs(rl, tests, nq, True)
                print(json.dumps(dict(b_tracked_matcher=out["b_tracked_matcher"], b_tracked_runs=out["b_tracked_runs"])), file=sys.stderr, flush=True)
            if "c" not in a.skip:
                pa, pb, H = pair_list(1)
                cut = int(qp[1])
                with api.DescSet(qp[:2], qd[:cut], qk[:cut]) as tests, api.Relocalizer(refs, rig) as rl:
                    out["c_one_query_matcher"] = matcher_ab(api, refs, tests, pa, pb, H, 40.0, max(a.turns, 9), **match)
                    out["c_one_query_runs"] = runs(rl, tests, 1, False)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
