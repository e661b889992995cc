#!/usr/bin/env python3
"""Measurement of the rotation-and-focal gate beside the homography gate (a probe, not a test; no threshold; reads nothing outside the
repository).  Geometry and shape of probe_reloc_landmarks_tracked.py: 1000 queries x 2000 features, 200 references, about 80 000
landmarks, priors 0.3 degrees and 2 % off, radius 40 px, about 1000 assembled matches per query.

Part 1, the gates alone.  One tracked landmark run leaves its table and view; the landmark assembly of them (api.landmark_assemble, the
run's own arrays) gives the assembled CSR and the two cameras.  On these SAME host arrays, in one process, after a warm-up of each,
alternating turns of api.gate_matches (ptz_match_gate_run, max_pair_matches 4096) and api.RotFocalGate.run (ptz_rotfocal_gate_run,
iters 128): the device time between the events around the gate's kernels, every turn, with minima and medians; queries with a model,
queries kept, matches kept.
Part 2, the runs.  ptz_relocalizer_run_landmarks_tracked and ptz_relocalizer_run_tracked with gate_model 0 and 1 the same way: wall
time, stage 4's device time, accepted count and median relative focal error.

usage: probe_rotfocal_gate.py [--images 200] [--features 2000] [--queries 1000] [--dim 128] [--turns 5] [--world 80000] [--iters 128]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

torch.cuda.init()
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import __graft_entry__ as ge  # noqa: E402
from probe_reloc_landmarks_tracked import W, H, images, tracks_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--turns", type=int, default=5)
    ap.add_argument("--world", type=int, default=80000)
    ap.add_argument("--iters", type=int, default=128)
    a = ap.parse_args()
    pkg = ge.load_package()
    api = pkg.api
    rng = np.random.default_rng(0)
    n_ref, nq = a.images, a.queries
    rig = pkg.synth.make_scene(0, n_ref, 20).cam_gt.copy()
    rig[:, 10:] = 0.0
    Rr = np.stack([pkg.synth.rodrigues(c[4:7]) for c in rig])
    src = rng.integers(0, n_ref, a.world)
    px = rng.uniform([8, 8], [W - 8, H - 8], (a.world, 2))
    n = np.stack([(px[:, 0] - rig[src, 2]) / rig[src, 0], (px[:, 1] - rig[src, 3]) / rig[src, 1], np.ones(a.world)], axis=1)
    X = np.einsum("nji,nj->ni", Rr[src], n)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    base = rng.integers(0, 256, (a.world, a.dim), dtype=np.uint8)
    rd, rk, rp, picks = images(rng, rig, Rr, X, base, a.features, 1.0, a.dim)
    q_cam = rig[np.arange(nq) % n_ref]
    qd, qk, qp, _ = images(rng, q_cam, Rr[np.arange(nq) % n_ref], X, base, a.features, 0.5, a.dim)
    tp, ti, tf = tracks_of(picks)
    wh = np.tile(np.array([W, H], dtype=np.int32), (nq, 1))
    priors = pkg.synth_reloc.perturb_cameras(q_cam, 0.3, 0.02, seed=0)
    out = dict(shape="online: %d queries x %d features, %d references x %d features" % (nq, a.features, n_ref, a.features), D=a.dim, turns=a.turns,
               iters=a.iters, radius_px=40.0, prior="0.3 deg, 2 %", thresh_px=4.0, min_inliers=6)
    m8 = dict(min_matches=8)
    gt = q_cam[:, 0]
    with api.DescSet(rp, rd, rk) as refs, api.DescSet(qp, qd, qk) as tests, api.Relocalizer(refs, rig) as rl, \
            api.LandmarkMap(refs, rig, tp, ti, tf) as lmap:
        lpri = dict(cams=priors, radius_px=40.0, max_view_bytes=16 << 30)
        # ---- part 1: both gates on the same assembled arrays
        rl.run(tests, wh, landmarks=lmap, landmark_prior=lpri, guided_grid=True, match=m8)
        view, g = rl.view(), rl.table()
        pair_of = np.repeat(np.arange(nq), np.diff(g["match_ptr"]))
        lifted = view["vis_lm"][view["vis_ptr"][pair_of] + g["idx_a"]].astype(np.int32)
        asm = api.landmark_assemble(lmap, g["match_ptr"], lifted, g["uv_b"], wh)
        ptr, ua, ub, cref, ccur = asm["match_ptr"], asm["uv_ref"], asm["uv_cur"], asm["cam_ref"], asm["cam_init"]
        sizes = np.diff(ptr)
        out.update(assembled_matches=int(ptr[-1]), assembled_per_query_median=float(np.median(sizes)), assembled_per_query_max=int(sizes.max()))
        with api.MatchGate(nq, len(ua), 4096) as hg, api.RotFocalGate(nq, len(ua)) as rg:
            gates = dict(homography=lambda: api.gate_matches(ptr, ua, ub, ransac_thresh=4.0, min_inliers=6, gate=hg),
                         rotfocal=lambda: rg.run(ptr, ua, ub, cref, ccur, thresh=4.0, min_inliers=6, iters=a.iters))
            for f in gates.values():
                f()
            ms = {k: [] for k in gates}
            last = {}
            for _ in range(a.turns):
                for k, f in gates.items():
                    last[k] = f()
                    ms[k].append(float(last[k]["device_ms"]))
        for k in gates:
            kept = np.diff(last[k]["out_ptr"])
            out["gate_" + k] = dict(device_ms_turns=ms[k], device_ms_min=float(np.min(ms[k])), device_ms_median=float(np.median(ms[k])),
                                    with_model=int((last[k]["found"] == 1).sum()), not_served=int((last[k]["found"] == -1).sum()),
                                    queries_kept=int((kept > 0).sum()), matches_kept=int(kept.sum()),
                                    queries_keeping_nothing_of_500_or_more=int(((kept == 0) & (sizes >= 500)).sum()))
        out["rotfocal_below_homography_in_every_turn"] = bool(all(r < h for r, h in zip(ms["rotfocal"], ms["homography"])))
        out["homography_over_rotfocal_median"] = out["gate_homography"]["device_ms_median"] / out["gate_rotfocal"]["device_ms_median"]
        # ---- part 2: the two tracked runs under either gate
        runs = {}
        for model in (0, 1):
            runs["landmarks_tracked_gate%d" % model] = lambda model=model: rl.run(tests, wh, landmarks=lmap, landmark_prior=lpri, guided_grid=True, match=m8,
                                                                                 gate_model=model, gate_iters=a.iters)
            runs["tracked_gate%d" % model] = lambda model=model: rl.run(tests, wh, max_refs=1, match=m8, prior=dict(cams=priors, radius_px=40.0, max_refs=8),
                                                                       guided_grid=True, gate_model=model, gate_iters=a.iters)
        for f in runs.values():
            f()
        wall, stage, last = {k: [] for k in runs}, {k: [] for k in runs}, {}
        for _ in range(a.turns):
            for k, f in runs.items():
                t0 = time.perf_counter()
                last[k] = f()
                wall[k].append(1e3 * (time.perf_counter() - t0))
                stage[k].append(last[k]["stage_ms"])
        for k in runs:
            acc = last[k]["accepted"] == 1
            out[k] = dict(wall_ms_turns=[float(x) for x in wall[k]], wall_ms_min=float(np.min(wall[k])), wall_ms_median=float(np.median(wall[k])),
                          stage_ms_median=[float(x) for x in np.median(np.array(stage[k]), axis=0)], accepted=int(acc.sum()),
                          matches_median=float(np.median(last[k]["n_matches"])), inliers_median=float(np.median(last[k]["n_inliers"])),
                          median_rel_focal_err=float(np.median(np.abs(last[k]["cam"][acc, 0] - gt[acc]) / gt[acc])) if acc.any() else None)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
