#!/usr/bin/env python3
"""Measurement of relocalization against the landmark map THROUGH THE PROBE-VOTE SHORTLIST beside the dense landmark run and the
shortlisted run against reference images (a probe, not a test; no threshold; reads nothing outside the repository).

The online shape and the consistent geometry of probe_reloc_landmarks_tracked.py, whose generators it imports: 1000 queries x 2000
features, 200 references x 2000 features, D = 128, about 80 000 landmarks, query q behind the camera of reference q mod 200.  In ONE
process, after a warm-up of each, alternating turns of
  landmarks               api.Relocalizer.run(..., landmarks=map)                                       ptz_relocalizer_run_landmarks
  shortlisted             api.Relocalizer.run(..., shortlist=dict(max_refs=8, n_probes=256))            ptz_relocalizer_run_shortlisted
  landmarks_shortlist_R   api.Relocalizer.run(..., landmarks=map, landmark_shortlist=dict(max_refs=R, n_probes=256))
for R = the R of profiles/landmark_shortlist_accuracy_cpu.json, 2 R, and --more (default 16: the homes a query of this shape sees).
Reports minimum and median wall time of each (host clock around calls that end in a stream wait), the per-stage device times (votes,
view, matcher, assembly, solve -- events on the run's stream), accepted queries, matches per query, the median focal error, the
view's size, and the same runs on ONE query alone.

usage: probe_reloc_landmarks_shortlisted.py [--images 200] [--features 2000] [--queries 1000] [--dim 128] [--turns 3] [--world 80000]
                                            [--more 16] [--out profiles/landmark_shortlist_probe.json]
Prints one JSON line and writes it to --out."""
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
from probe_reloc_landmarks_tracked import H, W, images, tracks_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--world", type=int, default=80000)
    ap.add_argument("--more", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landmark_shortlist_probe.json"))
    a = ap.parse_args()
    pkg = ge.load_package()
    api = pkg.api
    R0 = json.load(open(os.path.join(ROOT, "profiles", "landmark_shortlist_accuracy_cpu.json")))["chosen_R"]
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
    Rs = sorted({R0, 2 * R0, a.more})
    out = dict(shape="online: %d queries x %d features, %d references x %d features" % (nq, a.features, n_ref, a.features), D=a.dim,
               n_tracks=int(len(tp) - 1), turns=a.turns, n_probes=256, R_of_the_accuracy_probe=R0, R_measured=Rs)
    m8 = dict(min_matches=8)
    one = int(qp[1])
    with api.DescSet(rp, rd, rk) as refs, api.DescSet(qp, qd, qk) as tests, api.DescSet(qp[:2], qd[:one], qk[:one]) as single, \
            api.Relocalizer(refs, rig) as rl, api.LandmarkMap(refs, rig, tp, ti, tf) as lmap:
        t0 = time.perf_counter()
        groups = lmap.home_groups()
        lmap.home_set()
        sizes = np.diff(groups["home_ptr"])
        out.update(n_landmarks=lmap.n_landmarks, home_set_build_wall_ms=1e3 * (time.perf_counter() - t0), non_empty_homes=int((sizes > 0).sum()),
                   home_size_median=float(np.median(sizes)), home_size_max=int(sizes.max()))
        # the dense run's matches per home: how many homes a query's matches live in
        dense = rl.run(tests, wh, landmarks=lmap, match=m8)
        tab = rl.table()
        home = lmap.arrays()["lm_home"]
        per = [len(np.unique(home[tab["idx_a"][tab["match_ptr"][q]:tab["match_ptr"][q + 1]]])) for q in range(nq)]
        out.update(homes_with_a_dense_match_median=float(np.median(per)), homes_with_a_dense_match_max=int(np.max(per)))
        for batch, T, w in (("", tests, wh), ("one_query_", single, wh[:1])):
            runs = dict(landmarks=lambda T=T, w=w: rl.run(T, w, landmarks=lmap, match=m8),
                        shortlisted=lambda T=T, w=w: rl.run(T, w, max_refs=1, match=m8, shortlist=dict(max_refs=8, n_probes=256)))
            for R in Rs:
                runs["landmarks_shortlist_%d" % R] = lambda T=T, w=w, R=R: rl.run(T, w, landmarks=lmap, match=m8,
                                                                                  landmark_shortlist=dict(max_refs=R, n_probes=256))
            for f in runs.values():
                f()  # warm-up of every shape of the timed window
            wall, stage, extra, last = ({k: [] for k in runs} for _ in range(4))
            for _ in range(a.turns):
                for k, f in runs.items():
                    t0 = time.perf_counter()
                    last[k] = f()
                    wall[k].append(1e3 * (time.perf_counter() - t0))
                    stage[k].append(last[k]["stage_ms"])
                    extra[k].append([last[k].get("votes_ms", last[k].get("shortlist_ms", 0.0)), last[k].get("view_ms", 0.0)])
            gt = q_cam[:len(w), 0]
            for k in runs:
                acc = last[k]["accepted"] == 1
                st, ex = np.median(np.array(stage[k]), axis=0), np.median(np.array(extra[k]), axis=0)
                rec = dict(wall_ms_min=float(np.min(wall[k])), wall_ms_median=float(np.median(wall[k])), wall_ms_turns=[float(x) for x in wall[k]],
                           votes_ms=float(ex[0]), view_ms=float(ex[1]), matcher_ms=float(st[0] + st[1]), assembly_ms=float(st[2]), gate_ms=float(st[3]),
                           solve_ms=float(st[4]), accepted=int(acc.sum()), matches_median=float(np.median(last[k]["n_matches"])),
                           median_rel_focal_err=float(np.median(np.abs(last[k]["cam"][acc, 0] - gt[acc]) / gt[acc])) if acc.any() else None)
                if "n_visible" in last[k]:
                    nv = last[k]["n_visible"]
                    rec.update(n_visible_median=float(np.median(nv)), n_visible_max=int(nv.max()), n_short_median=float(np.median(last[k]["n_short"])),
                               lost_vs_dense=int(((last["landmarks"]["accepted"] == 1) & ~acc).sum()),
                               dense_matches_share=float(last[k]["n_matches"].sum() / max(int(last["landmarks"]["n_matches"].sum()), 1)))
                out[batch + k] = rec
            for R in Rs:
                out[batch + "landmarks_shortlist_%d_over_landmarks_wall" % R] = out[batch + "landmarks_shortlist_%d" % R]["wall_ms_median"] / out[batch + "landmarks"]["wall_ms_median"]
                out[batch + "landmarks_shortlist_%d_over_shortlisted_wall" % R] = out[batch + "landmarks_shortlist_%d" % R]["wall_ms_median"] / out[batch + "shortlisted"]["wall_ms_median"]
        del dense
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
