#!/usr/bin/env python3
"""Measurement of relocalization against a landmark map beside the two runs against reference images (a probe, not a test; no
threshold; reads nothing outside the repository).

Online shape: 1000 queries x 2000 features, 200 references x 2000 features, D = 128.  The references' features are noisy copies of
80 000 world descriptors, every reference a draw without replacement, so a world point is seen by five references on average: the
tracks have mean length about 5 and the map about 80 000 landmarks, one fifth of the resident rows.  In ONE process, after a warm-up of each,
alternating turns of
  all pairs    api.Relocalizer.run (ptz_relocalizer_run): every (reference, query) pair through the matcher;
  shortlisted  api.Relocalizer.run(..., shortlist=dict(max_refs=8, n_probes=256)) (ptz_relocalizer_run_shortlisted);
  landmarks    api.Relocalizer.run(..., landmarks=map) (ptz_relocalizer_run_landmarks): one (map, query) pair per query.
Reports minimum and median wall time of each (host clock around calls that end in a stream wait), the stage times of each, and the
one-off map build (device time of its launches, and wall time with the upload of the tracks, the download of the map and the packing
of its descriptor set).  All references carry ONE camera and a world point one pixel (plus noise) in every image that sees it, so the
geometry is consistent and the solves see the match counts a rig would give them; what the runs find is the tests' subject.

usage: probe_reloc_landmarks.py [--images 200] [--features 2000] [--queries 1000] [--dim 128] [--turns 3] [--track_len 5]
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
import __graft_entry__ as ge  # noqa: E402


def images(rng, n_img, n_feat, D, base, base_xy, share, noise=12):
    """n_img images of n_feat features: the first share * n_feat of every image are noisy copies of DISTINCT rows of base at their
    pixels (plus a pixel of noise), the rest uniform.  Returns (desc, xy, feat_ptr, pick [n_img, k]: the copied rows)."""
    d = rng.integers(0, 256, (n_img * n_feat, D), dtype=np.uint8)
    xy = rng.uniform([0, 0], [1920, 1080], (n_img * n_feat, 2)).astype(np.float32)
    k = int(share * n_feat)
    picks = np.zeros((n_img, k), dtype=np.int64)
    for m in range(n_img):
        pick = rng.choice(len(base), k, replace=False)
        picks[m] = pick
        d[m * n_feat:m * n_feat + k] = np.clip(base[pick].astype(np.int16) + rng.integers(-noise, noise + 1, (k, D)), 0, 255).astype(np.uint8)
        xy[m * n_feat:m * n_feat + k] = base_xy[pick] + rng.normal(0, 1.0, (k, 2)).astype(np.float32)
    return d, xy, (np.arange(n_img + 1) * n_feat).astype(np.int64), picks


def tracks_of(picks):
    """CSR of the tracks: one per base row some image copies, its views in ascending image order"""
    n_img, k = picks.shape
    img = np.repeat(np.arange(n_img), k)
    feat = np.tile(np.arange(k), n_img)
    order = np.lexsort((img, picks.reshape(-1)))
    _, counts = np.unique(picks.reshape(-1)[order], return_counts=True)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), img[order].astype(np.int32), feat[order].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--track_len", type=float, default=5.0)
    a = ap.parse_args()
    pkg = ge.load_package()
    api = pkg.api
    rng = np.random.default_rng(0)
    n_ref, nq = a.images, a.queries
    rig = np.tile(pkg.synth.make_scene(0, 4, 20).cam_gt[:1], (n_ref, 1))  # one camera for all: consistent rays whatever is drawn
    n_world = int(n_ref * a.features / a.track_len)
    base = rng.integers(0, 256, (n_world, a.dim), dtype=np.uint8)
    base_xy = rng.uniform([100, 100], [1820, 980], (n_world, 2)).astype(np.float32)
    rd, rk, rp, picks = images(rng, n_ref, a.features, a.dim, base, base_xy, 1.0)
    qd, qk, qp, _ = images(rng, nq, a.features, a.dim, base, base_xy, 0.5)
    tp, ti, tf = tracks_of(picks)
    wh = np.tile(np.array([1920, 1080], dtype=np.int32), (nq, 1))
    sl = dict(max_refs=8, n_probes=256)
    out = dict(shape="online: %d queries x %d features, %d references x %d features" % (nq, a.features, n_ref, a.features), D=a.dim,
               n_tracks=int(len(tp) - 1), mean_track_length=float(len(ti) / max(len(tp) - 1, 1)), turns=a.turns)
    with api.DescSet(rp, rd, rk) as refs, api.DescSet(qp, qd, qk) as tests, api.Relocalizer(refs, rig) as rl:
        builds = []
        lmap = None
        for _ in range(3):  # the one-off build, three times (the first warms the kernels)
            if lmap is not None:
                lmap.close()
            t0 = time.perf_counter()
            lmap = api.LandmarkMap(refs, rig, tp, ti, tf)
            builds.append((1e3 * (time.perf_counter() - t0), lmap.build_ms))
        out.update(n_landmarks=lmap.n_landmarks, map_build_wall_ms=[b[0] for b in builds], map_build_device_ms=[b[1] for b in builds],
                   resident_rows_references=int(n_ref * a.features), mac_ratio_landmarks_over_all_pairs=lmap.n_landmarks / float(n_ref * a.features))
        runs = dict(all_pairs=lambda: rl.run(tests, wh, max_refs=1, match=dict(min_matches=8)),
                    shortlisted=lambda: rl.run(tests, wh, max_refs=1, match=dict(min_matches=8), shortlist=sl),
                    landmarks=lambda: rl.run(tests, wh, landmarks=lmap, match=dict(min_matches=8)))
        for f in runs.values():
            f()  # warm-up of every shape of the timed window
        wall = {k: [] for k in runs}
        stage = {k: [] for k in runs}
        last = {}
        for _ in range(a.turns):
            for k, f in runs.items():
                t0 = time.perf_counter()
                last[k] = f()
                wall[k].append(1e3 * (time.perf_counter() - t0))
                stage[k].append(last[k]["stage_ms"])
        for k in runs:
            out[k + "_wall_ms_min"] = float(np.min(wall[k]))
            out[k + "_wall_ms_median"] = float(np.median(wall[k]))
            out[k + "_wall_ms_turns"] = [float(x) for x in wall[k]]
            out[k + "_stage_ms_median"] = [float(x) for x in np.median(np.array(stage[k]), axis=0)]
            out[k + "_accepted"] = int(last[k]["accepted"].sum())
            out[k + "_matches_median"] = float(np.median(last[k]["n_matches"]))
        out["shortlist_vote_pass_ms"] = float(last["shortlisted"]["shortlist_ms"])
        out["landmarks_over_all_pairs_wall"] = out["landmarks_wall_ms_median"] / out["all_pairs_wall_ms_median"]
        out["landmarks_over_shortlisted_wall"] = out["landmarks_wall_ms_median"] / out["shortlisted_wall_ms_median"]
        lmap.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
