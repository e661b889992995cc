#!/usr/bin/env python3
"""Measurement of relocalization against the landmark map FROM A PRIOR beside the dense landmark run and the two fast runs against
reference images (a probe, not a test; no threshold; reads nothing outside the repository).  The method of probe_reloc_landmarks.py.

Online shape: 1000 queries x 2000 features, 200 references x 2000 features, D = 128, about 80 000 landmarks.  Unlike the earlier
probes this one needs a consistent GEOMETRY, because the view is cut by it: the references are the 200 cameras of
synth.make_scene(0, 200, 20) (a full turn of pan at three tilts), the world is 80 000 rays drawn inside their frames, a reference
holds (up to) 2000 of the rays its frame sees as noisy copies of their descriptors at their projected pixels (1 px of noise), and
query q looks through the camera of reference q mod 200 with half of its features such copies.  Priors: the queries' cameras turned
by 0.3 degrees, the focal 2 % off; radius 40 px; guided_grid = 1.  In ONE process, after a warm-up of each, alternating turns of
  landmarks          api.Relocalizer.run(..., landmarks=map)                                  ptz_relocalizer_run_landmarks
  tracked            api.Relocalizer.run(..., prior=dict(cams=, radius_px=40, max_refs=8))    ptz_relocalizer_run_tracked
  shortlisted        api.Relocalizer.run(..., shortlist=dict(max_refs=8, n_probes=256))       ptz_relocalizer_run_shortlisted
  landmarks_tracked  api.Relocalizer.run(..., landmarks=map, landmark_prior=dict(cams=, radius_px=40))
Reports minimum and median wall time of each (host clock around calls that end in a stream wait), the stage times, n_visible, the
view's bytes and the accepted counts.

usage: probe_reloc_landmarks_tracked.py [--images 200] [--features 2000] [--queries 1000] [--dim 128] [--turns 3] [--world 80000]
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

W, H = 1920, 1080


def project(cam, R, X):
    """pixels of world rays X [n, 3] in a pinhole camera, and which of them lie 8 px inside its frame"""
    pc = X @ R.T
    with np.errstate(all="ignore"):
        u = cam[0] * pc[:, 0] / pc[:, 2] + cam[2]
        v = cam[1] * pc[:, 1] / pc[:, 2] + cam[3]
    return u, v, (pc[:, 2] > 0.1) & (u >= 8) & (u <= W - 8) & (v >= 8) & (v <= H - 8)


def images(rng, cams, Rs, X, base, n_feat, share, D, noise=12):
    """one image per camera: up to share * n_feat of the world rays its frame sees (drawn without replacement) as noisy copies at
    their pixels, the rest uniform.  Returns (desc, xy, feat_ptr, the rays copied per image)."""
    n = len(cams)
    d = rng.integers(0, 256, (n * n_feat, D), dtype=np.uint8)
    xy = rng.uniform([0, 0], [W, H], (n * n_feat, 2)).astype(np.float32)
    picks = []
    for m in range(n):
        u, v, vis = project(cams[m], Rs[m], X)
        seen = np.nonzero(vis)[0]
        pick = np.sort(rng.choice(seen, min(int(share * n_feat), len(seen)), replace=False))
        k = len(pick)
        d[m * n_feat:m * n_feat + k] = np.clip(base[pick].astype(np.int16) + rng.integers(-noise, noise + 1, (k, D)), 0, 255).astype(np.uint8)
        xy[m * n_feat:m * n_feat + k] = np.stack([u[pick], v[pick]], axis=1) + rng.normal(0, 1.0, (k, 2))
        picks.append(pick)
    return d, xy, (np.arange(n + 1) * n_feat).astype(np.int64), picks


def tracks_of(picks):
    """CSR of the tracks: one per world ray some image copies, its views in ascending image order"""
    img = np.concatenate([np.full(len(p), m) for m, p in enumerate(picks)])
    feat = np.concatenate([np.arange(len(p)) for p in picks])
    ray = np.concatenate(picks)
    order = np.lexsort((img, ray))
    _, counts = np.unique(ray[order], return_counts=True)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), img[order].astype(np.int32), feat[order].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--world", type=int, default=80000)
    a = ap.parse_args()
    pkg = ge.load_package()
    api = pkg.api
    rng = np.random.default_rng(0)
    n_ref, nq = a.images, a.queries
    rig = pkg.synth.make_scene(0, n_ref, 20).cam_gt.copy()
    rig[:, 10:] = 0.0
    Rr = np.stack([pkg.synth.rodrigues(c[4:7]) for c in rig])
    # the world: rays through uniform pixels of references drawn at random
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
    sl = dict(max_refs=8, n_probes=256)
    out = dict(shape="online: %d queries x %d features, %d references x %d features" % (nq, a.features, n_ref, a.features), D=a.dim,
               n_tracks=int(len(tp) - 1), mean_track_length=float(len(ti) / max(len(tp) - 1, 1)), turns=a.turns, radius_px=40.0, prior="0.3 deg, 2 %")
    m8 = dict(min_matches=8)
    with api.DescSet(rp, rd, rk) as refs, api.DescSet(qp, qd, qk) as tests, api.Relocalizer(refs, rig) as rl, \
            api.LandmarkMap(refs, rig, tp, ti, tf) as lmap:
        out.update(n_landmarks=lmap.n_landmarks, map_build_device_ms=lmap.build_ms)
        with api.landmark_visible(lmap, priors, wh, radius_px=40.0, max_view_bytes=16 << 30) as v:  # the view alone, once: its size
            nv = np.diff(v.arrays()["vis_ptr"])
            rows = int(((nv + 63) // 64 * 64).sum() + 64)
            out.update(n_visible_median=float(np.median(nv)), n_visible_min=int(nv.min()), n_visible_max=int(nv.max()), n_visible_total=int(nv.sum()),
                       view_rows=rows, view_bytes=int(rows * (64 * ((a.dim + 63) // 64) + 4) + 12 * nv.sum()), view_alone_device_ms=v.device_ms)
        fits = out["view_bytes"] + (1 << 20) < (2 << 30)  # the library's default max_view_bytes; beyond it a caller splits the batch
        out["view_fits_default_max_view_bytes"] = bool(fits)
        lpri = dict(cams=priors, radius_px=40.0) if fits else dict(cams=priors, radius_px=40.0, max_view_bytes=16 << 30)
        runs = dict(landmarks=lambda: rl.run(tests, wh, landmarks=lmap, match=m8),
                    tracked=lambda: rl.run(tests, wh, max_refs=1, match=m8, prior=dict(cams=priors, radius_px=40.0, max_refs=8), guided_grid=True),
                    shortlisted=lambda: rl.run(tests, wh, max_refs=1, match=m8, shortlist=sl),
                    landmarks_tracked=lambda: rl.run(tests, wh, landmarks=lmap, landmark_prior=lpri, guided_grid=True, match=m8))
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
        gt = q_cam[:, 0]
        for k in runs:
            acc = last[k]["accepted"] == 1
            out[k + "_wall_ms_min"] = float(np.min(wall[k]))
            out[k + "_wall_ms_median"] = float(np.median(wall[k]))
            out[k + "_wall_ms_turns"] = [float(x) for x in wall[k]]
            out[k + "_stage_ms_median"] = [float(x) for x in np.median(np.array(stage[k]), axis=0)]
            out[k + "_accepted"] = int(acc.sum())
            out[k + "_matches_median"] = float(np.median(last[k]["n_matches"]))
            out[k + "_median_rel_focal_err"] = float(np.median(np.abs(last[k]["cam"][acc, 0] - gt[acc]) / gt[acc])) if acc.any() else None
        lost = np.nonzero(last["landmarks_tracked"]["accepted"] == 0)[0]
        out["landmarks_tracked_lost"] = dict(queries=lost[:12].tolist(), n_visible=last["landmarks_tracked"]["n_visible"][lost[:12]].tolist(),
                                             n_matches=last["landmarks_tracked"]["n_matches"][lost[:12]].tolist(),
                                             n_inliers=last["landmarks_tracked"]["n_inliers"][lost[:12]].tolist(),
                                             n_inliers_median_all=float(np.median(last["landmarks_tracked"]["n_inliers"])),
                                             dense_accepts_them=bool((last["landmarks"]["accepted"][lost] == 1).all()))
        out["shortlist_vote_pass_ms"] = float(last["shortlisted"]["shortlist_ms"])
        out["tracked_prior_ms"] = float(last["tracked"]["prior_ms"])
        out["landmarks_tracked_view_ms"] = float(last["landmarks_tracked"]["view_ms"])
        for k in ("landmarks", "tracked", "shortlisted"):
            out["landmarks_tracked_over_" + k + "_wall"] = out["landmarks_tracked_wall_ms_median"] / out[k + "_wall_ms_median"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
