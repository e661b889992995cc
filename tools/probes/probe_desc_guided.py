#!/usr/bin/env python3
"""Measurement of the guided matcher beside the dense one (a probe, not a test).

Offline shape: 200 images x 2000 features, D = 128, all 19 900 unordered pairs, both directions (cross_check), ground-truth pair
homographies, radius 4 px.  The images are views of one planar canvas of points (rotation, zoom, shift: every pair has an exact
homography H_b H_a^-1); an image holds the canvas points it sees, up to 70 % of its features, and uniform distractors.  Times
device_ms of ptz_desc_match_pairs_guided beside device_ms of ptz_desc_match_pairs on the same pairs, in one process, alternating,
`--runs` turns after a warm-up of each, and reports minimum and median of both and their ratio.

The one condition the design rests on: the guided pass takes less device time than the dense pass (a radius search that is not
cheaper would mean masking the dense kernel was the simpler design).  The exit status is 1 if it does not hold.

usage: probe_desc_guided.py [--images 200] [--features 2000] [--dim 128] [--radius 4] [--runs 7]
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

W, H_PX = 1920, 1080


def views(rng, n_img, n_feat, D, share=0.7, noise=12):
    """(feat_ptr, desc, kp, world-to-image homographies [n_img, 3, 3])"""
    n_world = 40 * n_feat
    world = rng.uniform([0, 0], [3 * W, 3 * H_PX], (n_world, 2))
    base = rng.integers(0, 256, (n_world, D), dtype=np.uint8)
    descs, kps, Hs = [], [], []
    for m in range(n_img):
        ang, zoom = rng.uniform(-0.2, 0.2), rng.uniform(0.8, 1.25)
        c, s = zoom * np.cos(ang), zoom * np.sin(ang)
        centre = rng.uniform([0.8 * W, 0.8 * H_PX], [2.2 * W, 2.2 * H_PX])
        A = np.array([[c, -s], [s, c]])
        t = np.array([W / 2, H_PX / 2]) - A @ centre
        Hm = np.array([[c, -s, t[0]], [s, c, t[1]], [0, 0, 1.0]])
        uv = world @ A.T + t
        seen = np.flatnonzero((uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H_PX))[:int(share * n_feat)]
        k = len(seen)
        d = rng.integers(0, 256, (n_feat, D), dtype=np.uint8)
        d[:k] = np.clip(base[seen].astype(np.int16) + rng.integers(-noise, noise + 1, (k, D)), 0, 255).astype(np.uint8)
        p = rng.uniform([0, 0], [W, H_PX], (n_feat, 2))
        p[:k] = uv[seen]
        descs.append(d); kps.append(p.astype(np.float32)); Hs.append(Hm)
    return (np.arange(n_img + 1) * n_feat).astype(np.int64), np.concatenate(descs), np.concatenate(kps), np.stack(Hs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--radius", type=float, default=4.0)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    pkg = ge.load_package()
    rng = np.random.default_rng(0)
    ptr, desc, kp, Hw = views(rng, a.images, a.features, a.dim)
    ia, ib = (x.astype(np.int32) for x in np.triu_indices(a.images, k=1))
    Hp = np.stack([Hw[y] @ np.linalg.inv(Hw[x]) for x, y in zip(ia, ib)])
    Hp /= Hp[:, 2:3, 2:3]
    dense_ms, guided_ms, n_dense, n_guided = [], [], 0, 0
    with pkg.api.DescSet(ptr, desc, kp) as s:
        for r in range(a.runs + 1):
            d = pkg.api.match_descriptors(s, s, ia, ib, resident=True, min_matches=8)
            g = pkg.api.match_descriptors_guided(s, s, ia, ib, Hp.reshape(-1, 9), None, a.radius, resident=True, min_matches=8)
            if r:
                dense_ms.append(d.device_ms); guided_ms.append(g.device_ms)
            n_dense, n_guided, chunks = d.n_matches, g.n_matches, (d.n_chunks, g.n_chunks)
            d.close(); g.close()
    candidates = 2.0 * len(ia) * a.features * a.features
    out = dict(shape="offline: all pairs of %d images" % a.images, pairs=int(len(ia)), features=a.features, D=a.dim, radius_px=a.radius,
               runs=a.runs, dense_ms_min=min(dense_ms), dense_ms_median=float(np.median(dense_ms)), guided_ms_min=min(guided_ms),
               guided_ms_median=float(np.median(guided_ms)), guided_over_dense=min(guided_ms) / min(dense_ms), dense_matches=n_dense,
               guided_matches=n_guided, n_chunks=chunks, candidate_tests=candidates,
               guided_ns_per_wave_candidate=min(guided_ms) * 1e6 / (candidates / 64))
    print(json.dumps(out), flush=True)
    return 0 if min(guided_ms) < min(dense_ms) else 1


if __name__ == "__main__":
    sys.exit(main())
