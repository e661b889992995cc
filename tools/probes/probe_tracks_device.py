#!/usr/bin/env python3
"""Measurement of the device tracks against the host detour they replace (a probe, not a test; no threshold).

Offline shape: 200 images x 2000 features, D = 128, all 19 900 pairs (probe_desc_match.py's descriptors), the match table resident
after the matcher; and one reference set's worth, 20 images, where launch latency dominates.  Two routes from the resident table to
a landmark map, in one process, alternating, five turns after a warm-up of each:
  device  ptz_tracks_from_matches + ptz_landmark_map_create_from_tracks: wall time of each, and the tracks' device time between events
  host    what run_ptz_reloc --landmarks does today: download of the table, ptzh_tracks_build (the host TracksBuilder: Build, Filter,
          both exports), ptz_landmark_map_create: wall time per part
First the two maps are asserted equal after canonicalisation (the host's tracks ranked by the node of their first view), then the
minimum and the median per route are reported.

usage: probe_tracks_device.py [--images 200 20] [--features 2000] [--turns 5] [--out profiles/tracks_device_probe.json]
Prints one JSON line per shape and writes them to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as ge  # noqa: E402
import host_util as hu  # noqa: E402
from probe_desc_match import descriptors  # noqa: E402

_p = lambda a: a.ctypes.data_as(C.c_void_p)


def host_tracks(ia, ib, table, min_len):
    """ptzh_tracks_build on the downloaded table: (trk_ptr, trk_img, trk_feat) in the builder's order"""
    src, dst = ia.astype(np.int64), ib.astype(np.int64)
    tid, tptr, ei, ef = C.POINTER(C.c_int32)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
    nt = hu.lib().ptzh_tracks_build(len(ia), _p(src), _p(dst), _p(table["match_ptr"]), _p(table["idx_a"]), _p(table["idx_b"]), min_len,
                                    C.byref(tid), C.byref(tptr), C.byref(ei), C.byref(ef))
    assert nt >= 0
    ptr = np.ctypeslib.as_array(tptr, (nt + 1,)).copy()
    nv = int(ptr[-1])
    img = np.ctypeslib.as_array(ei, (max(nv, 1),))[:nv].copy()
    feat = np.ctypeslib.as_array(ef, (max(nv, 1),))[:nv].copy()
    for x in (tid, tptr, ei, ef):
        hu.lib().ptzh_free(x)
    return ptr, img, feat


def run_shape(pkg, n_img, n_feat, D, turns, min_len=2):
    api = pkg.api
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (4 * n_feat, D), dtype=np.uint8)
    desc, fptr = descriptors(rng, n_img, n_feat, D, base)
    kp = rng.uniform([0, 0], [1920, 1080], (len(desc), 2)).astype(np.float32)
    cams = np.resize(pkg.synth.make_scene(0, 20, 100).cam_gt, (n_img, 15)).copy()
    ia, ib = (x.astype(np.int32) for x in np.triu_indices(n_img, k=1))
    rows = dict(device_wall_ms=[], device_tracks_wall_ms=[], device_tracks_device_ms=[], device_map_wall_ms=[], host_wall_ms=[],
                host_download_ms=[], host_tracks_ms=[], host_map_ms=[])
    with api.DescSet(fptr, desc, kp) as ds, api.match_descriptors(ds, ds, ia, ib, resident=True, min_matches=8) as m:
        def device_route():
            t0 = time.perf_counter()
            t = api.tracks_from_matches(ds, m, ia, ib, min_len=min_len)
            t1 = time.perf_counter()
            lmap = api.LandmarkMap.from_tracks(ds, cams, t, min_views=min_len)
            t2 = time.perf_counter()
            return t, lmap, (1e3 * (t2 - t0), 1e3 * (t1 - t0), t.device_ms, 1e3 * (t2 - t1))

        def host_route():
            t0 = time.perf_counter()
            table = m.download(uv=False)
            t1 = time.perf_counter()
            ptr, img, feat = host_tracks(ia, ib, table, min_len)
            t2 = time.perf_counter()
            lmap = api.LandmarkMap(ds, cams, ptr, img, feat, min_views=min_len)
            t3 = time.perf_counter()
            return (ptr, img, feat), lmap, (1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2))

        # warm-up of each, and the equality of what they build
        t, dmap, _ = device_route()
        (hp, hi, hf), hmap, _ = host_route()
        first = fptr[hi[hp[:-1]]] + hf[hp[:-1]]
        rank = np.empty(len(first), dtype=np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(len(first))
        tp, ti, tf, tn, _ = t.download()
        order = np.argsort(first, kind="stable")
        lens = np.diff(hp)
        assert np.array_equal(np.concatenate([[0], np.cumsum(lens[order])]), tp)
        take = np.concatenate([np.arange(hp[k], hp[k + 1]) for k in order]) if len(order) else np.zeros(0, dtype=np.int64)
        assert np.array_equal(hi[take], ti) and np.array_equal(hf[take], tf)
        a, b = dmap.arrays(), hmap.arrays()
        perm = np.argsort(rank[b["lm_track"]], kind="stable")
        assert np.array_equal(rank[b["lm_track"]][perm], a["lm_track"])
        for k in ("lm_ray", "lm_home", "lm_views", "lm_desc"):
            assert np.array_equal(b[k][perm], a[k]), k
        out = dict(shape="%d images x %d features, all %d pairs" % (n_img, n_feat, len(ia)), n_matches=m.n_matches, matcher_device_ms=m.device_ms,
                   n_tracks=t.n_tracks, n_views=t.n_views, counts=t.counts().tolist(), n_landmarks=dmap.n_landmarks, maps_equal=True, turns=turns)
        t.close(); dmap.close(); hmap.close()
        for _ in range(turns):
            t, lmap, d = device_route()
            t.close(); lmap.close()
            _, lmap, h = host_route()
            lmap.close()
            for key, v in zip(("device_wall_ms", "device_tracks_wall_ms", "device_tracks_device_ms", "device_map_wall_ms"), d):
                rows[key].append(v)
            for key, v in zip(("host_wall_ms", "host_download_ms", "host_tracks_ms", "host_map_ms"), h):
                rows[key].append(v)
    for key, v in rows.items():
        out[key] = dict(min=float(np.min(v)), median=float(np.median(v)), all=[round(float(x), 4) for x in v])
    out["device_below_host_in_every_turn"] = bool(all(d < h for d, h in zip(rows["device_wall_ms"], rows["host_wall_ms"])))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[200, 20])
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--turns", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_device_probe.json"))
    a = ap.parse_args()
    pkg = ge.load_package()
    res = [run_shape(pkg, n, a.features, a.dim, a.turns) for n in a.images]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
