#!/usr/bin/env python3
"""Measurement of the reference shortlist in front of the resident relocalization loop (a probe, not a test; no threshold).

Online shape: 1000 queries x 2000 features against 200 references, D = 128.  In ONE process, after a warm-up of both, alternating turns:
  all pairs    api.Relocalizer.run (ptz_relocalizer_run): every (reference, query) pair through the matcher -- the yardstick;
  shortlisted  api.Relocalizer.run(..., shortlist=dict(max_refs=R, n_probes=M)) (ptz_relocalizer_run_shortlisted), M = 256, R = 8.
Reports the two wall times (median over the turns, host clock around calls that end in a stream wait), the stage times of both, the
vote pass's device time, that time as a fraction of the dense matcher's device time on all pairs, and beside it the ratio of the two
multiply-accumulate counts, M / (2 n_q).  Then the vote pass alone for ONE query (the serving case), device time between events.
The images share descriptors, not a rig's geometry: this measures time only; what a shortlist keeps is the tests' subject.

usage: probe_reloc_shortlist.py [--images 200] [--features 2000] [--queries 1000] [--dim 128] [--turns 3] [--probes 256] [--refs 8]
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


def features(rng, n_img, n_feat, D, base, base_xy, noise=12):
    """n_img images of n_feat features; half of every image's rows are noisy copies of rows of `base` at the pixels base_xy (plus a
    pixel of noise), so that there is something to accept; the rest uniform."""
    d = rng.integers(0, 256, (n_img * n_feat, D), dtype=np.uint8)
    xy = rng.uniform([0, 0], [1920, 1080], (n_img * n_feat, 2)).astype(np.float32)
    k = n_feat // 2
    for m in range(n_img):
        pick = rng.integers(0, len(base), k)
        d[m * n_feat:m * n_feat + k] = np.clip(base[pick].astype(np.int16) + rng.integers(-noise, noise + 1, (k, D)), 0, 255).astype(np.uint8)
        xy[m * n_feat:m * n_feat + k] = base_xy[pick] + rng.normal(0, 1.0, (k, 2)).astype(np.float32)
    return d, xy, (np.arange(n_img + 1) * n_feat).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--probes", type=int, default=256)
    ap.add_argument("--refs", type=int, default=8)
    a = ap.parse_args()
    pkg = ge.load_package()
    api = pkg.api
    rng = np.random.default_rng(0)
    n_ref, nq = a.images, a.queries
    rig = pkg.synth.make_scene(0, n_ref, 20).cam_gt  # only the cameras matter
    base = rng.integers(0, 256, (4 * a.features, a.dim), dtype=np.uint8)
    base_xy = rng.uniform([100, 100], [1820, 980], (len(base), 2)).astype(np.float32)
    rd, rk, rp = features(rng, n_ref, a.features, a.dim, base, base_xy)
    qd, qk, qp = features(rng, nq, a.features, a.dim, base, base_xy)
    wh = np.tile(np.array([1920, 1080], dtype=np.int32), (nq, 1))
    sl = dict(max_refs=a.refs, n_probes=a.probes)
    m = min(a.probes, a.features)
    out = dict(shape="online: %d queries x %d features against %d references" % (nq, a.features, n_ref), D=a.dim, M=a.probes, R=a.refs,
               mac_ratio_vote_pass=m / (2.0 * a.features), mac_ratio_shortlisted_pairs=min(a.refs, n_ref) / float(n_ref))
    with api.DescSet(rp, rd, rk) as refs, api.DescSet(qp, qd, qk) as tests, api.Relocalizer(refs, rig) as rl:
        run_all = lambda: rl.run(tests, wh, max_refs=1, match=dict(min_matches=8))
        run_sl = lambda: rl.run(tests, wh, max_refs=1, match=dict(min_matches=8), shortlist=sl)
        run_all(); run_sl()  # warm-up of every shape of the timed window
        t_all, t_sl, s_all, s_sl, v_ms = [], [], [], [], []
        for _ in range(a.turns):
            t0 = time.perf_counter()
            ga = run_all()
            t1 = time.perf_counter()
            gs = run_sl()
            t2 = time.perf_counter()
            t_all.append(t1 - t0); t_sl.append(t2 - t1)
            s_all.append(ga["stage_ms"]); s_sl.append(gs["stage_ms"]); v_ms.append(gs["shortlist_ms"])
        s_all, s_sl = np.median(np.array(s_all), axis=0), np.median(np.array(s_sl), axis=0)
        vote = float(np.median(v_ms))
        out.update(all_pairs_wall_ms=1e3 * float(np.median(t_all)), shortlisted_wall_ms=1e3 * float(np.median(t_sl)),
                   all_pairs_wall_ms_turns=[1e3 * x for x in t_all], shortlisted_wall_ms_turns=[1e3 * x for x in t_sl],
                   all_pairs_stage_ms=[float(x) for x in s_all], shortlisted_stage_ms=[float(x) for x in s_sl], vote_pass_device_ms=vote,
                   vote_pass_over_dense_matcher=vote / float(s_all[0]), shortlisted_matcher_over_dense_matcher=float(s_sl[0] / s_all[0]),
                   pairs_all=int(nq * n_ref), pairs_shortlisted=int(gs["n_short"].sum()),
                   anchors_kept=int((ga["sel_ref"][:, 0] == gs["sel_ref"][:, 0]).sum()), accepted_all=int(ga["accepted"].sum()),
                   accepted_shortlisted=int(gs["accepted"].sum()), turns=a.turns)
        # the serving case: one query, the references split into groups
        one = []
        for r in range(a.turns + 2):
            got = api.desc_shortlist(refs, tests, query_img=np.array([r % nq], dtype=np.int32), **sl)
            if r >= 2:
                one.append(got["device_ms"])
        out["vote_pass_one_query_device_ms"] = float(np.median(one))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
