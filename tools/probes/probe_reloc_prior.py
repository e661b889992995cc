#!/usr/bin/env python3
"""Measurement of relocalization from prior cameras against the vote-shortlisted run (a probe, not a test; no threshold).

Online shape: 1000 queries x 2000 features against 200 references, D = 128, R = 8 references per query.  In ONE process, after a
warm-up of both, alternating turns:
  shortlisted  api.Relocalizer.run(..., shortlist=dict(max_refs=R, n_probes=256)) (ptz_relocalizer_run_shortlisted) -- the yardstick;
  tracked      api.Relocalizer.run(..., prior=dict(cams=..., radius_px=40, max_refs=R)) (ptz_relocalizer_run_tracked); the prior of
               query q is the camera of reference q mod n_ref turned by 0.3 degrees, its focal 2 % off.
Reports the two wall times (median and minimum over the turns, host clock around calls that end in a stream wait), the stage times of
both and the device time of the tracked run's stage 0.  The images share descriptors, not a rig's geometry (the tracked run's pairs are
real overlaps of the CAMERAS, their features are not): this measures time only; what a prior finds is the tests' subject.

usage: probe_reloc_prior.py [--images 200] [--features 2000] [--queries 1000] [--dim 128] [--turns 3] [--refs 8] [--radius 40]
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
from probe_reloc_shortlist import features  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--refs", type=int, default=8)
    ap.add_argument("--radius", type=float, default=40.0)
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
    priors = pkg.synth_reloc.perturb_cameras(rig[np.arange(nq) % n_ref], 0.3, 0.02, seed=0)
    sl = dict(max_refs=a.refs, n_probes=256)
    pr = dict(cams=priors, radius_px=a.radius, max_refs=a.refs)
    out = dict(shape="online: %d queries x %d features against %d references" % (nq, a.features, n_ref), D=a.dim, R=a.refs, radius_px=a.radius)
    with api.DescSet(rp, rd, rk) as refs, api.DescSet(qp, qd, qk) as tests, api.Relocalizer(refs, rig) as rl:
        run_sl = lambda: rl.run(tests, wh, max_refs=1, match=dict(min_matches=8), shortlist=sl)
        run_tr = lambda: rl.run(tests, wh, max_refs=1, match=dict(min_matches=8), prior=pr)
        run_sl(); run_tr()  # warm-up of every shape of the timed window
        t_sl, t_tr, s_sl, s_tr, p_ms = [], [], [], [], []
        for _ in range(a.turns):
            t0 = time.perf_counter()
            gs = run_sl()
            t1 = time.perf_counter()
            gt = run_tr()
            t2 = time.perf_counter()
            t_sl.append(1e3 * (t1 - t0)); t_tr.append(1e3 * (t2 - t1))
            s_sl.append(gs["stage_ms"]); s_tr.append(gt["stage_ms"]); p_ms.append(gt["prior_ms"])
        med = lambda v: [float(x) for x in np.median(np.array(v), axis=0)]
        low = lambda v: [float(x) for x in np.min(np.array(v), axis=0)]
        out.update(shortlisted_wall_ms=float(np.median(t_sl)), tracked_wall_ms=float(np.median(t_tr)), shortlisted_wall_ms_min=min(t_sl),
                   tracked_wall_ms_min=min(t_tr), shortlisted_wall_ms_turns=t_sl, tracked_wall_ms_turns=t_tr,
                   shortlisted_stage_ms=med(s_sl), tracked_stage_ms=med(s_tr), shortlisted_stage_ms_min=low(s_sl), tracked_stage_ms_min=low(s_tr),
                   shortlist_ms=float(gs["shortlist_ms"]), prior_ms=float(np.median(p_ms)), prior_ms_min=float(min(p_ms)),
                   pairs_shortlisted=int(gs["n_short"].sum()), pairs_tracked=int(gt["n_short"].sum()),
                   guided_matches_tracked=int(gt["n_matches"].sum()), accepted_shortlisted=int(gs["accepted"].sum()),
                   accepted_tracked=int(gt["accepted"].sum()), tracked_over_shortlisted=float(np.median(t_tr) / np.median(t_sl)), turns=a.turns)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
