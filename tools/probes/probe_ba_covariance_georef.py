"""Device time of the covariance of georeferenced cameras (ptz_ba_batch_covariance_georef) on one C2-sized rig (200 views x 500
observations, annotations on 6 views) beside ptz_ba_batch_covariance on the same rig without annotations, in the same process.
Both calls alternate, --repeat timed pairs after one warm-up pair; one JSON line with the minimum and the median of each and
their ratio.  The cubic stage grows by ((NC n_cam + 6) / (NF n_cam))^3, about 2.0 for PTZRay.  A measurement, not a test.

    python tools/probes/probe_ba_covariance_georef.py [--repeat 7] [--timeout 600]

The measurement runs in a child process of its own under --timeout seconds.
"""
import argparse
import copy
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as ge  # noqa: E402


def child(repeat, views, obs):
    pkg = ge.load_package()
    plain = pkg.synth.make_scene(0, views, obs)
    ann = pkg.synth.add_annotations(copy.copy(plain), n_annotated=6)
    n_ann = len(ann.obs3d["cam"])
    assert n_ann > 0, "the generator found no annotation on this rig"
    a = pkg.api.BaBatch([plain]); a.set_state(); a.solve()
    g = pkg.api.BaBatch([ann]); g.set_state(); g.solve()
    t2, tg = [], []
    for i in range(repeat + 1):
        _, _, st2, ms2 = a.covariance()
        cov, cen, s0, stg, msg = g.covariance_georef()
        if i:  # the first pair warms up: code objects, the pool's blocks
            t2.append(ms2); tg.append(msg)
    assert st2[0] == pkg.api.COV_OK and stg[0] == pkg.api.COV_OK, (st2, stg)
    nf, nc = 4, 5
    print(json.dumps(dict(views=views, annotations=n_ann, annotated_views=len(set(ann.obs3d["cam"])), order_2d2d=nf * views,
                          order_georef=nc * views + 6, cubic_growth=round(((nc * views + 6) / (nf * views)) ** 3, 3),
                          covariance_ms_min=round(min(t2), 4), covariance_ms_median=round(float(np.median(t2)), 4),
                          covariance_georef_ms_min=round(min(tg), 4), covariance_georef_ms_median=round(float(np.median(tg)), 4),
                          ratio_of_minima=round(min(tg) / min(t2), 3), ratio_of_medians=round(float(np.median(tg) / np.median(t2)), 3),
                          sigma0_features_px=round(float(s0[0, 0]), 4), sigma0_annotations_px=round(float(s0[0, 1]), 4),
                          sigma_centre_m=[round(float(v), 5) for v in np.sqrt(np.diag(cen[0]))],
                          median_sigma_f_px=round(float(np.median(np.sqrt(cov[0][:, 0, 0]))), 4))), flush=True)
    a.close(); g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--obs", type=int, default=500)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.repeat, args.views, args.obs)
        return 0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeat", str(args.repeat), "--views", str(args.views),
                            "--obs", str(args.obs)], timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print("no result within %d s" % args.timeout, file=sys.stderr)
        return 124
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
