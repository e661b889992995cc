"""Device time of the covariance of bundle-adjusted cameras (ptz_ba_batch_covariance) beside the device time of ONE Levenberg-
Marquardt iteration of the same batch (last solve's device time over its LM steps), in the same process: one C2 rig (200 views x
500 observations) and a batch of 64 C1 rigs (20 x 100).  One JSON line per configuration; the minimum and the median of --repeat
timed calls after one warm-up pair.  A measurement, not a test.

    python tools/probes/probe_ba_covariance.py [--repeat 5] [--timeout 600]

Every configuration runs in a child process of its own under --timeout seconds; after a child that fails or runs out of time
nothing more is started.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as ge  # noqa: E402

CONFIGS = {"c2x1": (1, 200, 500), "c1x64": (64, 20, 100)}


def child(name, repeat):
    pkg = ge.load_package()
    n, views, obs = CONFIGS[name]
    scenes = [pkg.synth.make_scene(i, views, obs) for i in range(n)]
    b = pkg.api.BaBatch(scenes)
    b.set_state()
    lm_iter, cov_ms = [], []
    for i in range(repeat + 1):
        summ = b.solve()
        steps = max(s["num_lm_steps"] for s in summ)
        ms0 = b.last_solve_ms() / max(steps, 1)
        cov, s0, st, ms1 = b.covariance()
        if i:  # the first pair warms up: code objects, the pool's blocks
            lm_iter.append(ms0); cov_ms.append(ms1)
    ok = st == pkg.api.COV_OK
    sd_f = np.concatenate([np.sqrt(c[:, 0, 0]) for c, o in zip(cov, ok) if o])
    sd_r = np.concatenate([np.sqrt(np.einsum("cii->ci", c)[1:, 1:4]).reshape(-1) for c, o in zip(cov, ok) if o])
    print(json.dumps(dict(config=name, problems=n, views=views, order=4 * views, lm_iteration_ms_min=round(min(lm_iter), 4),
                          lm_iteration_ms_median=round(float(np.median(lm_iter)), 4), covariance_ms_min=round(min(cov_ms), 4),
                          covariance_ms_median=round(float(np.median(cov_ms)), 4),
                          covariance_over_lm_iteration=round(min(cov_ms) / min(lm_iter), 2), computed=int(ok.sum()),
                          median_sigma_f_px=round(float(np.median(sd_f)), 4), median_sigma_rot_deg=round(float(np.degrees(np.median(sd_r))), 6),
                          median_sigma0_px=round(float(np.median(s0[ok])), 4))), flush=True)
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--config", nargs="+", default=list(CONFIGS))
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.repeat)
        return 0
    for name in args.config:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeat", str(args.repeat)], timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s; stopping" % (name, args.timeout), file=sys.stderr)
            return 124
        if r.returncode != 0:
            print("%s: exit status %d; stopping" % (name, r.returncode), file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
