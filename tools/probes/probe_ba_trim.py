"""Device time of the residual report (ptz_ba_batch_residuals) and of one selection (ptz_ba_batch_trim_select, which takes the
report and the rule in one pass) on one C2 rig (200 views x 500 observations) beside one LM iteration of the same batch
(last_solve_ms / num_lm_steps of a solve in the same process).  --repeat timed rounds after one warm-up round; one JSON line with
the minimum and the median of each.  A measurement, not a test.

    python tools/probes/probe_ba_trim.py [--repeat 7] [--timeout 600]

The measurement runs in a child process of its own under --timeout seconds.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as ge  # noqa: E402


def child(repeat, views, obs):
    pkg = ge.load_package()
    sc = pkg.synth.make_scene(0, views, obs)
    b = pkg.api.BaBatch([sc])
    b.set_state()
    t_rep, t_nomed, t_sel, t_sel0, t_it = [], [], [], [], []
    for i in range(repeat + 1):
        summ = b.solve()[0]
        it_ms = b.last_solve_ms() / max(1, summ["num_lm_steps"])
        rep = b.residuals()[0]
        nomed = b.residuals(median=False)[0]
        _, thr, nrej, ms_sel = b.trim_select(4.0, 3.0)
        _, _, _, ms_sel0 = b.trim_select(4.0, 0.0)
        if i:  # the first round warms up: code objects, the pool's blocks
            t_rep.append(rep["device_ms"]); t_nomed.append(nomed["device_ms"]); t_sel.append(ms_sel); t_sel0.append(ms_sel0); t_it.append(it_ms)

    def mm(t):
        return dict(min=round(1e3 * min(t), 1), median=round(1e3 * float(np.median(t)), 1))

    print(json.dumps(dict(views=views, n_obs=int(sc.n_obs), n_ray=int(sc.n_ray), lm_steps=int(summ["num_lm_steps"]),
                          lm_iteration_us=mm(t_it), report_us=mm(t_rep), report_without_median_us=mm(t_nomed), select_us=mm(t_sel),
                          select_k_sigma_0_us=mm(t_sel0), rms_px=round(rep["rms"], 4), median_px=round(rep["median"], 4),
                          threshold_px=round(float(thr[0]), 4), n_reject=int(nrej[0]))), flush=True)
    b.close()


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
