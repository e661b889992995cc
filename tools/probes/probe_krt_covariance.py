"""Device time of the per-query covariance (ptz_krt_covariance_batch) beside the device time of the solve (ptz_krt_solve_batch)
on the same batch, in the same process: the C5 shape, 100 000 queries x 128 matches, factor types F and FDist.  One
linearisation is one of the roughly sixteen passes a solve makes over a query's matches, so the covariance must come out well
below the solve.  One JSON line per factor type; the minimum and the median of --repeat timed calls after one warm-up call.

    python tools/probes/probe_krt_covariance.py [--n_query 100000] [--repeat 5] [--timeout 300]

Every factor type runs in a child process of its own under --timeout seconds; after a child that fails or runs out of time
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


def child(ft, n_query, repeat):
    pkg = ge.load_package()
    rb = pkg.synth.make_reloc_queries(n_query, 128, seed_id=3, factor_type=ft)
    solve, cov_ms = [], []
    for i in range(repeat + 1):
        cam, _, acc, ms0 = pkg.api.krt_solve_batch(rb)
        cov, s0, st, ms1 = pkg.api.krt_covariance_batch(rb, cam, accepted=acc)
        if i:  # the first pair warms up: code objects, the pool's blocks
            solve.append(ms0); cov_ms.append(ms1)
    ok = st == pkg.api.COV_OK
    rot0 = 1
    print(json.dumps(dict(n_query=n_query, n_match=128, factor_type=ft, solve_ms_min=round(min(solve), 3),
                          solve_ms_median=round(float(np.median(solve)), 3), covariance_ms_min=round(min(cov_ms), 3),
                          covariance_ms_median=round(float(np.median(cov_ms)), 3),
                          covariance_over_solve=round(min(cov_ms) / min(solve), 4),
                          match_bytes_per_s_in_covariance=round(16.0 * n_query * 128 / (min(cov_ms) * 1e-3), 0),
                          accepted=int(acc.sum()), computed=int(ok.sum()),
                          median_sigma_f_px=round(float(np.median(np.sqrt(cov[ok, 0, 0]))), 4),
                          median_sigma_rot_deg=[round(float(np.degrees(np.median(np.sqrt(cov[ok, rot0 + k, rot0 + k])))), 6) for k in range(3)],
                          median_sigma0_px=round(float(np.median(s0[ok])), 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_query", type=int, default=100000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--factor_type", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--child", type=int, default=-1)
    args = ap.parse_args()
    if args.child >= 0:
        child(args.child, args.n_query, args.repeat)
        return 0
    for ft in args.factor_type:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(ft), "--n_query", str(args.n_query), "--repeat",
                                str(args.repeat)], timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("factor type %d: no result within %d s; stopping" % (ft, args.timeout), file=sys.stderr)
            return 124
        if r.returncode != 0:
            print("factor type %d: exit status %d; stopping" % (ft, r.returncode), file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
