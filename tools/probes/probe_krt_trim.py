"""Device time of the residual report (ptz_krt_residuals_batch) and of the trimmed solve (ptz_krt_solve_batch_trimmed) beside the
device time of the plain solve (ptz_krt_solve_batch) on the same batch, in the same process: the C5 shape, 100 000 queries x 128
matches, clean and with 30 % of every query's matches replaced by uniform pixels.  What to hold the clean figure against: one
solve, plus one report, plus the early returns of the rounds in which no query is active any more.  One JSON line per (factor
type, contamination); the three calls ALTERNATE after one warm-up turn, the minimum and the median of --repeat turns are given.

    python tools/probes/probe_krt_trim.py [--n_query 100000] [--repeat 5] [--timeout 300]

Every case runs in a child process of its own under --timeout seconds; after a child that fails or runs out of time nothing more
is started.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as ge  # noqa: E402


def child(ft, frac, n_query, repeat):
    pkg = ge.load_package()
    rb = pkg.synth.make_reloc_queries(n_query, 128, seed_id=3, factor_type=ft)
    wrong = np.zeros(len(rb.uv_cur), dtype=bool)
    if frac > 0:
        rng = np.random.default_rng(5)
        rb.uv_cur = np.array(rb.uv_cur, dtype=np.float32)
        wrong = rng.random(len(rb.uv_cur)) < frac
        rb.uv_cur[wrong] = rng.uniform([0, 0], [1920, 1080], (int(wrong.sum()), 2)).astype(np.float32)
    solve, report, trimmed = [], [], []
    for i in range(repeat + 1):
        cam, _, acc, ms0 = pkg.api.krt_solve_batch(rb)
        r = pkg.api.krt_residuals_batch(rb, cam, accepted=acc)
        tcam, _, tacc, kept, rep, ms2 = pkg.api.krt_solve_batch_trimmed(rb)
        if i:  # the first turn warms up: code objects, the pool's blocks
            solve.append(ms0); report.append(r["device_ms"]); trimmed.append(ms2)
    rounds = np.array([x["rounds"] for x in rep])
    k = kept.astype(bool)
    ferr = np.abs(tcam[:, 0] - rb.cam_gt[:, 0])[tacc != 0]
    print(json.dumps(dict(n_query=n_query, n_match=128, factor_type=ft, contaminated=frac, solve_ms_min=round(min(solve), 3),
                          solve_ms_median=round(float(np.median(solve)), 3), report_ms_min=round(min(report), 3),
                          report_ms_median=round(float(np.median(report)), 3), trimmed_ms_min=round(min(trimmed), 3),
                          trimmed_ms_median=round(float(np.median(trimmed)), 3), report_over_solve=round(min(report) / min(solve), 4),
                          trimmed_over_solve=round(min(trimmed) / min(solve), 4), accepted_plain=int(acc.sum()), accepted_trimmed=int(tacc.sum()),
                          rounds_mean=round(float(rounds.mean()), 3), rounds_max=int(rounds.max()),
                          flagged=int(sum(1 for x in rep if x["flags"])), wrong_kept=int((k & wrong).sum()), good_removed=int((~k & ~wrong).sum()),
                          median_focal_error_px=round(float(np.median(ferr)), 4) if len(ferr) else None)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_query", type=int, default=100000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--factor_type", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--contaminated", type=float, nargs="+", default=[0.0, 0.3])
    ap.add_argument("--child", type=int, default=-1)
    ap.add_argument("--child_frac", type=float, default=0.0)
    args = ap.parse_args()
    if args.child >= 0:
        child(args.child, args.child_frac, args.n_query, args.repeat)
        return 0
    for ft in args.factor_type:
        for frac in args.contaminated:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(ft), "--child_frac", str(frac), "--n_query",
                                    str(args.n_query), "--repeat", str(args.repeat)], timeout=args.timeout)
            except subprocess.TimeoutExpired:
                print("factor type %d, %g contaminated: no result within %d s; stopping" % (ft, frac, args.timeout), file=sys.stderr)
                return 124
            if r.returncode != 0:
                print("factor type %d, %g contaminated: exit status %d; stopping" % (ft, frac, r.returncode), file=sys.stderr)
                return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
