"""Device time of the RANSAC inlier gate and of the LM behind it (ptz_krt_solve_batch_gated) for C5-shaped relocalization
batches (128 matches per query) at 0 / 30 / 50 % injected outlier matches, beside the ungated ptz_krt_solve_batch on the same
arrays.  One JSON line per (queries, outlier fraction).

    python tools/probes/probe_match_gate.py [--n_query 10000] [--factor_type 0] [--repeat 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_query", type=int, nargs="+", default=[10000])
    ap.add_argument("--factor_type", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    pkg = ge.load_package()
    for n in args.n_query:
        base = pkg.synth.make_reloc_batch(n, 128, seed_id=7, factor_type=args.factor_type)
        clean = np.array(base.uv_cur, dtype=np.float32)
        for frac in (0.0, 0.3, 0.5):
            rng = np.random.default_rng(11)
            k = rng.random(len(clean)) < frac
            base.uv_cur = clean.copy()
            base.uv_cur[k] = rng.uniform([0, 0], [1920, 1080], (int(k.sum()), 2))
            plain, gate, lm = [], [], []
            for _ in range(args.repeat):
                _, _, acc0, ms0 = pkg.api.krt_solve_batch(base)
                cam, _, acc, ninl, mask, _, ms = pkg.api.krt_solve_batch_gated(base)
                plain.append(ms0); gate.append(ms[0]); lm.append(ms[1])
            ferr = np.abs(cam[:, 0] - base.cam_gt[:, 0])[acc.astype(bool) & (ninl > 0)]
            print(json.dumps(dict(n_query=n, factor_type=args.factor_type, outliers=frac, ungated_lm_ms=round(min(plain), 3),
                                  ungated_accepted=int(acc0.sum()), gate_ms=round(min(gate), 3), gated_lm_ms=round(min(lm), 3),
                                  gated_accepted=int((acc.astype(bool) & (ninl > 0)).sum()), inliers_min=int(ninl.min()),
                                  outliers_kept=int(mask[k].sum()), matches_kept=int(ninl.sum()), matches=len(k),
                                  median_abs_focal_error_px=round(float(np.median(ferr)), 3) if len(ferr) else None)), flush=True)


if __name__ == "__main__":
    main()
