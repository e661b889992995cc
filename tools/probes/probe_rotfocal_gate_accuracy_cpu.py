"""CPU check of the tracked landmark run's accuracy under the rotation-and-focal gate, no device: probe_landmark_prior_accuracy_cpu.py
with the numpy restatement of ptz_rotfocal.h (tests/rotfocal_util.py, 4 px, 128 iterations) in the place of the homography harness
as the gate on the assembled query -- same data set, same seeds 0 .. 5, F and FDist, same three runs (dense, prior, prior + gate with
min_inliers 6 and 30), each solved by the ORACLE's krt_solve_batch.  Prints a table and writes profiles/rotfocal_gate_accuracy_cpu.json.
Not a test."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import probe_landmark_prior_accuracy_cpu as base  # noqa: E402
import rotfocal_util as rf  # noqa: E402  (tests/ is on the path once base is imported)


def gate(_harness, asm, min_inliers):
    """the gate on the assembled query: (compacted CSR, inliers per query)"""
    ptr, keep = [0], []
    for q in range(len(asm["match_ptr"]) - 1):
        s = slice(int(asm["match_ptr"][q]), int(asm["match_ptr"][q + 1]))
        r = rf.find(asm["uv_ref"][s], asm["uv_cur"][s], asm["cam_ref"][q], asm["cam_init"][q, 2], asm["cam_init"][q, 3], 4.0, 128)
        m = r["mask"].astype(bool) if r["found"] else np.zeros(s.stop - s.start, dtype=bool)
        if m.sum() < max(min_inliers, 4):
            m[:] = False
        keep.append(m)
        ptr.append(ptr[-1] + int(m.sum()))
    keep = np.concatenate(keep) if keep else np.zeros(0, dtype=bool)
    return dict(asm, match_ptr=np.asarray(ptr, dtype=np.int64), uv_ref=asm["uv_ref"][keep], uv_cur=asm["uv_cur"][keep]), np.diff(ptr)


base.gate = gate


def main():
    pkg, orc = base.ge.load_package(), base.ge.load_oracle()
    orc.build()
    recs = []
    for ft in (0, 1):
        for seed in range(6):
            r = base.run(seed, ft, pkg, orc, None)
            recs.append(r)
            key = "median_k1_err" if ft else "median_focal_err"
            print(f"ft {ft} seed {seed}: {'k1' if ft else 'focal'} err dense {r['dense'][key]:.3e} prior {r['prior'][key]:.3e} prior+gate {r['prior_gate6'][key]:.3e}"
                  f" | gate/dense {r['ratio_gate_dense']:.2f} | focal {r['dense']['median_focal_err']:.3e} {r['prior_gate6']['median_focal_err']:.3e}"
                  f" | accepted {r['dense']['accepted']} {r['prior']['accepted']} {r['prior_gate6']['accepted']} {r['prior_gate30']['accepted']} lost {r['lost_vs_dense']}"
                  f" | matches {r['dense']['median_matches']:.0f} {r['prior']['median_matches']:.0f} {r['prior_gate6']['median_matches']:.0f}"
                  f" | gate30 = gate6: {r['gate30_equals_gate6']}", flush=True)
    for r in recs:  # (the lists of accepted queries are 0 .. 23 in every row: the counts say it)
        for v in r.values():
            if isinstance(v, dict):
                v.pop("accepted_queries", None)
    with open(os.path.join(base.ROOT, "profiles", "rotfocal_gate_accuracy_cpu.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in recs) + "\n]\n")


if __name__ == "__main__":
    main()
