"""CPU check of the landmark map's accuracy claim, no device: on the K = 4 accuracy test's data set (synth.make_scene(0, 20, 100)
rig, make_reloc_scene(n_query=24, n_feat=600, visible_share=0.5, noise_px=0.5), make_reloc_descriptors(D=128, noise=12,
n_distractors=50)), seeds 0 .. 5, F and FDist, three runs on the SAME descriptors:
  K = 1, K = 4   the numpy matcher over every (reference, query) pair, the numpy assembly (tests/reloc_assemble_util.py)
  landmarks      the numpy map build over synth_reloc.scene_tracks, the numpy matcher over the (map, query) pairs, the numpy
                 landmark assembly (tests/landmark_util.py)
each solved by the ORACLE's krt_solve_batch.  Prints a table and writes profiles/landmark_accuracy_cpu.json.  Not a test."""
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import desc_match_util as mu  # noqa: E402
import landmark_util as lu  # noqa: E402
import reloc_assemble_util as ru  # noqa: E402


def dist2(a, b):
    """desc_match_util.dist2 through float64 BLAS: every figure is an integer below 2^53, so the result is exact"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)).astype(np.int64)


def match_pairs(desc_a, ptr_a, kp_a, desc_b, ptr_b, kp_b, img_a, img_b, **opt):
    ptr, ia, ua, ub = [0], [], [], []
    for x, y in zip(img_a, img_b):
        a, b = desc_a[ptr_a[x]:ptr_a[x + 1]], desc_b[ptr_b[y]:ptr_b[y + 1]]
        t = None
        if len(a) and len(b):
            d2 = dist2(a, b)
            t = mu.top2(d2) + mu.top2(d2.T)
        i, j, _ = mu.accept(t, **opt)
        ia.append(i); ua.append(kp_a[ptr_a[x] + i]); ub.append(kp_b[ptr_b[y] + j])
        ptr.append(ptr[-1] + len(i))
    return dict(match_ptr=np.asarray(ptr, dtype=np.int64), idx_a=np.concatenate(ia).astype(np.int32),
                uv_a=np.concatenate(ua).astype(np.float32).reshape(-1, 2), uv_b=np.concatenate(ub).astype(np.float32).reshape(-1, 2))


def run(seed, ft, pkg, orc):
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt.copy()
    if ft:
        rig[:, 10] = np.random.default_rng(100).uniform(-0.05, 0.05, len(rig))
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=24, n_feat=600, visible_share=0.5, noise_px=0.5, factor_type=ft, seed=seed)
    (rp, rd, rk), (qp, qd, qk) = pkg.synth_reloc.make_reloc_descriptors(sc, D=128, noise=12, n_distractors=50, seed=seed)
    R = ru.rotations(rig)
    nq, n_ref = sc.n_query, sc.n_ref
    ia, ib = np.tile(np.arange(n_ref), nq), np.repeat(np.arange(nq), n_ref)
    m = match_pairs(rd, rp, rk, qd, qp, qk, ia, ib, min_matches=8)
    out = {}

    def solve(asm, name):
        b = types.SimpleNamespace(n_query=nq, match_ptr=asm["match_ptr"], uv_ref=asm["uv_ref"], uv_cur=asm["uv_cur"], cam_ref=asm["cam_ref"],
                                  cam_init=asm["cam_init"], factor_type=ft)
        cam, _, acc = orc.krt_solve_batch(b)[:3]
        out[name] = dict(cam=cam, acc=np.asarray(acc), n=np.diff(asm["match_ptr"]))

    for K in (1, 4):
        solve(ru.assemble(m["match_ptr"], m["uv_a"], m["uv_b"], ia.astype(np.int32), sc.query_ptr, rig, sc.query_wh, factor_type=ft, max_refs=K, ref_R=R),
              f"K{K}")
    tp, ti, tf, _ = pkg.synth_reloc.scene_tracks(sc, 50)
    lm = lu.build(rp, rd, rk, rig, tp, ti, tf, factor_type=ft, min_views=1, ref_R=R)
    lp = np.array([0, len(lm["lm_track"])], dtype=np.int64)
    ml = match_pairs(lm["lm_desc"], lp, np.zeros((len(lm["lm_track"]), 2), np.float32), qd, qp, qk, np.zeros(nq, int), np.arange(nq), min_matches=8)
    solve(lu.assemble(lm, ml["match_ptr"], ml["idx_a"], ml["uv_b"], rig, sc.query_wh, ref_R=R), "lm")
    both = (out["K1"]["acc"] == 1) & (out["K4"]["acc"] == 1) & (out["lm"]["acc"] == 1)
    col = 10 if ft else 0
    rec = dict(seed=seed, factor_type=ft, n_landmarks=int(len(lm["lm_track"])), n_ref_features=int(len(sc.ref_track)))
    for k, v in out.items():
        err = np.abs(v["cam"][both, col] - sc.cam_gt[both, col]) / (sc.cam_gt[both, col] if col == 0 else 1.0)
        ferr = np.abs(v["cam"][both, 0] - sc.cam_gt[both, 0]) / sc.cam_gt[both, 0]
        rec[k] = dict(accepted=int(v["acc"].sum()), median_err=float(np.median(err)), median_focal_err=float(np.median(ferr)),
                      median_matches=float(np.median(v["n"])))
    rec["lost_vs_K1"] = int(((out["K1"]["acc"] == 1) & (out["lm"]["acc"] == 0)).sum())
    rec["ratio_lm_K1"] = rec["lm"]["median_err"] / rec["K1"]["median_err"]
    rec["ratio_K4_K1"] = rec["K4"]["median_err"] / rec["K1"]["median_err"]
    return rec


def main():
    pkg, orc = ge.load_package(), ge.load_oracle()
    orc.build()
    recs = []
    for ft in (0, 1):
        for seed in range(6):
            r = run(seed, ft, pkg, orc)
            recs.append(r)
            print(f"ft {ft} seed {seed}: {'k1' if ft else 'focal'} err K1 {r['K1']['median_err']:.2e} K4 {r['K4']['median_err']:.2e} lm {r['lm']['median_err']:.2e}"
                  f" | lm/K1 {r['ratio_lm_K1']:.2f} K4/K1 {r['ratio_K4_K1']:.2f} | accepted {r['K1']['accepted']} {r['K4']['accepted']} {r['lm']['accepted']}"
                  f" lost {r['lost_vs_K1']} | matches {r['K1']['median_matches']:.0f} {r['K4']['median_matches']:.0f} {r['lm']['median_matches']:.0f}"
                  f" | landmarks {r['n_landmarks']} of {r['n_ref_features']} features", flush=True)
    with open(os.path.join(ROOT, "profiles", "landmark_accuracy_cpu.json"), "w") as f:
        json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
