"""CPU check of the tracked landmark run's accuracy claim, no device: on the data set of tests/test_gpu_relocalizer_prior.py
(synth.make_scene(0, 20, 100) rig, make_reloc_scene(n_query=24, n_feat=600, visible_share=0.5, noise_px=0.5),
make_reloc_descriptors(D=128, noise=12, n_distractors=50, repeat_share=0.7, repeat_group=4, repeat_noise=6),
synth_reloc.scene_tracks(sc, 50)), scene, descriptor and perturbation seed equal, seeds 0 .. 5, F and FDist, three runs on the SAME
descriptors against the SAME numpy map (tests/landmark_util.py):
  dense          the numpy matcher over the (map, query) pairs, the numpy landmark assembly -- ptz_relocalizer_run_landmarks
  prior          priors perturb_cameras(cam_gt, 0.3 degrees, 2 %): the restated view (tests/landmark_prior_util.py, radius 40 px),
                 the restated guided matcher under identity H on it, the lift, the landmark assembly, the prior camera rule
  prior + gate   the same with the homography_harness RANSAC (4 px) as the gate on the assembled query, min_inliers 6 and 30
each solved by the ORACLE's krt_solve_batch; a gated query the gate kept nothing of is not accepted.  A fourth row runs priors 30
degrees off (F, seed 0).  Prints a table and writes profiles/landmark_prior_accuracy_cpu.json.  Not a test."""
import ctypes as C
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import desc_guided_util as gu  # noqa: E402
import desc_match_util as mu  # noqa: E402
import homography_corpus as hc  # noqa: E402
import landmark_prior_util as lpu  # noqa: E402
import landmark_util as lu  # noqa: E402
import reloc_assemble_util as ru  # noqa: E402
import reloc_prior_util as pu  # noqa: E402

RADIUS = 40.0
I9 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.float64)


def dist2(a, b):
    """desc_match_util.dist2 through float64 BLAS: every figure is an integer below 2^53, so the result is exact"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)).astype(np.int64)


mu.dist2 = dist2  # (the guided restatement calls it through its module)


def match_dense(lm_desc, qd, qp, qk, nq, **opt):
    ptr, ia, ub = [0], [], []
    for q in range(nq):
        b = qd[qp[q]:qp[q + 1]]
        d2 = dist2(lm_desc, b)
        i, j, _ = mu.accept(mu.top2(d2) + mu.top2(d2.T), **opt)
        ia.append(i); ub.append(qk[qp[q] + j])
        ptr.append(ptr[-1] + len(i))
    return dict(match_ptr=np.asarray(ptr, dtype=np.int64), idx_a=np.concatenate(ia).astype(np.int32),
                uv_b=np.concatenate(ub).astype(np.float32).reshape(-1, 2))


def gate(harness, asm, min_inliers):
    """the gate on the assembled query: (compacted CSR, inliers per query)"""
    _, found, mask = hc.run_per_pair(harness.h_find_homography, asm["match_ptr"], asm["uv_ref"], asm["uv_cur"], 4.0)
    ptr, keep = [0], []
    for q in range(len(found)):
        m = mask[int(asm["match_ptr"][q]):int(asm["match_ptr"][q + 1])].astype(bool)
        if not (found[q] == 1 and m.sum() >= max(min_inliers, 4)):
            m[:] = False
        keep.append(m)
        ptr.append(ptr[-1] + int(m.sum()))
    keep = np.concatenate(keep) if keep else np.zeros(0, dtype=bool)
    return dict(asm, match_ptr=np.asarray(ptr, dtype=np.int64), uv_ref=asm["uv_ref"][keep], uv_cur=asm["uv_cur"][keep]), np.diff(ptr)


def prior_assembly(lm, view, qd, qp, qk, rig, R, wh, priors, ft, nq):
    g = gu.match_pairs_guided(lm["lm_desc"][view["vis_lm"]], view["vis_ptr"], view["vis_uv"], qd, qp, qk, np.arange(nq), np.arange(nq),
                              np.tile(I9, (nq, 1)), None, RADIUS, min_matches=8)
    pair_of = np.repeat(np.arange(nq), np.diff(g["match_ptr"]))
    lifted = view["vis_lm"][view["vis_ptr"][pair_of] + g["idx_a"]].astype(np.int32)
    asm = lu.assemble(lm, g["match_ptr"], lifted, g["uv_b"], rig, wh, ref_R=R)
    asm["cam_init"] = pu.prior_camera(asm["cam_init"], priors, ft)
    return asm


def run(seed, ft, pkg, orc, harness, angle=0.3, only_prior=False):
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt.copy()
    if ft:
        rig[:, 10] = np.random.default_rng(100).uniform(-0.05, 0.05, len(rig))
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=24, n_feat=600, visible_share=0.5, noise_px=0.5, factor_type=ft, seed=seed)
    (rp, rd, rk), (qp, qd, qk) = pkg.synth_reloc.make_reloc_descriptors(sc, D=128, noise=12, n_distractors=50, seed=seed, repeat_share=0.7,
                                                                        repeat_group=4, repeat_noise=6)
    R = ru.rotations(rig)
    nq = sc.n_query
    tp, ti, tf, _ = pkg.synth_reloc.scene_tracks(sc, 50)
    lm = lu.build(rp, rd, rk, rig, tp, ti, tf, factor_type=ft, min_views=1, ref_R=R)
    priors = pkg.synth_reloc.perturb_cameras(sc.cam_gt, angle, 0.02, seed=seed)
    view = lpu.visible(lm["lm_ray"], priors, sc.query_wh, ft, RADIUS)
    out = {}

    def solve(asm, name, ninl=None):
        b = types.SimpleNamespace(n_query=nq, match_ptr=asm["match_ptr"], uv_ref=asm["uv_ref"], uv_cur=asm["uv_cur"], cam_ref=asm["cam_ref"],
                                  cam_init=asm["cam_init"], factor_type=ft)
        cam, _, acc = orc.krt_solve_batch(b)[:3]
        acc = np.asarray(acc) * (1 if ninl is None else (ninl > 0))
        out[name] = dict(cam=cam, acc=acc, n=np.diff(asm["match_ptr"]))

    if not only_prior:
        md = match_dense(lm["lm_desc"], qd, qp, qk, nq, min_matches=8)
        solve(lu.assemble(lm, md["match_ptr"], md["idx_a"], md["uv_b"], rig, sc.query_wh, ref_R=R), "dense")
    asm = prior_assembly(lm, view, qd, qp, qk, rig, R, sc.query_wh, priors, ft, nq)
    if not only_prior:
        solve(asm, "prior")
    for mi in (6, 30):
        g, ninl = gate(harness, asm, mi)
        solve(g, f"prior_gate{mi}", ninl)
    nv = np.diff(view["vis_ptr"])
    rec = dict(seed=seed, factor_type=ft, angle_deg=angle, n_landmarks=int(len(lm["lm_track"])), n_visible_median=float(np.median(nv)),
               n_visible_max=int(nv.max()))
    both = np.ones(nq, dtype=bool)
    for v in out.values():
        both &= v["acc"] == 1
    for k, v in out.items():
        rec[k] = dict(accepted=int(v["acc"].sum()), accepted_queries=np.nonzero(v["acc"])[0].tolist(), median_matches=float(np.median(v["n"])))
        if both.any():
            rec[k]["median_focal_err"] = float(np.median(np.abs(v["cam"][both, 0] - sc.cam_gt[both, 0]) / sc.cam_gt[both, 0]))
            rec[k]["median_k1_err"] = float(np.median(np.abs(v["cam"][both, 10] - sc.cam_gt[both, 10])))
    if not only_prior:
        key = "median_k1_err" if ft else "median_focal_err"
        rec["lost_vs_dense"] = int(((out["dense"]["acc"] == 1) & (out["prior_gate6"]["acc"] == 0)).sum())
        rec["ratio_gate_dense"] = rec["prior_gate6"][key] / rec["dense"][key]
        rec["ratio_nogate_dense"] = rec["prior"][key] / rec["dense"][key]
        rec["gate30_equals_gate6"] = bool(np.array_equal(out["prior_gate6"]["cam"], out["prior_gate30"]["cam"]))
    return rec


def main():
    pkg, orc = ge.load_package(), ge.load_oracle()
    orc.build()
    harness = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "libhomography_harness.so"))
    recs = []
    for ft in (0, 1):
        for seed in range(6):
            r = run(seed, ft, pkg, orc, harness)
            recs.append(r)
            key = "median_k1_err" if ft else "median_focal_err"
            print(f"ft {ft} seed {seed}: {'k1' if ft else 'focal'} err dense {r['dense'][key]:.2e} prior {r['prior'][key]:.2e} prior+gate {r['prior_gate6'][key]:.2e}"
                  f" | gate/dense {r['ratio_gate_dense']:.2f} nogate/dense {r['ratio_nogate_dense']:.2f} | focal {r['dense']['median_focal_err']:.2e}"
                  f" {r['prior']['median_focal_err']:.2e} {r['prior_gate6']['median_focal_err']:.2e}"
                  f" | accepted {r['dense']['accepted']} {r['prior']['accepted']} {r['prior_gate6']['accepted']} {r['prior_gate30']['accepted']} lost {r['lost_vs_dense']}"
                  f" | matches {r['dense']['median_matches']:.0f} {r['prior']['median_matches']:.0f} {r['prior_gate6']['median_matches']:.0f}"
                  f" | gate30 = gate6: {r['gate30_equals_gate6']} | {r['n_landmarks']} landmarks, visible median {r['n_visible_median']:.0f} max {r['n_visible_max']}",
                  flush=True)
    far = run(0, 0, pkg, orc, harness, angle=30.0, only_prior=True)
    recs.append(far)
    print(f"priors 30 degrees off (F, seed 0): accepted min_inliers 6: {far['prior_gate6']['accepted']} {far['prior_gate6']['accepted_queries']},"
          f" min_inliers 30: {far['prior_gate30']['accepted']}; visible median {far['n_visible_median']:.0f}", flush=True)
    with open(os.path.join(ROOT, "profiles", "landmark_prior_accuracy_cpu.json"), "w") as f:
        json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
