"""GPU tests of run_ptz_reloc --gate_model rotfocal [--gate_iters T] and of KRTOptimizer::SetGateModel: on the small tool data set of
test_gpu_run_ptz_reloc_landmarks_prior.py the run with the flag registers every image the default run registers, its records carry
gate_model and gate_f and are the bits of api.Relocalizer.run(gate_model=1) on the same files; the flag's errors; without the flag the
tool writes the committed golden's bytes; the host class behind the gate equals the composition of the public calls by hand."""
import ctypes as C
import hashlib
import json
import os
import types

import numpy as np
import pytest

import desc_match_util as du
import host_util
import test_gpu_run_ptz_reloc_landmarks_prior as base

pytestmark = pytest.mark.gpu

GOLDEN = base.GOLDEN
LM = dict(max_num_iterations=200)


def test_landmark_prior_run_with_the_rotfocal_gate(pkg, tmp_path):
    """Eight queries, six with a prior in the file (one tracked landmark run), two without (the dense landmark run, gated because the
    flags imply --inlier_matches)."""
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=8, n_feat=200, visible_share=0.7, seed=3)
    refs, tests = pkg.synth_reloc.make_reloc_descriptors(sc, D=64, noise=8, n_distractors=20, seed=1, repeat_share=0.7)
    paths, names, args = base._rig_on_disk(pkg, str(tmp_path), sc, refs, tests)
    pri = pkg.synth_reloc.perturb_cameras(sc.cam_gt, 0.3, 0.02, seed=2)
    pri[:, 2], pri[:, 3] = 960.0, 540.0
    with_prior, rest = [0, 1, 3, 4, 6, 7], [2, 5]
    entries = {os.path.splitext(names[q])[0]: pkg.dataset_io.camera_json_entry(os.path.splitext(names[q])[0], pri[q], 1920, 1080) for q in with_prior}
    prior_path = str(tmp_path / "priors.json")
    json.dump({"cameras": entries}, open(prior_path, "w"), indent=4)
    out0, out1, out2 = str(tmp_path / "default"), str(tmp_path / "rotfocal"), str(tmp_path / "rotfocal300")
    common = [*args, "--landmarks", "--landmark_prior_params", prior_path]
    r0 = base._run_tool(*common, "--output", out0)
    r1 = base._run_tool(*common, "--gate_model", "rotfocal", "--output", out1)
    r2 = base._run_tool(*common, "--gate_model", "rotfocal", "--gate_iters", "300", "--output", out2)
    assert r0.returncode == 0 and r1.returncode == 0 and r2.returncode == 0, r1.stderr[-1500:]
    default, got, got300 = base._cameras(out0), base._cameras(out1), base._cameras(out2)
    assert len(default) == 8 and set(got) >= set(default) and set(got300) >= set(default)  # every image the default run registers
    assert all("gate_model" not in rec and "gate_f" not in rec for rec in default.values())
    # the homography value of the flag is the run without it
    out3 = str(tmp_path / "homography")
    assert base._run_tool(*common, "--gate_model", "homography", "--output", out3).returncode == 0
    assert open(os.path.join(out3, "tests.json"), "rb").read() == open(os.path.join(out0, "tests.json"), "rb").read()
    # the records are the Python runs' on the same files and the same map
    (rp, rd, rk), (qp, qd, qk) = refs, tests
    api = pkg.api

    def subset(qs):
        ptr = np.concatenate([[0], np.cumsum([qp[q + 1] - qp[q] for q in qs])]).astype(np.int64)
        rows = np.concatenate([np.arange(qp[q], qp[q + 1]) for q in qs])
        return api.DescSet(ptr, qd[rows], qk[rows])

    ref_entries = json.load(open(paths["ref_params"]))["cameras"]
    ref_in = np.stack([base._as_the_tool_reads(ref_entries[os.path.splitext(n)[0]]) for n in paths["ref_names"]])
    cams_in = np.stack([base._as_the_tool_reads(json.load(open(prior_path))["cameras"][os.path.splitext(names[q])[0]]) for q in with_prior])
    kw = dict(inlier_matches=True, match=dict(min_matches=8), gate_model=1, **LM)
    with api.DescSet(rp, rd, rk) as R, api.Relocalizer(R, ref_in) as rl, base._tool_map(api, R, ref_in, sc.n_ref) as lmap:
        with subset(with_prior) as T:
            trk = rl.run(T, sc.query_wh[with_prior], landmarks=lmap, landmark_prior=dict(cams=cams_in, radius_px=40.0), **kw)
            trk_f = rl.gate_models()["model"][:, 0]
            trk300 = rl.run(T, sc.query_wh[with_prior], landmarks=lmap, landmark_prior=dict(cams=cams_in, radius_px=40.0), gate_iters=300, **kw)
        with subset(rest) as T:
            den = rl.run(T, sc.query_wh[rest], landmarks=lmap, **kw)
            den_f = rl.gate_models()["model"][:, 0]
    assert trk["accepted"].all() and den["accepted"].all()
    for res, fs, qs, flag in ((trk, trk_f, with_prior, 1), (den, den_f, rest, 0)):
        for k, q in enumerate(qs):
            rec = got[os.path.splitext(names[q])[0]]
            assert rec["gate_model"] == "rotfocal" and rec["gate_f"] == fs[k] and rec["tracked"] == flag, (q, rec)
            assert rec["K"][0] == res["cam"][k, 0] and rec["n_matches"] == res["n_matches"][k]
            # the solve's focal within 5e-3 of the truth as in the default run's test; the gate's minimal model within the 1e-2 of its contract
            assert abs(rec["K"][0] / sc.cam_gt[q, 0] - 1) < 5e-3 and abs(rec["gate_f"] / sc.cam_gt[q, 0] - 1) < 1e-2
    for k, q in enumerate(with_prior):
        assert got300[os.path.splitext(names[q])[0]]["K"][0] == trk300["cam"][k, 0]


def test_flag_errors_and_the_old_bytes(pkg, tmp_path):
    rb, _, _, paths = du.chain_reloc(pkg, str(tmp_path))
    files = ["--ref_images", paths["ref_images"], "--ref_features", paths["ref_features"], "--ref_params", paths["ref_params"],
             "--test_images", paths["test_images"], "--test_features", paths["test_features"]]
    args = files + ["--match_descriptors"]
    out = str(tmp_path / "err")
    for bad, word in ((["--gate_model", "rotfocal"], "--inlier_matches"), (["--gate_model", "affine", "--inlier_matches"], "--gate_model"),
                      (["--gate_iters", "64", "--inlier_matches"], "--gate_iters"),
                      (["--gate_model", "rotfocal", "--inlier_matches", "--gate_iters", "0"], "--gate_iters"),
                      (["--gate_model", "rotfocal", "--inlier_matches", "--gate_iters", "5000"], "--gate_iters"),
                      (["--gate_model", "homography", "--inlier_matches", "--gate_iters", "64"], "--gate_iters")):
        r = base._run_tool(*args, *bad, "--output", out)
        assert r.returncode == 1 and word in r.stderr, (bad, r.returncode, r.stderr[-300:])
    r = base._run_tool(*files, "--gate_model", "rotfocal", "--inlier_matches", "--output", out)  # the flag implies --on_device
    assert r.returncode == 1 and "--match_descriptors" in r.stderr
    assert not os.path.exists(os.path.join(out, "tests.json"))
    # the image run with the flag: every record carries the keys
    out_r = str(tmp_path / "rotfocal")
    assert base._run_tool(*args, "--inlier_matches", "--gate_model", "rotfocal", "--output", out_r).returncode == 0
    g = base._cameras(out_r)
    print("image run under the rotation-and-focal gate:", len(g), "registered")
    assert all(rec["gate_model"] == "rotfocal" and rec["gate_f"] > 0 for rec in g.values())
    # without the flag: the match-file run and the on-device run write what they wrote
    out_f, out_d = str(tmp_path / "file"), str(tmp_path / "device")
    assert base._run_tool(*files, "--output", out_f).returncode == 0
    assert open(os.path.join(out_f, "tests.json"), "rb").read() == open(os.path.join(GOLDEN, "desc_chain_run_ptz_reloc.json"), "rb").read()
    assert base._run_tool(*args, "--on_device", "--output", out_d).returncode == 0
    data = open(os.path.join(out_d, "tests.json"), "rb").read()
    assert hashlib.sha256(data).hexdigest() == json.load(open(os.path.join(GOLDEN, "run_ptz_reloc_before_prior.json")))["on_device_plain"]


def test_krt_optimizer_behind_the_gate_equals_the_hand_composition(pkg):
    """KRTOptimizer::SetGateModel(1, iters) -> Solve(): four queries with one match in three replaced by a random pixel, each through the
    host class and through RotFocalGate.run + krt_solve_batch on the compacted matches: the same camera, summary, kept set and focal."""
    api = pkg.api
    rb = pkg.synth.make_reloc_batch(4, 96, seed_id=6, factor_type=0)
    uvr, uvc = np.asarray(rb.uv_ref, np.float32), np.array(rb.uv_cur, dtype=np.float32)
    rng = np.random.default_rng(11)
    wrong = rng.random(len(uvc)) < 0.3
    uvc[wrong] = rng.uniform([0, 0], [1920, 1080], (int(wrong.sum()), 2))
    L = host_util.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for q in range(4):
        s = slice(int(rb.match_ptr[q]), int(rb.match_ptr[q + 1]))
        a, b = np.ascontiguousarray(uvr[s]), np.ascontiguousarray(uvc[s])
        ref, cur = np.ascontiguousarray(rb.cam_ref[q], dtype=np.float64), np.array(rb.cam_init[q], dtype=np.float64)
        assert L.ptzh_krt_solve_gate_model(p(ref), p(cur), len(a), p(a), p(b), 200, C.c_double(100.0), 0, 2, 128, None, None, None) == -1
        assert L.ptzh_krt_solve_gate_model(p(ref), p(cur), len(a), p(a), p(b), 200, C.c_double(100.0), 0, 1, 0, None, None, None) == -1
        for iters in (128, 300):
            cur = np.array(rb.cam_init[q], dtype=np.float64)
            kept, f, summ = np.zeros(len(a), dtype=np.uint8), C.c_double(), api.LmSummary()
            assert L.ptzh_krt_solve_gate_model(p(ref), p(cur), len(a), p(a), p(b), 200, C.c_double(100.0), 0, 1, iters, C.byref(summ), p(kept),
                                               C.byref(f)) == 1
            with api.RotFocalGate(1, len(a)) as gate:
                g = gate.run(np.array([0, len(a)]), a, b, ref[None], rb.cam_init[q][None], thresh=4.0, min_inliers=6, iters=iters)
            one = types.SimpleNamespace(n_query=1, match_ptr=g["out_ptr"], uv_ref=g["out_uv_a"], uv_cur=g["out_uv_b"], cam_ref=ref[None],
                                        cam_init=rb.cam_init[q][None], factor_type=0)
            cam, s1, acc, _ = api.krt_solve_batch(one, **LM)
            assert acc[0] == 1 and g["found"][0] == 1 and np.array_equal(kept, g["mask"]) and f.value == g["model"][0, 0]
            assert kept[wrong[s]].sum() <= 2  # (the recovery cap of the contract's tests: max(2, n / 100) wrong matches)
            assert summ.as_dict() == s1[0]
            back = np.zeros(15)
            R9 = np.zeros(9)
            L.ptzh_camera_roundtrip(p(np.ascontiguousarray(cam[0])), p(back), p(R9))  # (the class hands K, R, t, dist back through Camera)
            assert cur[0] == cam[0, 0] and np.abs(cur - back).max() < 1e-12
        cur = np.array(rb.cam_init[q], dtype=np.float64)
        plain = np.array(rb.cam_init[q], dtype=np.float64)
        assert L.ptzh_krt_solve_gate_model(p(ref), p(cur), len(a), p(a), p(b), 200, C.c_double(100.0), 0, 0, 128, None, None, None) == \
            L.ptzh_krt_solve(p(ref), p(plain), len(a), p(a), p(b), 200, C.c_double(100.0), 0, None, None)
        assert np.array_equal(cur, plain)  # model 0: the class as it was
