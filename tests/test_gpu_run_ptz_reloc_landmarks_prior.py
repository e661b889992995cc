"""GPU tests of run_ptz_reloc --match_descriptors --landmarks --landmark_prior_params / --landmark_sequence: the tool's records are
those of api.Relocalizer.run(landmarks=, landmark_prior=) on the same files and the same map (the references matched among
themselves, the host TracksBuilder's tracks); a 12-frame pan / zoom sweep with a cut is tracked frame to frame against the map and
re-detected after the cut by the dense landmark run; the new flags need --landmarks; and without them the tool writes the bytes it
wrote before (tests/golden/desc_chain_run_ptz_reloc.json, and the on-device digest of tests/golden/run_ptz_reloc_before_prior.json)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import types

import numpy as np
import pytest

import desc_match_util as du
import host_util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LM = dict(max_num_iterations=200)


def _run_tool(*args):
    return subprocess.run([os.path.join(ROOT, "ptz-calib_amd", "bin", "run_ptz_reloc"), *args], capture_output=True, text=True, timeout=600)


def _cameras(out):
    return json.load(open(os.path.join(out, "tests.json")))["cameras"]


def _rig_on_disk(pkg, root, sc, refs, tests):
    """the rig's references and the scene's queries as a run_ptz_reloc data set (the layout of write_reloc_set)"""
    rig = sc.ref_cams
    rb = types.SimpleNamespace(n_query=sc.n_ref, cam_ref=rig, cam_gt=rig, cam_init=rig, match_ptr=np.zeros(sc.n_ref + 1, np.int64),
                               uv_ref=np.zeros((0, 2), np.float32), uv_cur=np.zeros((0, 2), np.float32), factor_type=0)
    paths = pkg.dataset_io.write_reloc_set(root, rb)
    (rp, rd, rk), (qp, qd, qk) = refs, tests
    pkg.dataset_io.write_features(paths["ref_features"], paths["ref_names"], rp, rk, desc=rd)
    names = paths["test_names"][:sc.n_query]
    for n in paths["test_names"][sc.n_query:]:
        os.remove(os.path.join(paths["test_images"], n))
    for f in os.listdir(paths["test_features"]):
        os.remove(os.path.join(paths["test_features"], f))
    pkg.dataset_io.write_features(paths["test_features"], names, qp, qk, desc=qd)
    args = ["--ref_images", paths["ref_images"], "--ref_features", paths["ref_features"], "--ref_params", paths["ref_params"],
            "--test_images", paths["test_images"], "--test_features", paths["test_features"], "--match_descriptors"]
    return paths, names, args


def _as_the_tool_reads(entry):
    """the 15 doubles the tool makes of a camera record (K, R, t, dist; the rotation vector by the host library's RodriguesInv)"""
    R = np.ascontiguousarray(entry["R"], dtype=np.float64)
    rv = np.zeros(3)
    host_util.lib().ptzh_rodrigues_inv(R.ctypes.data_as(C.c_void_p), rv.ctypes.data_as(C.c_void_p))
    K = entry["K"]
    return np.array([K[0], K[4], K[2], K[5], *rv, *entry["t"], *entry["dist"]])


def _tool_map(api, R, cams_in, n_ref):
    """the map the tool builds: the references among themselves (every pair once), the host TracksBuilder, min 2 views"""
    ia, ib = np.triu_indices(n_ref, 1)
    m = api.match_descriptors(R, R, ia.astype(np.int32), ib.astype(np.int32), min_matches=8)
    pairs = [(int(a), int(b), list(zip(m["idx_a"][m["match_ptr"][p]:m["match_ptr"][p + 1]].tolist(), m["idx_b"][m["match_ptr"][p]:m["match_ptr"][p + 1]].tolist())))
             for p, (a, b) in enumerate(zip(ia, ib)) if m["match_ptr"][p + 1] > m["match_ptr"][p]]
    tracks = host_util.tracks_build(pairs, min_len=2)
    views = [(i, f) for t in sorted(tracks) for i, f in sorted(tracks[t].items())]
    tp = np.concatenate([[0], np.cumsum([len(tracks[t]) for t in sorted(tracks)])]).astype(np.int64)
    return api.LandmarkMap(R, cams_in, tp, [v[0] for v in views], [v[1] for v in views], min_views=2)


@pytest.mark.parametrize("extra", [[], ["--trim_px", "2", "--uncertainty", "--guided_grid", "--landmark_prior_radius", "30"]], ids=["plain", "trimmed_cov_grid_r30"])
def test_landmark_prior_params_records_are_the_python_runs(pkg, tmp_path, extra):
    """Eight queries, priors 0.3 degrees / 2 % off for six of them in the file: those six are one tracked landmark run, the other two
    go through the dense landmark run (gated: the new flags imply --inlier_matches); the focal of every record is the bits of
    api.Relocalizer.run on the same arrays."""
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=8, n_feat=200, visible_share=0.7, seed=3)
    refs, tests = pkg.synth_reloc.make_reloc_descriptors(sc, D=64, noise=8, n_distractors=20, seed=1, repeat_share=0.7)
    paths, names, args = _rig_on_disk(pkg, str(tmp_path), sc, refs, tests)
    pri = pkg.synth_reloc.perturb_cameras(sc.cam_gt, 0.3, 0.02, seed=2)
    pri[:, 2], pri[:, 3] = 960.0, 540.0
    with_prior, rest = [0, 1, 3, 4, 6, 7], [2, 5]
    entries = {os.path.splitext(names[q])[0]: pkg.dataset_io.camera_json_entry(os.path.splitext(names[q])[0], pri[q], 1920, 1080) for q in with_prior}
    prior_path = str(tmp_path / "priors.json")
    json.dump({"cameras": entries}, open(prior_path, "w"), indent=4)
    out = str(tmp_path / "out")
    r = _run_tool(*args, "--landmarks", "--landmark_prior_params", prior_path, *extra, "--output", out)
    assert r.returncode == 0, r.stderr[-1500:]
    got = _cameras(out)
    assert len(got) == 8, r.stderr[-1500:]
    (rp, rd, rk), (qp, qd, qk) = refs, tests
    api = pkg.api

    def subset(qs):
        ptr = np.concatenate([[0], np.cumsum([qp[q + 1] - qp[q] for q in qs])]).astype(np.int64)
        rows = np.concatenate([np.arange(qp[q], qp[q + 1]) for q in qs])
        return api.DescSet(ptr, qd[rows], qk[rows])

    ref_entries = json.load(open(paths["ref_params"]))["cameras"]
    ref_in = np.stack([_as_the_tool_reads(ref_entries[os.path.splitext(n)[0]]) for n in paths["ref_names"]])
    cams_in = np.stack([_as_the_tool_reads(json.load(open(prior_path))["cameras"][os.path.splitext(names[q])[0]]) for q in with_prior])
    kw = dict(inlier_matches=True, match=dict(min_matches=8), trim=dict(trim_px=2.0) if extra else None, uncertainty=bool(extra), **LM)
    with api.DescSet(rp, rd, rk) as R, api.Relocalizer(R, ref_in) as rl, _tool_map(api, R, ref_in, sc.n_ref) as lmap:
        with subset(with_prior) as T:
            trk = rl.run(T, sc.query_wh[with_prior], landmarks=lmap, landmark_prior=dict(cams=cams_in, radius_px=30.0 if extra else 40.0),
                         guided_grid=bool(extra), **kw)
        with subset(rest) as T:
            den = rl.run(T, sc.query_wh[rest], landmarks=lmap, **kw)
        n_lm = lmap.n_landmarks
    assert trk["accepted"].all() and den["accepted"].all() and n_lm > 100
    for res, qs, flag in ((trk, with_prior, 1), (den, rest, 0)):
        for k, q in enumerate(qs):
            rec = got[os.path.splitext(names[q])[0]]
            back, R9 = np.zeros(15), np.zeros(9)
            cam = np.ascontiguousarray(res["cam"][k])
            host_util.lib().ptzh_camera_roundtrip(cam.ctypes.data_as(C.c_void_p), back.ctypes.data_as(C.c_void_p), R9.ctypes.data_as(C.c_void_p))
            # (the focal is the run's bits; the matrix goes through the tool's own camera class on its way into the record)
            assert rec["tracked"] == flag and rec["K"][0] == cam[0] and np.abs(np.array(rec["R"]) - R9).max() < 1e-12, (q, flag)
            assert rec["n_landmarks"] == n_lm and rec["n_matches"] == res["n_matches"][k]
            assert rec["n_visible"] == (trk["n_visible"][k] if flag else 0) and (rec["n_visible"] > 0) == bool(flag)
            assert abs(rec["K"][0] / sc.cam_gt[q, 0] - 1) < 5e-3
            assert ("sigma_f" in rec) == bool(extra) and ("rms_px" in rec) == bool(extra)
    if not extra:  # --landmarks without the new flags: the dense run's records, no new key
        out_l = str(tmp_path / "out_dense")
        assert _run_tool(*args, "--landmarks", "--output", out_l).returncode == 0
        dense = _cameras(out_l)
        assert len(dense) == 8 and all("n_landmarks" in rec and "tracked" not in rec and "n_visible" not in rec for rec in dense.values())


def test_landmark_sequence_tracks_frame_to_frame_and_redetects_after_a_cut(pkg, tmp_path):
    """synth_reloc's sequence: 12 frames, 0.4 degrees and 1 % zoom per frame (some 30 px at the corners, inside the 40 px radius), a
    cut of 45 degrees at frame 7: frames 1 .. 6 and 8 .. 11 are tracked against the map from the frame before, frames 0 and 7 are not
    (7 is lost under frame 6's camera and run again dense), all are registered."""
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt
    sc = pkg.synth_reloc.make_reloc_sequence(rig, n_frames=12, step_deg=0.4, zoom_rate=0.01, cut_at=7, n_feat=200, visible_share=0.7, seed=5)
    refs, tests = pkg.synth_reloc.make_reloc_descriptors(sc, D=64, noise=8, n_distractors=20, seed=1, repeat_share=0.7)
    paths, names, args = _rig_on_disk(pkg, str(tmp_path), sc, refs, tests)
    out = str(tmp_path / "out")
    r = _run_tool(*args, "--landmarks", "--landmark_sequence", "--output", out)
    assert r.returncode == 0, r.stderr[-1500:]
    got = _cameras(out)
    assert len(got) == 12, r.stderr[-1500:]
    recs = [got[os.path.splitext(n)[0]] for n in names]
    flags = [rec["tracked"] for rec in recs]
    print("tracked", flags, "n_visible", [rec["n_visible"] for rec in recs], "n_matches", [rec["n_matches"] for rec in recs])
    assert flags == [0, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1]
    for q, rec in enumerate(recs):
        assert abs(rec["K"][0] / sc.cam_gt[q, 0] - 1) < 5e-3, q
        assert (rec["n_visible"] > 0) == bool(flags[q])


def test_the_new_flags_need_landmarks_and_the_old_bytes_stand(pkg, tmp_path):
    rb, _, _, paths = du.chain_reloc(pkg, str(tmp_path))
    base = ["--ref_images", paths["ref_images"], "--ref_features", paths["ref_features"], "--ref_params", paths["ref_params"],
            "--test_images", paths["test_images"], "--test_features", paths["test_features"]]
    args = base + ["--match_descriptors"]
    out = str(tmp_path / "err")
    for bad in (["--landmark_prior_params", paths["ref_params"]], ["--landmark_sequence"], ["--landmark_prior_radius", "20"],
                ["--on_device", "--landmark_sequence"], ["--sequence", "--landmark_prior_radius", "20"]):
        r = _run_tool(*args, *bad, "--output", out)
        assert r.returncode == 1 and "--landmarks" in r.stderr, (bad, r.returncode, r.stderr[-300:])
    for bad in (["--landmark_prior_radius", "20"], ["--landmark_sequence", "--landmark_prior_radius", "0"],
                ["--landmark_sequence", "--landmark_prior_radius", "-4"], ["--landmark_sequence", "--sequence"],
                ["--landmark_sequence", "--save_matches", str(tmp_path / "m.txt")]):
        r = _run_tool(*args, "--landmarks", *bad, "--output", out)
        assert r.returncode == 1 and "--landmark" in r.stderr, (bad, r.returncode, r.stderr[-300:])
    assert not os.path.exists(os.path.join(out, "tests.json"))
    # without the new flags: the match-file run and the on-device run write what they wrote
    out_f, out_d = str(tmp_path / "file"), str(tmp_path / "device")
    assert _run_tool(*base, "--output", out_f).returncode == 0
    assert open(os.path.join(out_f, "tests.json"), "rb").read() == open(os.path.join(GOLDEN, "desc_chain_run_ptz_reloc.json"), "rb").read()
    assert _run_tool(*args, "--on_device", "--output", out_d).returncode == 0
    data = open(os.path.join(out_d, "tests.json"), "rb").read()
    assert hashlib.sha256(data).hexdigest() == json.load(open(os.path.join(GOLDEN, "run_ptz_reloc_before_prior.json")))["on_device_plain"]
