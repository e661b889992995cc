"""GPU tests of run_ptz_reloc --match_descriptors --prior_params / --sequence: the tool's records are those of
api.Relocalizer.run(prior=...) on the same files; a 12-frame pan / zoom sweep with a cut is tracked frame to frame and re-detected
after the cut; without the new flags the tool writes the bytes it wrote before this mode existed (digests of tests.json taken from
the tool as it was, on desc_match_util.chain_reloc's data, for the flag sets of test_gpu_run_ptz_reloc_shortlist.py)."""
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "run_ptz_reloc_before_prior.json")
FLAG_SETS = {"plain": [], "multi_ref": ["--multi_ref", "2"],
             "all": ["--match_guided", "4", "--inlier_matches", "--trim_px", "2", "--uncertainty", "--multi_ref", "3"]}
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


def test_prior_params_records_are_the_python_runs(pkg, tmp_path):
    """Eight queries, priors 0.3 degrees / 2 % off for six of them in the file: those six are one tracked run (K = 3), the other two
    go through the all-pairs path; the focal of every record is the bits of api.Relocalizer.run on the same arrays."""
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=8, n_feat=200, seed=3)
    refs, tests = pkg.synth_reloc.make_reloc_descriptors(sc, D=64, noise=8, n_distractors=20, seed=1, repeat_share=0.7)
    paths, names, args = _rig_on_disk(pkg, str(tmp_path), sc, refs, tests)
    pri = pkg.synth_reloc.perturb_cameras(sc.cam_gt, 0.3, 0.02, seed=2)
    pri[:, 2], pri[:, 3] = 960.0, 540.0
    with_prior = [0, 1, 3, 4, 6, 7]
    entries = {os.path.splitext(names[q])[0]: pkg.dataset_io.camera_json_entry(os.path.splitext(names[q])[0], pri[q], 1920, 1080) for q in with_prior}
    prior_path = str(tmp_path / "priors.json")
    json.dump({"cameras": entries}, open(prior_path, "w"), indent=4)
    out, sm = str(tmp_path / "out"), str(tmp_path / "matches.txt")
    r = _run_tool(*args, "--prior_params", prior_path, "--multi_ref", "3", "--output", out, "--save_matches", sm)
    assert r.returncode == 0, r.stderr[-1500:]
    got = _cameras(out)
    assert len(got) == 8
    (rp, rd, rk), (qp, qd, qk) = refs, tests
    api = pkg.api

    def subset(qs):
        ptr = np.concatenate([[0], np.cumsum([qp[q + 1] - qp[q] for q in qs])]).astype(np.int64)
        rows = np.concatenate([np.arange(qp[q], qp[q + 1]) for q in qs])
        return api.DescSet(ptr, qd[rows], qk[rows])

    cams_in = np.stack([_as_the_tool_reads(json.load(open(prior_path))["cameras"][os.path.splitext(names[q])[0]]) for q in with_prior])
    rest = [2, 5]
    with api.DescSet(rp, rd, rk) as R, api.Relocalizer(R, rig) as rl:
        with subset(with_prior) as T:
            trk = rl.run(T, sc.query_wh[with_prior], max_refs=3, inlier_matches=True, match=dict(min_matches=8), prior=dict(cams=cams_in), **LM)
        with subset(rest) as T:
            den = rl.run(T, sc.query_wh[rest], max_refs=3, inlier_matches=True, match=dict(min_matches=8), **LM)
    assert trk["accepted"].all() and den["accepted"].all()
    for res, qs, flag in ((trk, with_prior, 1), (den, rest, 0)):
        for k, q in enumerate(qs):
            rec = got[os.path.splitext(names[q])[0]]
            back, R9 = np.zeros(15), np.zeros(9)
            cam = np.ascontiguousarray(res["cam"][k])
            host_util.lib().ptzh_camera_roundtrip(cam.ctypes.data_as(C.c_void_p), back.ctypes.data_as(C.c_void_p), R9.ctypes.data_as(C.c_void_p))
            # (the focal is the run's bits; the matrix goes through the tool's own camera class on its way into the record)
            assert rec["tracked"] == flag and rec["K"][0] == cam[0] and np.abs(np.array(rec["R"]) - R9).max() < 1e-12, (q, flag)
            assert rec["n_refs"] == res["n_sel"][k] and rec["n_matches"] == res["n_matches"][k]
            assert rec["n_shortlist"] == (trk["n_short"][k] if flag else sc.n_ref)
            assert abs(rec["K"][0] / sc.cam_gt[q, 0] - 1) < 5e-3
    blocks = du.read_matches_file(sm)
    tracked_blocks = [b for b in blocks if b[1] in {names[q] for q in with_prior}]
    assert 0 < len(tracked_blocks) <= 8 * len(with_prior) and len(blocks) > len(tracked_blocks)
    # the flags need each other
    assert _run_tool(*args[:-1], "--prior_params", prior_path, "--output", out).returncode == 1
    assert _run_tool(*args, "--prior_radius", "20", "--output", out).returncode == 1
    assert _run_tool(*args, "--sequence", "--prior_refs", "0", "--output", out).returncode == 1


def test_sequence_tracks_frame_to_frame_and_redetects_after_a_cut(pkg, tmp_path):
    """12 frames, 0.4 degrees and 1 % zoom per frame (some 30 px at the corners, inside the 40 px radius), a cut of 45 degrees at
    frame 7: frames 1 .. 6 and 8 .. 11 are tracked from the frame before, frames 0 and 7 are not (7 is lost under frame 6's camera and run again over all pairs), all are registered."""
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt
    sc = pkg.synth_reloc.make_reloc_sequence(rig, n_frames=12, step_deg=0.4, zoom_rate=0.01, cut_at=7, n_feat=200, seed=5)
    refs, tests = pkg.synth_reloc.make_reloc_descriptors(sc, D=64, noise=8, n_distractors=20, seed=1, repeat_share=0.7)
    paths, names, args = _rig_on_disk(pkg, str(tmp_path), sc, refs, tests)
    out = str(tmp_path / "out")
    r = _run_tool(*args, "--sequence", "--multi_ref", "3", "--output", out)
    assert r.returncode == 0, r.stderr[-1500:]
    got = _cameras(out)
    assert len(got) == 12, r.stderr[-1500:]
    flags = [got[os.path.splitext(n)[0]]["tracked"] for n in names]
    print("tracked", flags, "n_shortlist", [got[os.path.splitext(n)[0]]["n_shortlist"] for n in names])
    assert flags == [0, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1]
    for q, n in enumerate(names):
        assert abs(got[os.path.splitext(n)[0]]["K"][0] / sc.cam_gt[q, 0] - 1) < 5e-3, q


@pytest.mark.parametrize("flags", list(FLAG_SETS))
def test_without_the_new_flags_the_bytes_are_the_earlier_tools(pkg, tmp_path, flags):
    rb, _, _, paths = du.chain_reloc(pkg, str(tmp_path))
    args = ["--ref_images", paths["ref_images"], "--ref_features", paths["ref_features"], "--ref_params", paths["ref_params"],
            "--test_images", paths["test_images"], "--test_features", paths["test_features"], "--match_descriptors"]
    want = json.load(open(GOLDEN))
    for mode, extra in (("on_device", ["--on_device"]), ("shortlist", ["--shortlist", str(len(paths["ref_names"]))])):
        out = str(tmp_path / (mode + "_" + flags))
        r = _run_tool(*args, *extra, *FLAG_SETS[flags], "--output", out)
        assert r.returncode == 0, r.stderr[-1500:]
        data = open(os.path.join(out, "tests.json"), "rb").read()
        assert hashlib.sha256(data).hexdigest() == want[mode + "_" + flags], (mode, flags)
        assert b"tracked" not in data
