"""GPU tests of run_ptz_reloc --match_descriptors --landmarks on the synthetic data-set writer: 24 of 24 test images are
relocalized against the landmark map; the cameras are those of api.Relocalizer.run(landmarks=) on the same files (the references
matched among themselves, the host TracksBuilder's tracks, the map); the flag combinations that make no sense exit non-zero with a
message; and without the flag the tool writes the bytes it wrote before this mode existed (the digests of
tests/golden/run_ptz_reloc_before_prior.json, taken from the earlier tool on desc_match_util.chain_reloc's data)."""
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
FLAG_SETS = {"plain": [], "all": ["--match_guided", "4", "--inlier_matches", "--trim_px", "2", "--uncertainty", "--multi_ref", "3"]}
LM = dict(max_num_iterations=200)


def _run_tool(*args):
    return subprocess.run([os.path.join(ROOT, "ptz-calib_amd", "bin", "run_ptz_reloc"), *args], capture_output=True, text=True, timeout=600)


def _cameras(out):
    return json.load(open(os.path.join(out, "tests.json")))["cameras"]


@pytest.fixture(scope="module")
def on_disk(pkg, tmp_path_factory):
    """the 20-view rig's references and 24 queries as a run_ptz_reloc data set (the layout of write_reloc_set)"""
    root = str(tmp_path_factory.mktemp("reloc_landmarks"))
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=24, n_feat=200, visible_share=0.7, seed=3)
    refs, tests = pkg.synth_reloc.make_reloc_descriptors(sc, D=64, noise=8, n_distractors=20, seed=1)
    n = max(sc.n_ref, sc.n_query)
    rb = types.SimpleNamespace(n_query=n, cam_ref=np.resize(rig, (n, 15)), cam_gt=np.resize(rig, (n, 15)), cam_init=np.resize(rig, (n, 15)),
                               match_ptr=np.zeros(n + 1, np.int64), uv_ref=np.zeros((0, 2), np.float32), uv_cur=np.zeros((0, 2), np.float32),
                               factor_type=0)
    paths = pkg.dataset_io.write_reloc_set(root, rb)
    (rp, rd, rk), (qp, qd, qk) = refs, tests
    for kind, keep in (("ref", sc.n_ref), ("test", sc.n_query)):  # the writer makes n of each: keep the rig's references, the scene's queries
        for name in paths[kind + "_names"][keep:]:
            os.remove(os.path.join(paths[kind + "_images"], name))
        for f in os.listdir(paths[kind + "_features"]):
            os.remove(os.path.join(paths[kind + "_features"], f))
    ref_names, names = paths["ref_names"][:sc.n_ref], paths["test_names"][:sc.n_query]
    pkg.dataset_io.write_features(paths["ref_features"], ref_names, rp, rk, desc=rd)
    pkg.dataset_io.write_features(paths["test_features"], names, qp, qk, desc=qd)
    ref_params = os.path.join(root, "ref_params_rig.json")
    json.dump({"cameras": {os.path.splitext(nm)[0]: pkg.dataset_io.camera_json_entry(os.path.splitext(nm)[0], rig[i], 1920, 1080)
                           for i, nm in enumerate(ref_names)}}, open(ref_params, "w"), indent=4)
    args = ["--ref_images", paths["ref_images"], "--ref_features", paths["ref_features"], "--ref_params", ref_params,
            "--test_images", paths["test_images"], "--test_features", paths["test_features"], "--match_descriptors"]
    return sc, rig, refs, tests, names, args, root, ref_params, ref_names


def _as_the_tool_reads(entry):
    """the 15 doubles the tool makes of a camera record (K, R, t, dist; the rotation vector by the host library's RodriguesInv)"""
    R = np.ascontiguousarray(entry["R"], dtype=np.float64)
    rv = np.zeros(3)
    host_util.lib().ptzh_rodrigues_inv(R.ctypes.data_as(C.c_void_p), rv.ctypes.data_as(C.c_void_p))
    K = entry["K"]
    return np.array([K[0], K[4], K[2], K[5], *rv, *entry["t"], *entry["dist"]])


@pytest.mark.parametrize("extra", [[], ["--inlier_matches", "--trim_px", "2", "--uncertainty"]], ids=["plain", "gated_trimmed_cov"])
def test_landmarks_relocalize_every_image_with_the_python_runs_cameras(pkg, on_disk, extra):
    sc, rig, refs, tests, names, args, root, ref_params, ref_names = on_disk
    out = os.path.join(root, "out_" + str(len(extra)))
    r = _run_tool(*args, "--landmarks", *extra, "--output", out)
    assert r.returncode == 0, r.stderr[-1500:]
    got = _cameras(out)
    assert len(got) == 24, r.stderr[-1500:]
    # the same map in python: the references among themselves (every pair once), the host TracksBuilder, min 2 views
    api = pkg.api
    (rp, rd, rk), (qp, qd, qk) = refs, tests
    cams_in = np.stack([_as_the_tool_reads(json.load(open(ref_params))["cameras"][os.path.splitext(n)[0]]) for n in ref_names])
    ia, ib = np.triu_indices(sc.n_ref, 1)
    with api.DescSet(rp, rd, rk) as R, api.DescSet(qp, qd, qk) as T, api.Relocalizer(R, cams_in) as rl:
        m = api.match_descriptors(R, R, ia.astype(np.int32), ib.astype(np.int32), min_matches=8)
        pairs = [(int(a), int(b), list(zip(m["idx_a"][m["match_ptr"][p]:m["match_ptr"][p + 1]].tolist(), m["idx_b"][m["match_ptr"][p]:m["match_ptr"][p + 1]].tolist())))
                 for p, (a, b) in enumerate(zip(ia, ib)) if m["match_ptr"][p + 1] > m["match_ptr"][p]]
        tracks = host_util.tracks_build(pairs, min_len=2)
        views = [(i, f) for t in sorted(tracks) for i, f in sorted(tracks[t].items())]
        tp = np.concatenate([[0], np.cumsum([len(tracks[t]) for t in sorted(tracks)])]).astype(np.int64)
        with api.LandmarkMap(R, cams_in, tp, [v[0] for v in views], [v[1] for v in views], min_views=2) as lmap:
            res = rl.run(T, sc.query_wh, landmarks=lmap, match=dict(min_matches=8), inlier_matches=bool(extra), trim=dict(trim_px=2.0) if extra else None,
                         uncertainty=bool(extra), **LM)
            n_lm = lmap.n_landmarks
    assert res["accepted"].all() and n_lm > 1000
    for q, n in enumerate(names):
        rec = got[os.path.splitext(n)[0]]
        back, R9 = np.zeros(15), np.zeros(9)
        cam = np.ascontiguousarray(res["cam"][q])
        host_util.lib().ptzh_camera_roundtrip(cam.ctypes.data_as(C.c_void_p), back.ctypes.data_as(C.c_void_p), R9.ctypes.data_as(C.c_void_p))
        # (the focal is the run's bits; the matrix goes through the tool's own camera class on its way into the record)
        assert rec["K"][0] == cam[0] and np.abs(np.array(rec["R"]) - R9).max() < 1e-12, q
        assert rec["n_landmarks"] == n_lm and rec["n_matches"] == res["n_matches"][q]
        assert abs(rec["K"][0] / sc.cam_gt[q, 0] - 1) < 5e-3
        assert ("sigma_f" in rec) == bool(extra) and ("rms_px" in rec) == bool(extra)


def test_flag_combinations_that_are_errors(on_disk):
    sc, rig, refs, tests, names, args, root, ref_params, ref_names = on_disk
    out = os.path.join(root, "out_err")
    for bad in (["--match_guided", "4"], ["--shortlist", "4"], ["--multi_ref", "2"], ["--prior_params", ref_params], ["--sequence"],
                ["--save_matches", os.path.join(root, "m.txt")], ["--landmark_min_views", "0"]):
        r = _run_tool(*args, "--landmarks", *bad, "--output", out)
        assert r.returncode == 1 and "--landmark" in r.stderr, (bad, r.returncode, r.stderr[-300:])
    r = _run_tool(*args[:-1], "--landmarks", "--output", out)  # without --match_descriptors
    assert r.returncode == 1 and "--match_descriptors" in r.stderr
    r = _run_tool(*args, "--landmark_min_views", "3", "--output", out)  # without --landmarks
    assert r.returncode == 1 and "--landmarks" in r.stderr
    assert not os.path.exists(os.path.join(out, "tests.json"))


@pytest.mark.parametrize("flags", list(FLAG_SETS))
def test_without_the_flag_the_bytes_are_the_earlier_tools(pkg, tmp_path, flags):
    rb, _, _, paths = du.chain_reloc(pkg, str(tmp_path))
    args = ["--ref_images", paths["ref_images"], "--ref_features", paths["ref_features"], "--ref_params", paths["ref_params"],
            "--test_images", paths["test_images"], "--test_features", paths["test_features"], "--match_descriptors"]
    want = json.load(open(GOLDEN))
    out = str(tmp_path / ("on_device_" + flags))
    r = _run_tool(*args, "--on_device", *FLAG_SETS[flags], "--output", out)
    assert r.returncode == 0, r.stderr[-1500:]
    data = open(os.path.join(out, "tests.json"), "rb").read()
    assert hashlib.sha256(data).hexdigest() == want["on_device_" + flags], flags
    assert b"n_landmarks" not in data
