"""GPU tests of run_ptz_reloc --match_descriptors --landmarks --landmark_shortlist R: the tool's records carry n_shortlist and
n_visible and are those of api.Relocalizer.run(landmarks=, landmark_shortlist=) on the same files and the same map; with
--landmark_prior_params the images without a prior, and with --landmark_sequence the untracked frames, go through the shortlisted
landmark run; the flag needs --landmarks; and without it --landmarks alone, with --landmark_prior_params and with
--landmark_sequence write the bytes the tool wrote before the flag existed (tests/golden/run_ptz_reloc_before_landmark_shortlist.json:
the sha256 of the three outputs, recorded from a build of the commit before on the data sets of data_set() and sequence_set())."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import host_util
from test_gpu_run_ptz_reloc_landmarks_prior import _as_the_tool_reads, _cameras, _rig_on_disk, _run_tool, _tool_map

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "run_ptz_reloc_before_landmark_shortlist.json")
LM = dict(max_num_iterations=200)
WITH_PRIOR, REST = [0, 1, 3, 4, 6, 7], [2, 5]
R = 4


def data_set(pkg, root):
    """eight queries against the 20-view rig on disk, and a priors file (0.3 degrees / 2 % off) for six of them"""
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=8, n_feat=200, visible_share=0.7, seed=3)
    refs, tests = pkg.synth_reloc.make_reloc_descriptors(sc, D=64, noise=8, n_distractors=20, seed=1, repeat_share=0.7)
    paths, names, args = _rig_on_disk(pkg, root, sc, refs, tests)
    pri = pkg.synth_reloc.perturb_cameras(sc.cam_gt, 0.3, 0.02, seed=2)
    pri[:, 2], pri[:, 3] = 960.0, 540.0
    entries = {os.path.splitext(names[q])[0]: pkg.dataset_io.camera_json_entry(os.path.splitext(names[q])[0], pri[q], 1920, 1080) for q in WITH_PRIOR}
    prior_path = os.path.join(root, "priors.json")
    json.dump({"cameras": entries}, open(prior_path, "w"), indent=4)
    return sc, refs, tests, paths, names, args, prior_path


def sequence_set(pkg, root):
    """synth_reloc's sequence on disk: 12 frames, 0.4 degrees and 1 % zoom per frame, a cut of 45 degrees at frame 7"""
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt
    sc = pkg.synth_reloc.make_reloc_sequence(rig, n_frames=12, step_deg=0.4, zoom_rate=0.01, cut_at=7, n_feat=200, visible_share=0.7, seed=5)
    refs, tests = pkg.synth_reloc.make_reloc_descriptors(sc, D=64, noise=8, n_distractors=20, seed=1, repeat_share=0.7)
    paths, names, args = _rig_on_disk(pkg, root, sc, refs, tests)
    return sc, names, args


def digest(out):
    return hashlib.sha256(open(os.path.join(out, "tests.json"), "rb").read()).hexdigest()


@pytest.mark.parametrize("extra", [[], ["--inlier_matches", "--trim_px", "2", "--uncertainty", "--shortlist_probes", "128", "--shortlist_min_votes", "2"]],
                         ids=["plain", "gated_trimmed_cov_m128"])
def test_records_are_the_python_runs(pkg, tmp_path, extra):
    sc, refs, tests, paths, names, args, prior_path = data_set(pkg, str(tmp_path))
    out = str(tmp_path / "out")
    r = _run_tool(*args, "--landmarks", "--landmark_shortlist", str(R), *extra, "--output", out)
    assert r.returncode == 0, r.stderr[-1500:]
    got = _cameras(out)
    assert len(got) == 8, r.stderr[-1500:]
    (rp, rd, rk), (qp, qd, qk) = refs, tests
    api = pkg.api
    ref_entries = json.load(open(paths["ref_params"]))["cameras"]
    ref_in = np.stack([_as_the_tool_reads(ref_entries[os.path.splitext(n)[0]]) for n in paths["ref_names"]])
    kw = dict(inlier_matches=bool(extra), match=dict(min_matches=8), trim=dict(trim_px=2.0) if extra else None, uncertainty=bool(extra), **LM)
    sl = dict(max_refs=R, n_probes=128, min_votes=2) if extra else dict(max_refs=R)
    with api.DescSet(rp, rd, rk) as Rs, api.DescSet(qp, qd, qk) as T, api.Relocalizer(Rs, ref_in) as rl, _tool_map(api, Rs, ref_in, sc.n_ref) as lmap:
        res = rl.run(T, sc.query_wh, landmarks=lmap, landmark_shortlist=sl, **kw)
        n_lm = lmap.n_landmarks
    assert res["accepted"].all() and (res["n_short"] > 0).all() and (res["n_visible"] < n_lm).all()
    for q in range(8):
        rec = got[os.path.splitext(names[q])[0]]
        back, R9 = np.zeros(15), np.zeros(9)
        cam = np.ascontiguousarray(res["cam"][q])
        host_util.lib().ptzh_camera_roundtrip(cam.ctypes.data_as(C.c_void_p), back.ctypes.data_as(C.c_void_p), R9.ctypes.data_as(C.c_void_p))
        assert rec["K"][0] == cam[0] and np.abs(np.array(rec["R"]) - R9).max() < 1e-12, q
        assert rec["n_shortlist"] == res["n_short"][q] and rec["n_visible"] == res["n_visible"][q] and "tracked" not in rec
        assert rec["n_landmarks"] == n_lm and rec["n_matches"] == res["n_matches"][q]
        # (accuracy only where the run removes wrong matches: 70 % of this texture repeats, and the plain run has neither gate nor trim)
        assert not extra or abs(rec["K"][0] / sc.cam_gt[q, 0] - 1) < 5e-3
        assert ("sigma_f" in rec) == bool(extra) and ("rms_px" in rec) == bool(extra)


def test_images_without_a_prior_and_untracked_frames_are_shortlisted(pkg, tmp_path):
    """--landmark_prior_params: the six images with an entry are tracked (n_shortlist 0), the other two shortlisted; --landmark_sequence:
    frame 0 is not tracked and has n_shortlist > 0, frames 1 .. 6 and 8 .. 11 are tracked, frame 7 (lost under frame 6's camera after
    the cut) is run again untracked, through the shortlist"""
    sc, refs, tests, paths, names, args, prior_path = data_set(pkg, str(tmp_path / "a"))
    out = str(tmp_path / "out_a")
    r = _run_tool(*args, "--landmarks", "--landmark_prior_params", prior_path, "--landmark_shortlist", str(R), "--output", out)
    assert r.returncode == 0, r.stderr[-1500:]
    got = _cameras(out)
    assert len(got) == 8
    for q in range(8):
        rec = got[os.path.splitext(names[q])[0]]
        assert rec["tracked"] == int(q in WITH_PRIOR) and (rec["n_shortlist"] > 0) == (q in REST) and rec["n_visible"] > 0, (q, rec)
        assert abs(rec["K"][0] / sc.cam_gt[q, 0] - 1) < 5e-3
    sq, snames, sargs = sequence_set(pkg, str(tmp_path / "b"))
    out = str(tmp_path / "out_b")
    r = _run_tool(*sargs, "--landmarks", "--landmark_sequence", "--landmark_shortlist", str(R), "--output", out)
    assert r.returncode == 0, r.stderr[-1500:]
    got = _cameras(out)
    recs = [got[os.path.splitext(n)[0]] for n in snames]
    print("tracked", [rec["tracked"] for rec in recs], "n_shortlist", [rec["n_shortlist"] for rec in recs], "n_visible", [rec["n_visible"] for rec in recs])
    assert len(got) == 12 and [rec["tracked"] for rec in recs] == [0, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1]
    assert recs[0]["tracked"] == 0 and recs[0]["n_shortlist"] > 0 and recs[0]["n_visible"] > 0
    for q, rec in enumerate(recs):
        assert abs(rec["K"][0] / sq.cam_gt[q, 0] - 1) < 5e-3, q
        assert rec["n_shortlist"] == 0 if rec["tracked"] else rec["n_shortlist"] >= 0


def test_without_the_flag_the_old_bytes_stand_and_the_flag_needs_landmarks(pkg, tmp_path):
    want = json.load(open(GOLDEN))
    sc, refs, tests, paths, names, args, prior_path = data_set(pkg, str(tmp_path / "a"))
    for key, extra in (("landmarks", []), ("landmark_prior_params", ["--landmark_prior_params", prior_path])):
        out = str(tmp_path / key)
        r = _run_tool(*args, "--landmarks", *extra, "--output", out)
        assert r.returncode == 0, r.stderr[-1500:]
        assert digest(out) == want[key], key
        assert all("n_shortlist" not in rec for rec in _cameras(out).values())
    sq, snames, sargs = sequence_set(pkg, str(tmp_path / "b"))
    out = str(tmp_path / "landmark_sequence")
    assert _run_tool(*sargs, "--landmarks", "--landmark_sequence", "--output", out).returncode == 0
    assert digest(out) == want["landmark_sequence"]
    err = str(tmp_path / "err")
    for bad in (["--landmark_shortlist", "4"], ["--on_device", "--landmark_shortlist", "4"], ["--shortlist", "4", "--landmark_shortlist", "4"]):
        r = _run_tool(*args, *bad, "--output", err)
        assert r.returncode == 1 and "--landmarks" in r.stderr, (bad, r.returncode, r.stderr[-300:])
    for bad in (["--landmark_shortlist", "0"], ["--landmark_shortlist", "4", "--shortlist_probes", "0"], ["--landmark_shortlist", "4", "--shortlist", "4"]):
        r = _run_tool(*args, "--landmarks", *bad, "--output", err)
        assert r.returncode == 1, (bad, r.returncode, r.stderr[-300:])
    r = _run_tool(*args, "--shortlist_probes", "64", "--output", err)  # the vote options still need one of the two lists
    assert r.returncode == 1 and "--landmark_shortlist" in r.stderr
    assert not os.path.exists(os.path.join(err, "tests.json"))
