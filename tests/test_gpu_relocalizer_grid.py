"""GPU tests of the guided_grid selector above the matcher: api.Relocalizer.run(..., guided_grid=True) returns every per-query
output and the match table bit-equal to guided_grid=False, from a prior camera (the data of test_gpu_relocalizer_prior.py) and with the
gate-then-guided stage 2 (desc_guided_util.repeated_reloc); run_ptz_reloc and run_ptz_ba write the same bytes with and without
--guided_grid, the --save_matches file included."""
import filecmp
import json
import os
import subprocess

import numpy as np
import pytest

import desc_guided_util as gu
from test_gpu_relocalizer_prior import LM, MATCH, PER_QUERY, PRIOR, TRIM, _same, data  # noqa: F401  (data: the module's fixture)
from test_gpu_run_ptz_reloc_prior import _rig_on_disk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = ("match_ptr", "idx_a", "idx_b", "dist2", "uv_a", "uv_b")


def _run_tool(name, *args):
    return subprocess.run([os.path.join(ROOT, "ptz-calib_amd", "bin", name), *args], capture_output=True, text=True, timeout=600)


def _assert_same_run(x, y, what):
    for key in PER_QUERY:
        assert _same(x[key], y[key]), (what, key)
    for key in TABLE:
        assert np.array_equal(x["table"][key], y["table"][key]), (what, "table", key)
    for key in ("match_ptr", "uv_ref", "uv_cur", "src"):
        assert np.array_equal(x["asm"][key], y["asm"][key]), (what, "assembled", key)


@pytest.mark.parametrize("ft", [0, 1])
@pytest.mark.parametrize("K", [1, 4])
def test_tracked_runs_are_equal(pkg, data, K, ft):  # noqa: F811
    """24 queries, repeated texture, priors 0.3 degrees and 2 % off; camera, accepted, summary, sel_ref, n_matches, n_inliers, trim
    report and covariance, and table()"""
    d = data[ft]
    runs = []
    with pkg.api.DescSet(*d.refs) as refs, pkg.api.DescSet(*d.tests) as tests, pkg.api.Relocalizer(refs, d.rig) as rl:
        for grid in (False, True, False):
            got = rl.run(tests, d.sc.query_wh, max_refs=K, factor_type=ft, match=MATCH, prior=dict(PRIOR, cams=d.prior), trim=TRIM,
                         uncertainty=True, guided_grid=grid, **LM)
            got["table"], got["asm"] = rl.table(), rl.matches()
            runs.append(got)
    _assert_same_run(runs[1], runs[0], (K, ft))
    _assert_same_run(runs[2], runs[0], (K, ft, "scan kernel after the grid kernel"))
    assert runs[1]["accepted"].sum() == 24 and runs[1]["table"]["match_ptr"][-1] > 5000 and runs[1]["stage_ms"][1] > 0 and runs[1]["stage_ms"][0] == 0


def test_stage_two_is_equal_and_the_option_is_checked(pkg, tmp_path):
    """run(guided_radius=4): the gate on all pairs, then the guided pass under its H -- with either kernel; any value of guided_grid
    but 0 and 1 is PTZ_EINVAL"""
    rb, refs, tests, _ = gu.repeated_reloc(pkg, str(tmp_path))
    wh = np.tile(np.array([1920, 1080], dtype=np.int32), (rb.n_query, 1))
    runs = []
    with pkg.api.DescSet(*refs) as R, pkg.api.DescSet(*tests) as T, pkg.api.Relocalizer(R, rb.cam_ref) as rl:
        for grid in (False, True):
            got = rl.run(T, wh, max_refs=4, guided_radius=4.0, inlier_matches=True, match=MATCH, trim=TRIM, uncertainty=True, guided_grid=grid, **LM)
            got["table"], got["asm"] = rl.table(), rl.matches()
            runs.append(got)
        for bad in (2, -1):
            with pytest.raises(pkg.api.PtzError) as e:
                rl.run(T, wh, guided_radius=4.0, match=MATCH, guided_grid=bad, **LM)
            assert e.value.code == -1
            with pytest.raises(pkg.api.PtzError):
                rl.run(T, wh, match=MATCH, guided_grid=bad, **LM)   # checked whether or not a guided pass would run
    _assert_same_run(runs[1], runs[0], "stage 2")
    assert runs[1]["accepted"].all() and runs[1]["stage_ms"][1] > 0 and runs[1]["table"]["match_ptr"][-1] > 1000


def _assert_same_files(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and names
    for n in names:
        assert filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False), n


def test_run_ptz_reloc_writes_the_same_bytes(pkg, tmp_path):
    """--prior_params (six of eight queries tracked, the others all-pairs with --match_guided 4) with and without --guided_grid"""
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=8, n_feat=200, seed=3)
    refs, tests = pkg.synth_reloc.make_reloc_descriptors(sc, D=64, noise=8, n_distractors=20, seed=1, repeat_share=0.7)
    paths, names, args = _rig_on_disk(pkg, str(tmp_path), sc, refs, tests)
    pri = pkg.synth_reloc.perturb_cameras(sc.cam_gt, 0.3, 0.02, seed=2)
    pri[:, 2], pri[:, 3] = 960.0, 540.0
    entries = {os.path.splitext(names[q])[0]: pkg.dataset_io.camera_json_entry(os.path.splitext(names[q])[0], pri[q], 1920, 1080) for q in (0, 1, 3, 4, 6, 7)}
    prior_path = str(tmp_path / "priors.json")
    json.dump({"cameras": entries}, open(prior_path, "w"), indent=4)
    outs = []
    for tag, extra in (("scan", []), ("grid", ["--guided_grid"])):
        out, sm = str(tmp_path / ("out_" + tag)), str(tmp_path / (tag + ".txt"))
        r = _run_tool("run_ptz_reloc", *args, "--prior_params", prior_path, "--match_guided", "4", "--multi_ref", "3", "--output", out, "--save_matches", sm, *extra)
        assert r.returncode == 0, r.stderr[-1500:]
        outs.append((out, sm))
    _assert_same_files(outs[0][0], outs[1][0])
    assert filecmp.cmp(outs[0][1], outs[1][1], shallow=False) and os.path.getsize(outs[0][1]) > 1000
    cams = json.load(open(os.path.join(outs[1][0], "tests.json")))["cameras"]
    assert len(cams) == 8 and sum(c["tracked"] for c in cams.values()) == 6


def test_run_ptz_ba_writes_the_same_bytes(pkg, tmp_path):
    """--match_descriptors --match_guided 4 on the 20-view rig with repeated descriptors, with and without --guided_grid"""
    _, _, _, _, _, paths = gu.repeated_rig(pkg, str(tmp_path / "rig"))
    args = ["-i", paths["images"], "-a", paths["annotation"], "-f", paths["features"], "--match_descriptors", "--match_guided", "4"]
    outs = []
    for tag, extra in (("scan", []), ("grid", ["--guided_grid"])):
        out, sm = str(tmp_path / ("out_" + tag)), str(tmp_path / (tag + ".txt"))
        r = _run_tool("run_ptz_ba", *args, "--output=" + out, "--save_matches", sm, *extra)
        assert r.returncode == 0 and "Registered/Total: 20/20" in r.stderr, r.stderr[-2000:]
        outs.append((out, sm))
    _assert_same_files(outs[0][0], outs[1][0])
    assert filecmp.cmp(outs[0][1], outs[1][1], shallow=False) and os.path.getsize(outs[0][1]) > 10000
