"""The descriptor matcher in the chain: a directory of feature files to calibrated cameras (run_ptz_ba --match_descriptors) and to
relocalized test images (run_ptz_reloc --match_descriptors), the match table being computed instead of read.  The matcher's
output is held to the numpy restatement as sets per pair; the tools to their own runs on the saved match file, byte for byte."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import desc_match_util as du

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _run_tool(name, *args):
    return subprocess.run([os.path.join(ROOT, "ptz-calib_amd", "bin", name), *args], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def rig(pkg, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("desc_rig"))
    sc, tb, ptr, desc, kp, paths = du.chain_rig(pkg, root)
    n = tb.n_img
    ia, ib = (x.astype(np.int32) for x in np.divmod(np.arange(n * n), n))
    k = ia != ib
    ia, ib = ia[k], ib[k]
    want = du.match_pairs(desc, ptr, desc, ptr, ia, ib, ratio=0.8, cross_check=True, min_matches=8)
    return dict(root=root, sc=sc, tb=tb, ptr=ptr, desc=desc, kp=kp, paths=paths, ia=ia, ib=ib, want=want)


def _sets(csr, ia, ib):
    out = {}
    for p, (x, y) in enumerate(zip(ia.tolist(), ib.tolist())):
        sl = slice(int(csr["match_ptr"][p]), int(csr["match_ptr"][p + 1]))
        if sl.stop > sl.start:
            out[(x, y)] = set(zip(csr["idx_a"][sl].tolist(), csr["idx_b"][sl].tolist()))
    return out


def test_matcher_recovers_the_table(pkg, rig):
    table = {(s, d): set(ms) for s, d, ms in rig["tb"].pairs()}
    # the test's own guard, on the CPU: the restatement recovers exactly the table's matches, and no other pair is non-empty
    assert _sets(rig["want"], rig["ia"], rig["ib"]) == table
    with pkg.api.DescSet(rig["ptr"], rig["desc"], rig["kp"]) as s:
        got = pkg.api.match_descriptors(s, s, rig["ia"], rig["ib"], ratio=0.8, cross_check=1, min_matches=8)
    assert _sets(got, rig["ia"], rig["ib"]) == table
    for k in ("match_ptr", "idx_a", "idx_b", "dist2"):
        assert np.array_equal(got[k], rig["want"][k]), k


def test_run_ptz_ba_match_descriptors(pkg, rig, tmp_path):
    paths = rig["paths"]
    args = ["-i", paths["images"], "-a", paths["annotation"]]
    saved = str(tmp_path / "m.txt")
    out_a, out_b, out_f = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "f")
    ra = _run_tool("run_ptz_ba", *args, "-f", paths["features"], "--output=" + out_a, "--match_descriptors", "--save_matches", saved)
    assert ra.returncode == 0, ra.stderr[-3000:]
    # the saved file holds the restatement's matches, (j, i) as the transposed (i, j) sorted by the feature of j, in table order
    names = paths["names"]
    want = {(names[x], names[y]): sorted(ms) for (x, y), ms in _sets(rig["want"], rig["ia"], rig["ib"]).items()}
    blocks = du.read_matches_file(saved)
    assert blocks == want and list(blocks.keys()) == sorted(want.keys())
    # the same tool on a copy of the feature directory whose pairs_matches.txt is the saved file
    feat2 = str(tmp_path / "features2")
    shutil.copytree(paths["features"], feat2)
    shutil.copyfile(saved, os.path.join(feat2, "pairs_matches.txt"))
    rb = _run_tool("run_ptz_ba", *args, "-f", feat2, "--output=" + out_b)
    assert rb.returncode == 0, rb.stderr[-3000:]
    ja, jb = open(os.path.join(out_a, "rig0.json"), "rb").read(), open(os.path.join(out_b, "rig0.json"), "rb").read()
    assert ja == jb
    # every view registered, at the accuracy of the run on the generator's own match file (the tool tests' bound for this rig)
    rf = _run_tool("run_ptz_ba", *args, "-f", paths["features"], "--output=" + out_f)
    assert rf.returncode == 0 and "Registered/Total: 20/20" in rf.stderr
    assert "Registered/Total: 20/20" in ra.stderr and "Georeferencing End: success" in ra.stderr
    res, ref = (json.load(open(os.path.join(o, "rig0.json")))["cameras"] for o in (out_a, out_f))
    fe = np.array([abs(res[n]["K"][0] / rig["sc"].cam_gt[i, 0] - 1) for i, n in enumerate(res)])
    fr = np.array([abs(ref[n]["K"][0] / rig["sc"].cam_gt[i, 0] - 1) for i, n in enumerate(ref)])
    print(f"relative focal error: matched descriptors max {fe.max():.3e}, generator's match file max {fr.max():.3e}")
    assert len(res) == 20 and fe.max() < 2e-3 and fr.max() < 2e-3
    # without the flag: the bytes the parent commit's tool wrote on this data set
    assert open(os.path.join(out_f, "rig0.json"), "rb").read() == open(os.path.join(GOLDEN, "desc_chain_run_ptz_ba.json"), "rb").read()
    # the window option: only pairs of cyclic index distance <= 2
    rw = _run_tool("run_ptz_ba", *args, "-f", paths["features"], "--output=" + str(tmp_path / "w"), "--match_descriptors", "--match_window", "2",
                   "--save_matches", str(tmp_path / "w.txt"))
    print("run_ptz_ba --match_window 2: exit", rw.returncode, [l for l in rw.stderr.splitlines() if "Registered" in l or "End" in l])
    # neighbours and next neighbours of the ring of views are enough to chain every view in
    assert rw.returncode == 0 and "Registered/Total: 20/20" in rw.stderr and "Georeferencing End: success" in rw.stderr, rw.stderr[-2000:]
    wb = du.read_matches_file(str(tmp_path / "w.txt"))
    idx = {n: i for i, n in enumerate(names)}
    near = {k: v for k, v in want.items() if min(abs(idx[k[0]] - idx[k[1]]), 20 - abs(idx[k[0]] - idx[k[1]])) <= 2}
    assert wb == near and len(near) > 0


def test_run_ptz_reloc_match_descriptors(pkg, tmp_path):
    rb, (rptr, rdesc), (tptr, tdesc), paths = du.chain_reloc(pkg, str(tmp_path))
    n = rb.n_query
    args = ["--ref_images", paths["ref_images"], "--ref_features", paths["ref_features"], "--ref_params", paths["ref_params"],
            "--test_images", paths["test_images"]]
    saved = str(tmp_path / "m.txt")
    out_a, out_b, out_f = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "f")
    ra = _run_tool("run_ptz_reloc", *args, "--test_features", paths["test_features"], "--output", out_a, "--match_descriptors", "--save_matches", saved)
    assert ra.returncode == 0, ra.stderr[-3000:]
    # blocks test image by test image, references in order; their matches are the restatement's
    it, ir = (x.astype(np.int32) for x in np.divmod(np.arange(n * n), n))
    want = du.match_pairs(rdesc, rptr, tdesc, tptr, ir, it, ratio=0.8, cross_check=True, min_matches=8)
    sets = _sets(want, ir, it)
    blocks = du.read_matches_file(saved)
    assert blocks == {(paths["ref_names"][r], paths["test_names"][t]): sorted(ms) for (r, t), ms in sets.items()}
    assert list(blocks.keys()) == [(paths["ref_names"][r], paths["test_names"][t]) for t in range(n) for r in range(n) if (r, t) in sets]
    # FindBestMatch on the restatement's matches: most matches, the first (lowest reference) on a tie -- reference q for test q
    for t in range(n):
        best, size = -1, 0
        for r in range(n):
            if len(sets.get((r, t), ())) > size:
                best, size = r, len(sets[(r, t)])
        assert best == t and size >= 0.9 * 96
    # the run on its own saved file
    feat2 = str(tmp_path / "test_features2")
    shutil.copytree(paths["test_features"], feat2)
    shutil.copyfile(saved, os.path.join(feat2, "pairs_matches.txt"))
    rb2 = _run_tool("run_ptz_reloc", *args, "--test_features", feat2, "--output", out_b)
    assert rb2.returncode == 0, rb2.stderr[-3000:]
    assert open(os.path.join(out_a, "tests.json"), "rb").read() == open(os.path.join(out_b, "tests.json"), "rb").read()
    res = json.load(open(os.path.join(out_a, "tests.json")))["cameras"]
    # every query is accepted, as on the generator's own match file (the golden run below), in the order of the test images
    assert list(res.keys()) == [os.path.splitext(t)[0] for t in paths["test_names"]], ra.stderr[-2000:]
    for q in range(n):  # the right reference was chosen: the camera is the query's (the bound of the tool tests)
        assert abs(res[os.path.splitext(paths["test_names"][q])[0]]["K"][0] / rb.cam_gt[q, 0] - 1) < 5e-3
    # without the flag: the bytes the parent commit's tool wrote on this data set
    rf = _run_tool("run_ptz_reloc", *args, "--test_features", paths["test_features"], "--output", out_f)
    assert rf.returncode == 0
    assert open(os.path.join(out_f, "tests.json"), "rb").read() == open(os.path.join(GOLDEN, "desc_chain_run_ptz_reloc.json"), "rb").read()
    assert list(json.load(open(os.path.join(out_f, "tests.json")))["cameras"].keys()) == list(res.keys())
