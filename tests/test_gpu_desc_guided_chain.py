"""The guided matcher in the chain, on descriptors that repeat: the device's two-pass table (first pass, pair homographies, guided
pass) against the restatement's with the host estimator, and a directory of feature files to calibrated cameras
(run_ptz_ba --match_descriptors --match_guided 4) and to relocalized test images (run_ptz_reloc ... --match_guided 4).  The tools'
saved matches are held to the restatement, their outputs to their own runs on the saved match file, byte for byte."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import desc_guided_util as gu
import desc_match_util as du
import host_util as hu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = dict(ratio=0.8, cross_check=True, min_matches=8)


def _run_tool(name, *args):
    return subprocess.run([os.path.join(ROOT, "ptz-calib_amd", "bin", name), *args], capture_output=True, text=True, timeout=600)


def _sets(csr, ia, ib):
    out = {}
    for p, (x, y) in enumerate(zip(np.asarray(ia).tolist(), np.asarray(ib).tolist())):
        sl = slice(int(csr["match_ptr"][p]), int(csr["match_ptr"][p + 1]))
        if sl.stop > sl.start:
            out[(x, y)] = sorted(zip(csr["idx_a"][sl].tolist(), csr["idx_b"][sl].tolist()))
    return out


@pytest.fixture(scope="module")
def rig(pkg, tmp_path_factory):
    """the repeated-descriptor rig on disk and the restatement's two passes over every unordered pair (the tool's pair list)"""
    root = str(tmp_path_factory.mktemp("desc_guided_rig"))
    sc, tb, ptr, desc, kp, paths = gu.repeated_rig(pkg, root)
    ia, ib = (x.astype(np.int32) for x in np.triu_indices(tb.n_img, 1))
    first, H, found, second = gu.two_pass(hu.lib(), desc, ptr, kp, desc, ptr, kp, ia, ib, radius_px=4.0, ransac_thresh=4.0, min_inliers=6, **OPT)
    return dict(sc=sc, tb=tb, ptr=ptr, desc=desc, kp=kp, paths=paths, ia=ia, ib=ib, first=first, H=H, found=found, second=second,
                table={(s, d): set(ms) for s, d, ms in tb.pairs()})


def test_two_pass_table_on_the_device(pkg, rig):
    """first pass, ptz_homography_ransac_batch on its pixel pairs, the gate's rule, guided pass: the restatement's arrays, and the
    caps of the CPU guard on the device's own output"""
    ia, ib, ptr, desc, kp = (rig[k] for k in ("ia", "ib", "ptr", "desc", "kp"))
    with pkg.api.DescSet(ptr, desc, kp) as s:
        first = pkg.api.match_descriptors(s, s, ia, ib, ratio=0.8, cross_check=1, min_matches=8)
        for k in ("match_ptr", "idx_a", "idx_b", "dist2"):
            assert np.array_equal(first[k], rig["first"][k]), k
        H, found, mask, _ = pkg.api.find_homographies(first["match_ptr"], first["uv_a"], first["uv_b"], ransac_thresh=4.0)
        ones = np.bincount(np.repeat(np.arange(len(ia)), np.diff(first["match_ptr"])), weights=mask, minlength=len(ia)).astype(np.int64)
        ok = ((found == 1) & (ones >= 6)).astype(np.int32)
        assert np.array_equal(ok, rig["found"]) and np.array_equal(H.reshape(-1, 9)[ok == 1], rig["H"][ok == 1])
        second = pkg.api.match_descriptors_guided(s, s, ia, ib, H.reshape(-1, 9), ok, 4.0, ratio=0.8, cross_check=1, min_matches=8)
    gu.assert_equal(second, rig["second"], "two passes")
    n1, hit1, tot = gu.table_score(first, ia, ib, rig["table"])
    n2, hit2, _ = gu.table_score(second, ia, ib, rig["table"])
    print(f"table {tot}; first pass {n1} matches, {hit1} in the table, {n1 - hit1} not; two passes {n2}, {hit2} in the table, {n2 - hit2} not; "
          f"guided pass {second['device_ms']:.3f} ms, first pass {first['device_ms']:.3f} ms")
    assert hit1 <= 0.60 * tot and n1 - hit1 >= 0.10 * n1
    assert hit2 >= 0.90 * tot and n2 - hit2 <= 0.005 * n2


def test_run_ptz_ba_match_guided(pkg, rig, tmp_path):
    paths = rig["paths"]
    args = ["-i", paths["images"], "-a", paths["annotation"]]
    saved = str(tmp_path / "m.txt")
    out_a, out_b, out_u = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "u")
    ra = _run_tool("run_ptz_ba", *args, "-f", paths["features"], "--output=" + out_a, "--match_descriptors", "--match_guided", "4",
                   "--save_matches", saved)
    assert ra.returncode == 0, ra.stderr[-3000:]
    # the saved file holds the restatement's two-pass matches, (j, i) as the transposed (i, j) sorted by the feature of j, in table order
    names = paths["names"]
    want = {}
    for (x, y), ms in _sets(rig["second"], rig["ia"], rig["ib"]).items():
        want[(names[x], names[y])] = ms
        want[(names[y], names[x])] = sorted((j, i) for i, j in ms)
    blocks = du.read_matches_file(saved)
    assert blocks == want and list(blocks.keys()) == sorted(want.keys())
    assert "Registered/Total: 20/20" in ra.stderr and "Georeferencing End: success" in ra.stderr, ra.stderr[-2000:]
    res = json.load(open(os.path.join(out_a, "rig0.json")))["cameras"]
    fe = np.array([abs(res[n]["K"][0] / rig["sc"].cam_gt[i, 0] - 1) for i, n in enumerate(res)])
    print(f"relative focal error with --match_guided 4: max {fe.max():.3e}")
    assert len(res) == 20 and fe.max() < 2e-3
    # the same tool on a copy of the feature directory whose pairs_matches.txt is the saved file
    feat2 = str(tmp_path / "features2")
    shutil.copytree(paths["features"], feat2)
    shutil.copyfile(saved, os.path.join(feat2, "pairs_matches.txt"))
    rb = _run_tool("run_ptz_ba", *args, "-f", feat2, "--output=" + out_b)
    assert rb.returncode == 0, rb.stderr[-3000:]
    assert open(os.path.join(out_a, "rig0.json"), "rb").read() == open(os.path.join(out_b, "rig0.json"), "rb").read()
    # the unguided run on the same data, once: its outcome is reported, not asserted
    ru = _run_tool("run_ptz_ba", *args, "-f", paths["features"], "--output=" + out_u, "--match_descriptors")
    line = [l for l in ru.stderr.splitlines() if "Registered/Total" in l or "Georeferencing End" in l]
    msg = f"unguided run on the same data: exit {ru.returncode}, {line}"
    if ru.returncode == 0 and os.path.exists(os.path.join(out_u, "rig0.json")):
        un = json.load(open(os.path.join(out_u, "rig0.json")))["cameras"]
        idx = {n: i for i, n in enumerate(res)}
        fu = [abs(un[n]["K"][0] / rig["sc"].cam_gt[idx[n], 0] - 1) for n in un if n in idx]
        msg += f", {len(un)} cameras, max relative focal error {max(fu) if fu else float('nan'):.3e}"
    print(msg)
    # the flag needs --match_descriptors, and a radius that is a positive number
    assert _run_tool("run_ptz_ba", *args, "-f", paths["features"], "--output=" + out_u, "--match_guided", "4").returncode == 1
    assert _run_tool("run_ptz_ba", *args, "-f", paths["features"], "--output=" + out_u, "--match_descriptors", "--match_guided", "0").returncode == 1


def test_run_ptz_reloc_match_guided(pkg, tmp_path):
    rb, (rptr, rdesc, rkp), (tptr, tdesc, tkp), paths = gu.repeated_reloc(pkg, str(tmp_path))
    n = rb.n_query
    assert n == 24
    args = ["--ref_images", paths["ref_images"], "--ref_features", paths["ref_features"], "--ref_params", paths["ref_params"],
            "--test_images", paths["test_images"]]
    saved = str(tmp_path / "m.txt")
    out_a, out_b = str(tmp_path / "a"), str(tmp_path / "b")
    ra = _run_tool("run_ptz_reloc", *args, "--test_features", paths["test_features"], "--output", out_a, "--match_descriptors",
                   "--match_guided", "4", "--save_matches", saved)
    assert ra.returncode == 0, ra.stderr[-3000:]
    # blocks test image by test image, references in order; their matches are the restatement's two passes
    it, ir = (x.astype(np.int32) for x in np.divmod(np.arange(n * n), n))
    first, H, found, second = gu.two_pass(hu.lib(), rdesc, rptr, rkp, tdesc, tptr, tkp, ir, it, radius_px=4.0, ransac_thresh=4.0, min_inliers=6, **OPT)
    sets = _sets(second, ir, it)
    blocks = du.read_matches_file(saved)
    assert blocks == {(paths["ref_names"][r], paths["test_names"][t]): ms for (r, t), ms in sets.items()}
    assert list(blocks.keys()) == [(paths["ref_names"][r], paths["test_names"][t]) for t in range(n) for r in range(n) if (r, t) in sets]
    # the data repeats: the first pass alone keeps little of a query's matches, the two passes nearly all
    n1, n2 = np.diff(first["match_ptr"])[ir == it], np.diff(second["match_ptr"])[ir == it]
    print(f"matches of a query with its own reference: first pass {n1.min()} .. {n1.max()}, two passes {n2.min()} .. {n2.max()} of 96")
    assert n1.max() <= 0.6 * 96 and n2.min() >= 0.9 * 96
    for t in range(n):  # FindBestMatch: most matches, the first (lowest reference) on a tie -- reference q for test q
        best, size = -1, 0
        for r in range(n):
            if len(sets.get((r, t), ())) > size:
                best, size = r, len(sets[(r, t)])
        assert best == t
    # the run on its own saved file
    feat2 = str(tmp_path / "test_features2")
    shutil.copytree(paths["test_features"], feat2)
    shutil.copyfile(saved, os.path.join(feat2, "pairs_matches.txt"))
    rb2 = _run_tool("run_ptz_reloc", *args, "--test_features", feat2, "--output", out_b)
    assert rb2.returncode == 0, rb2.stderr[-3000:]
    assert open(os.path.join(out_a, "tests.json"), "rb").read() == open(os.path.join(out_b, "tests.json"), "rb").read()
    res = json.load(open(os.path.join(out_a, "tests.json")))["cameras"]
    assert list(res.keys()) == [os.path.splitext(t)[0] for t in paths["test_names"]], ra.stderr[-2000:]
    for q in range(n):  # the right reference was chosen: the camera is the query's (the bound of the tool tests)
        assert abs(res[os.path.splitext(paths["test_names"][q])[0]]["K"][0] / rb.cam_gt[q, 0] - 1) < 5e-3
    assert _run_tool("run_ptz_reloc", *args, "--test_features", paths["test_features"], "--output", out_b, "--match_guided", "4").returncode == 1
