"""GPU tests of the RANSAC inlier gating of matches (ptz_match_gate, ptz_krt_solve_batch_gated, LoadInlierMatchesInfo on the
device, the tools' --inlier_matches).  The gate selects and moves data: its outputs are compared BITWISE with what numpy
builds from the public estimator (api.find_homographies) -- keep = mask & passes[pair_of_match] -- and the gated solve with
the composition by hand.  Only the robustness test holds cameras to the oracle with a tolerance, the one
test_gpu_parity.py::test_krt_batch_parity uses."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import homography_corpus as hc
import host_util as hu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- helpers
def numpy_gate(ptr, found, mask, min_inliers):
    """The rule: pair p passes with found[p] == 1 and at least max(min_inliers, 4) mask ones; a passing pair keeps its
    matches with mask byte 1 in their order.  Returns (keep [n_match] bool, out_ptr [n_pair + 1], out_index)."""
    n = np.diff(ptr)
    pair_of = np.repeat(np.arange(len(n)), n)
    ones = np.bincount(pair_of, weights=mask, minlength=len(n)).astype(np.int64)
    passes = (found == 1) & (ones >= max(min_inliers, 4))
    keep = mask.astype(bool) & passes[pair_of]
    out_ptr = np.concatenate([[0], np.cumsum(np.bincount(pair_of[keep], minlength=len(n)))]).astype(np.int64)
    return keep, out_ptr, np.flatnonzero(keep).astype(np.int32)


def outlier_batch(pkg, ftype, frac, n_query=96, n_match=128, seed_id=7, lost=()):
    """The batches of the issue's table: a fraction of uv_cur replaced by uniform pixels; queries `lost` entirely."""
    rb = pkg.synth.make_reloc_batch(n_query, n_match, seed_id=seed_id, factor_type=ftype)
    rb.uv_cur = np.array(rb.uv_cur, dtype=np.float32)
    rng = np.random.default_rng(11)
    k = rng.random(len(rb.uv_cur)) < frac
    rb.uv_cur[k] = rng.uniform([0, 0], [1920, 1080], (int(k.sum()), 2))
    rng2 = np.random.default_rng(5)
    for q in lost:
        a, b = int(rb.match_ptr[q]), int(rb.match_ptr[q + 1])
        rb.uv_cur[a:b] = rng2.uniform([0, 0], [1920, 1080], (b - a, 2))
    return rb


def compacted(rb, keep, out_ptr):
    return types.SimpleNamespace(n_query=rb.n_query, match_ptr=out_ptr, uv_ref=np.asarray(rb.uv_ref, np.float32)[keep],
                                 uv_cur=np.asarray(rb.uv_cur, np.float32)[keep], cam_ref=rb.cam_ref, cam_init=rb.cam_init,
                                 factor_type=rb.factor_type)


def by_hand(pkg, rb, min_inliers=0, **opt):
    """find_homographies, numpy compaction, krt_solve_batch on the compacted batch (empty ranges for queries that do not pass)."""
    ptr = np.asarray(rb.match_ptr, np.int64)
    H, found, mask, _ = pkg.api.find_homographies(ptr, rb.uv_ref, rb.uv_cur)
    keep, out_ptr, _ = numpy_gate(ptr, found, mask, min_inliers)
    cam, summ, acc, _ = pkg.api.krt_solve_batch(compacted(rb, keep, out_ptr), **opt)
    return dict(cam=cam, summ=summ, acc=acc, n_inliers=np.diff(out_ptr).astype(np.int32), mask=keep.astype(np.uint8), H=H, found=found,
                keep=keep, out_ptr=out_ptr)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------- test 4
def test_gate_matches_equals_numpy_compaction_of_public_mask(pkg):
    """The 2000-pair corpus (sizes 0-3000, NaN pixels, degenerate and pure-outlier pairs) through a gate of
    max_pair_matches = 3000: H, found, mask are api.find_homographies'; the compacted CSR and out_index are numpy's, for
    min_inliers 0, 4, 20.  Through a gate of 400: larger pairs have found = -1 and empty ranges, all others are unchanged."""
    ptr, src, dst = hc.corpus(seed=0, n_pairs=2000)
    H, found, mask, _ = pkg.api.find_homographies(ptr, src, dst)
    sizes = np.diff(ptr)
    assert sizes.max() == 3000 and sizes.min() == 0 and (found == 0).any() and (found == 1).sum() > 1500
    with pkg.api.MatchGate(len(sizes), len(src), 3000) as gate:
        for min_inl in (0, 4, 20):
            g = pkg.api.gate_matches(ptr, src, dst, min_inliers=min_inl, gate=gate)
            keep, out_ptr, out_index = numpy_gate(ptr, found, mask, min_inl)
            assert np.array_equal(g["found"], found) and same_bits(g["H"], H) and np.array_equal(g["mask"], mask)
            assert np.array_equal(g["out_ptr"], out_ptr) and np.array_equal(g["out_index"], out_index)
            assert same_bits(g["out_uv_a"], src[keep]) and same_bits(g["out_uv_b"], dst[keep])
        # min_inliers = 20 drops pairs that 4 keeps
        assert numpy_gate(ptr, found, mask, 20)[1][-1] < numpy_gate(ptr, found, mask, 4)[1][-1]
    g = pkg.api.gate_matches(ptr, src, dst, max_pair_matches=400)
    big = sizes > 400
    assert big.sum() > 10
    found4 = np.where(big, -1, found).astype(np.int32)
    big_m = np.repeat(big, sizes)
    mask4 = np.where(big_m, 0, mask).astype(np.uint8)
    keep, out_ptr, out_index = numpy_gate(ptr, found4, mask4, 0)
    assert np.array_equal(g["found"], found4) and np.array_equal(g["mask"], mask4)
    assert same_bits(g["H"], np.where(big[:, None, None], 0.0, H))
    assert np.array_equal(g["out_ptr"], out_ptr) and np.array_equal(g["out_index"], out_index)
    assert np.array_equal(np.diff(g["out_ptr"])[big], np.zeros(int(big.sum()), dtype=np.int64))
    assert same_bits(g["out_uv_a"], src[keep]) and same_bits(g["out_uv_b"], dst[keep])


# ---------------------------------------------------------------------------------------------------------------- test 5
LOST = (5, 17, 40, 95)  # queries whose uv_cur is uniform noise: the estimator may still find a model with a handful of "inliers"
CASES = [(0, 0.0, (), 0), (0, 0.3, (), 0), (0, 0.5, (), 0), (1, 0.0, (), 0), (1, 0.3, (), 0), (1, 0.5, (), 0), (0, 0.3, LOST, 0),
         (0, 0.3, LOST, 20)]


@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("ftype,frac,lost,min_inliers", CASES)
def test_gated_solve_equals_composition_by_hand(pkg, ftype, frac, lost, min_inliers, lanes):
    """ptz_krt_solve_batch_gated == find_homographies + numpy compaction + krt_solve_batch, for ALL queries: cameras, summaries,
    accepted, n_inliers, kept mask, H.  The noise queries pass or not as find_homographies says (they do with min_inliers = 0: a
    model with five "inliers"; none has twenty)."""
    rb = outlier_batch(pkg, ftype, frac, lost=lost)
    want = by_hand(pkg, rb, min_inliers=min_inliers, krt_lanes_per_query=lanes)
    cam, summ, acc, ninl, mask, H, ms = pkg.api.krt_solve_batch_gated(rb, min_inliers=min_inliers, krt_lanes_per_query=lanes)
    assert same_bits(cam, want["cam"]) and np.array_equal(acc, want["acc"])
    assert summ == want["summ"]
    assert np.array_equal(ninl, want["n_inliers"]) and np.array_equal(mask, want["mask"]) and same_bits(H, want["H"])
    assert ms[0] > 0 and ms[1] > 0
    if lost:
        print("noise queries: found", want["found"][list(lost)], "inliers kept", ninl[list(lost)], "accepted", acc[list(lost)])
        assert (np.delete(ninl, list(lost)) >= 20).all()
        if min_inliers == 20:
            assert (ninl[list(lost)] == 0).all()  # a uniform-noise query has no twenty matches on one homography


def test_query_that_does_not_pass_gets_the_empty_query_result(pkg):
    """The convention for a query the gate leaves without matches is ptz_krt_solve_batch's own for an empty range, pinned here:
    an LM over no residuals converges at once (termination 0, no iterations, zero cost), CheckResults finds nothing to object to
    (its reprojection error is 0 / 0, which is not >= the threshold) and the query counts as accepted, with the initial camera
    handed back through the world <- local conversion.  n_inliers = 0 is what tells such a query apart."""
    rb = outlier_batch(pkg, 0, 0.3, lost=(2,))
    cam, summ, acc, ninl, mask, H, _ = pkg.api.krt_solve_batch_gated(rb, min_inliers=30)
    empty = types.SimpleNamespace(n_query=1, match_ptr=np.zeros(2, dtype=np.int64), uv_ref=np.zeros((1, 2), np.float32),
                                  uv_cur=np.zeros((1, 2), np.float32), cam_ref=rb.cam_ref[2:3], cam_init=rb.cam_init[2:3], factor_type=0)
    ecam, esumm, eacc, _ = pkg.api.krt_solve_batch(empty)
    print("empty query:", esumm[0], "accepted", eacc[0], "camera moved by", np.abs(ecam[0] - rb.cam_init[2]).max())
    assert ninl[2] == 0 and not mask[rb.match_ptr[2]:rb.match_ptr[3]].any()
    assert same_bits(cam[2], ecam[0]) and summ[2] == esumm[0] and acc[2] == eacc[0]
    assert esumm[0]["termination_type"] == 0 and esumm[0]["num_iterations"] == 0 and esumm[0]["num_residuals"] == 0
    assert esumm[0]["initial_cost"] == 0.0 and esumm[0]["final_cost"] == 0.0 and eacc[0] == 1
    assert np.abs(ecam[0] - rb.cam_init[2]).max() < 1e-9
    assert (np.delete(ninl, 2) >= 30).all()


# ---------------------------------------------------------------------------------------------------------------- test 6
@pytest.mark.parametrize("ftype", [0, 1])
@pytest.mark.parametrize("frac,least", [(0.3, 71), (0.5, 52)])
def test_gate_brings_relocalization_back_under_outliers(pkg, orc, ftype, frac, least):
    """One wrong match in three (or two) takes the ungated solve from 96 accepted queries to none; the gated one accepts all 96
    with at least 71 (52) inliers each.  The gated cameras against the oracle on the kept matches, as test_krt_batch_parity
    holds the ungated ones: numeric-diff Jacobian, same termination and iteration count, f and rotation within 1e-6."""
    rb = outlier_batch(pkg, ftype, frac)
    _, _, acc0, _ = pkg.api.krt_solve_batch(rb)
    cam, summ, acc, ninl, mask, H, _ = pkg.api.krt_solve_batch_gated(rb)
    print(f"ftype {ftype} outliers {frac}: ungated accepted {int(acc0.sum())}, gated {int(acc.sum())}, inliers min {int(ninl.min())}")
    assert acc0.sum() == 0
    assert acc.sum() == 96 and ninl.min() >= least
    uvr, uvc = np.asarray(rb.uv_ref, np.float32), np.asarray(rb.uv_cur, np.float32)
    worst_f = worst_r = 0.0
    for q in range(rb.n_query):
        s = slice(rb.match_ptr[q], rb.match_ptr[q + 1])
        k = mask[s].astype(bool)
        loc0 = orc.krt_world_to_local(rb.cam_ref[q], rb.cam_init[q])
        loc, osumm, _ = orc.krt_solve(uvr[s][k], uvc[s][k], rb.cam_ref[q], loc0, factor_type=ftype, jacobian_mode=orc.JAC_NUMERIC)
        assert orc.krt_check(osumm, loc, 100.0)
        assert summ[q]["termination_type"] == osumm["termination_type"]
        assert summ[q]["num_iterations"] == osumm["num_iterations"]
        want = orc.krt_local_to_world(rb.cam_ref[q], loc, ftype)
        df = abs(cam[q, 0] - want[0]) / want[0]
        dr = np.abs(orc.rodrigues(cam[q, 4:7]) - orc.rodrigues(want[4:7])).max()
        worst_f, worst_r = max(worst_f, df), max(worst_r, dr)
        assert df < 1e-6 and dr < 1e-6
    print(f"  worst relative f difference {worst_f:.2e}, worst rotation entry difference {worst_r:.2e}, "
          f"median abs focal error {np.median(np.abs(cam[:, 0] - rb.cam_gt[:, 0])):.3f} px")


# ---------------------------------------------------------------------------------------------------------------- test 7
def test_device_resident_chain_gate_then_solve():
    """MatchGate.run_device then krt_solve_batch_device on its outputs, torch tensors, one stream, no host synchronisation in
    between; twice on one gate with different batches.  Own process with torch initialised first (see
    test_krt_device_resident_entry_matches_host_entry)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "run_match_gate_chain.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and r.stdout.count("gate chain ok") == 2, r.stdout[-2000:] + r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------------------- test 8
def _probe(cmd, a="", b=""):
    lib = hu.lib()
    lib.ptzh_io_probe.restype = C.c_void_p
    p = lib.ptzh_io_probe(cmd.encode(), a.encode(), b.encode())
    txt = C.string_at(p).decode()
    lib.ptzh_free(C.c_void_p(p))
    return json.loads(txt)


@pytest.mark.parametrize("min_inliers", [0, 6])
def test_device_gated_loader_equals_host_gated_loader(pkg, tmp_path, min_inliers):
    """LoadInlierMatchesInfo(..., device 0) on the rig test_gpu_homography.py loads ungated (24 views, 30 % outlier matches):
    every cell equals the host-gated loader's (indices, matches, mask, counts, H bits, H_empty, confidence), and H / H_empty are
    the ungated device loader's."""
    sc = pkg.synth.make_scene(2, 24, 150)
    tb = hc.inject_outliers(pkg.synth.make_match_table(sc), 0.3, seed=3)
    paths = pkg.dataset_io.write_rig(str(tmp_path), sc, tb)
    r = _probe("load_inliers_device:%d" % min_inliers, paths["images"], paths["features"])
    assert r["ok"] and r["loaded"] and r["identical"] and r["same_H"]
    assert r["table_cells"] == 24 * 24 and len(r["cells"]) == tb.n_pairs
    host = _probe("load_inliers:%d" % min_inliers, paths["images"], paths["features"])
    assert host["cells"] == r["cells"]
    kept = sum(c["num_inliers"] for c in r["cells"])
    assert 0 < kept < len(tb.t) and all(c["mask_ones"] == c["mask_len"] == c["num_inliers"] == len(c["matches"]) for c in r["cells"])


# ---------------------------------------------------------------------------------------------------------------- test 9
def _run_tool(name, *args):
    exe = os.path.join(ROOT, "ptz-calib_amd", "bin", name)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize("ftype", [0, 1])
def test_run_ptz_reloc_inlier_matches(pkg, orc, tmp_path, ftype):
    """run_ptz_reloc --inlier_matches on a written set with 30 % outlier matches writes the cameras krt_solve_batch_gated returns
    for the same problems (the files round numbers: 1e-9, as test_run_ptz_reloc_tool_matches_batch_api); without the flag it
    registers none."""
    rb = outlier_batch(pkg, ftype, 0.3, n_query=12, n_match=96, seed_id=6)
    paths = pkg.dataset_io.write_reloc_set(str(tmp_path), rb)
    args = ["--ref_images", paths["ref_images"], "--ref_features", paths["ref_features"], "--ref_params", paths["ref_params"],
            "--test_images", paths["test_images"], "--test_features", paths["test_features"]] + (["--dist"] if ftype else [])
    out0, out1 = str(tmp_path / "out_plain"), str(tmp_path / "out_gated")
    r0 = _run_tool("run_ptz_reloc", *args, "--output", out0)
    assert r0.returncode == 0, r0.stderr
    assert json.load(open(os.path.join(out0, "tests.json")))["cameras"] in ({}, None, [])
    assert r0.stderr.count("Running ptz-reloc failed") == rb.n_query
    r1 = _run_tool("run_ptz_reloc", *args, "--output", out1, "--inlier_matches")
    assert r1.returncode == 0, r1.stderr
    res = json.load(open(os.path.join(out1, "tests.json")))["cameras"]
    cam_w, summ, acc, ninl, _, _, _ = pkg.api.krt_solve_batch_gated(rb, min_inliers=6, max_num_iterations=200)  # the tool's default
    want = [os.path.splitext(paths["test_names"][q])[0] for q in range(rb.n_query) if acc[q] and ninl[q] > 0]
    assert list(res.keys()) == want and len(want) == rb.n_query
    for q in range(rb.n_query):
        c = res[os.path.splitext(paths["test_names"][q])[0]]
        K = np.array(c["K"]).reshape(3, 3); R = np.array(c["R"]).reshape(3, 3)
        assert abs(K[0, 0] / cam_w[q, 0] - 1) < 1e-9 and np.abs(R - orc.rodrigues(cam_w[q, 4:7])).max() < 1e-9
        if ftype:
            assert abs(c["dist"][0] - cam_w[q, 10]) < 1e-9


def _ba_run(paths, out_dir, *flags):
    r = _run_tool("run_ptz_ba", "-i", paths["images"], "-f", paths["features"], "-a", paths["annotation"], "--output=" + out_dir, *flags)
    m = re.search(r"Registered/Total: (\d+)/(\d+)", r.stderr)
    cams = None
    f = os.path.join(out_dir, "rig0.json")
    if r.returncode == 0 and os.path.exists(f):
        cams = json.load(open(f))["cameras"]
    return r, (int(m.group(1)) if m else None), cams


def _focal_errors(cams, sc, names):
    idx = {os.path.splitext(n)[0]: i for i, n in enumerate(names)}
    return np.array([abs(np.array(c["K"])[0] / sc.cam_gt[idx[n], 0] - 1) for n, c in cams.items()])


def test_run_ptz_ba_inlier_matches(pkg, tmp_path):
    """run_ptz_ba --gpu_homography --inlier_matches on a 20-view rig with 30 % outlier matches: exit status 0, finite cameras,
    and as many registered views as the tool reports on the clean data set of the rig.  The focal errors (gated, ungated, clean)
    are printed, not bounded.  Also printed: the run with --min_inliers 4, the bare rule -- two pairs of this rig have 8 matches
    with 3 and 4 wrong ones among them, a homography through four matches fits them exactly whichever they are, and the wrong
    matches that survive that way wreck a squared-loss pipeline (18 of 20 views, errors of hundreds of pixels); the tools'
    default of 6 inliers lets none of the 2 269 injected matches through here."""
    sc = pkg.synth.add_annotations(pkg.synth.make_scene(1, 20, 100))
    clean = pkg.dataset_io.write_rig(str(tmp_path / "clean"), sc, pkg.synth.make_match_table(sc), annotations=sc.obs3d)
    tb = hc.inject_outliers(pkg.synth.make_match_table(sc), 0.3, seed=4)
    dirty = pkg.dataset_io.write_rig(str(tmp_path / "dirty"), sc, tb, annotations=sc.obs3d)
    rc, n_clean, cams_clean = _ba_run(clean, str(tmp_path / "out_clean"))
    assert rc.returncode == 0 and n_clean is not None, rc.stderr
    rg, n_gated, cams_gated = _ba_run(dirty, str(tmp_path / "out_gated"), "--gpu_homography", "--inlier_matches")
    rp, n_plain, cams_plain = _ba_run(dirty, str(tmp_path / "out_plain"), "--gpu_homography")
    r4, n_four, cams_four = _ba_run(dirty, str(tmp_path / "out_four"), "--gpu_homography", "--inlier_matches", "--min_inliers", "4")
    for tag, r, n, cams in (("clean", rc, n_clean, cams_clean), ("30 % gated", rg, n_gated, cams_gated), ("30 % ungated", rp, n_plain, cams_plain),
                            ("30 % gated, --min_inliers 4", r4, n_four, cams_four)):
        fe = _focal_errors(cams, sc, clean["names"]) if cams else np.array([np.nan])
        print(f"run_ptz_ba {tag}: exit {r.returncode}, registered {n}, relative focal error median {np.median(fe):.3e} max {fe.max():.3e}")
    assert rg.returncode == 0, rg.stderr
    assert n_gated == n_clean, rg.stderr[-3000:]
    for c in cams_gated.values():
        assert all(np.isfinite(np.array(c[k], dtype=np.float64)).all() for k in ("K", "R", "t", "pos", "dist"))
    # the host estimator gives the same gated run
    rh, n_host, cams_host = _ba_run(dirty, str(tmp_path / "out_gated_host"), "--inlier_matches")
    assert rh.returncode == 0 and cams_host == cams_gated
