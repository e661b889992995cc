"""GPU tests of the batched RANSAC homography estimator (ptz_homography_ransac_batch, api.find_homographies): one launch over
a match table returns, for every pair, the host estimator's found flag, H and inlier mask bit for bit (host/homography.cc
through libptzcalib_host.so), whatever the batch the pair is in; the device path of LoadMatchesInfo and run_ptz_ba's
--gpu_homography change no output."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import homography_corpus as hc
import host_util as hu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(ptr, src, dst):
    return hc.run_per_pair(hu.lib().ptzh_find_homography, ptr, src, dst)


def _device(api, ptr, src, dst):
    H, found, mask, ms = api.find_homographies(ptr, src, dst)
    assert ms > 0
    return H, found, mask


def _assert_same(a, b):
    Ha, fa, ma = a
    Hb, fb, mb = b
    assert np.array_equal(fa, fb), np.flatnonzero(fa != fb)[:10]
    bad = np.flatnonzero((Ha.view(np.uint64) != Hb.view(np.uint64)).any(axis=(1, 2)))
    assert bad.size == 0, bad[:10]
    assert np.array_equal(ma, mb)


def test_corpus_bitwise_equal_to_host(pkg):
    ptr, src, dst = hc.corpus(seed=0, n_pairs=2000)
    _assert_same(_device(pkg.api, ptr, src, dst), _host(ptr, src, dst))


def _pick(ptr, src, dst, sel):
    """The pairs `sel` (in that order) as a table of their own."""
    return hc.pack([(src[ptr[p]:ptr[p + 1]], dst[ptr[p]:ptr[p + 1]]) for p in sel])


def test_c2_table_with_outliers_independent_of_batch(pkg):
    """The C2-shaped rig (200 views x 500 tracks, ~8 500 pairs) with 30 % outlier matches: equal to the host; every pair's
    result is the same in the whole table, in the reversed table and in three separate calls."""
    tb = hc.inject_outliers(pkg.synth.make_match_table(pkg.synth.make_scene(1, 200, 500)), 0.3, seed=1)
    ptr, src, dst = hc.table_arrays(tb)
    n = len(ptr) - 1
    assert n > 8000
    whole = _device(pkg.api, ptr, src, dst)
    _assert_same(whole, _host(ptr, src, dst))
    assert whole[1].sum() > 0.99 * n
    rev = np.arange(n)[::-1]
    r = _device(pkg.api, *_pick(ptr, src, dst, rev))
    _assert_same((r[0][::-1], r[1][::-1], np.concatenate([r[2][int(a):int(b)] for a, b in zip(*_rev_bounds(ptr))])), whole)
    for part in np.array_split(np.arange(n), 3):
        s = _device(pkg.api, *_pick(ptr, src, dst, part))
        _assert_same(s, (whole[0][part], whole[1][part], whole[2][ptr[part[0]]:ptr[part[-1] + 1]]))


def _rev_bounds(ptr):
    """Where pair p's mask lies in the reversed table, for p in the original order."""
    n = np.diff(ptr)[::-1]
    rptr = np.concatenate([[0], np.cumsum(n)])
    k = np.arange(len(n))[::-1]
    return rptr[k], rptr[k + 1]


def test_edge_cases_in_one_launch(pkg):
    """0, 3, 4 and 5 matches, a pair of 20 000 matches (far beyond the LDS), degenerate pairs (points on a line, one source
    point five times) and an 80 %-outlier pair whose bound stays above the cap (2000 iterations), in one call."""
    rng = np.random.default_rng(7)
    t = rng.uniform(0, 1, 60)
    line = np.c_[100 + 1500 * t, 200 + 600 * t].astype(np.float32)
    a5, b5 = hc.make_pair(rng, 5, 0.0)
    pairs = [hc.make_pair(rng, 0, 0.0), hc.make_pair(rng, 3, 0.0), hc.make_pair(rng, 4, 0.0), hc.make_pair(rng, 5, 0.0),
             hc.make_pair(rng, 20000, 0.3), (line, hc.make_pair(rng, 60, 0.0)[1]), (np.repeat(a5[:1], 5, axis=0), b5),
             hc.make_pair(rng, 500, 0.8), hc.make_pair(rng, 1200, 1.0)]
    ptr, src, dst = hc.pack(pairs)
    dev = _device(pkg.api, ptr, src, dst)
    _assert_same(dev, _host(ptr, src, dst))
    assert list(dev[1]) == [0, 0, 1, 1, 1, dev[1][5], 0, 1, 1]
    # the 80 % pair: about 20 % inliers keep the adaptive bound above 2000, so all 2000 hypotheses were drawn and scored
    bound = np.zeros(501, dtype=np.int32)
    assert pkg.api.lib().ptz_debug_homography_bounds(500, hc._p(bound)) == 0
    k = int(dev[2][ptr[7]:ptr[8]].sum())
    assert 60 < k < 160 and bound[k] > 2000
    # the 20 000-match pair keeps the host's quirk: its first accepted model (a few inliers) overflows the bound to INT_MIN and
    # ends the loop after that iteration -- reproduced, not fixed
    big = np.zeros(20001, dtype=np.int32)
    assert pkg.api.lib().ptz_debug_homography_bounds(20000, hc._p(big)) == 0
    assert big[4] == -2**31 and dev[2][ptr[4]:ptr[5]].sum() < 100


def _probe(cmd, a="", b=""):
    lib = hu.lib()
    lib.ptzh_io_probe.restype = C.c_void_p
    p = lib.ptzh_io_probe(cmd.encode(), a.encode(), b.encode())
    txt = C.string_at(p).decode()
    lib.ptzh_free(C.c_void_p(p))
    return json.loads(txt)


def test_load_matches_info_device_overload_equals_host_loader(pkg, tmp_path):
    """LoadMatchesInfo(..., device_id) on a rig written by dataset_io.write_rig with 30 % outlier matches: every cell of the
    N x N table (indices, matches, mask, counts, H bits, H_empty, confidence) equals the host loader's."""
    sc = pkg.synth.make_scene(2, 24, 150)
    tb = hc.inject_outliers(pkg.synth.make_match_table(sc), 0.3, seed=3)
    paths = pkg.dataset_io.write_rig(str(tmp_path), sc, tb)
    r = _probe("load_device", paths["images"], paths["features"])
    assert r["ok"] and r["loaded"] and r["identical"]
    assert r["table_cells"] == 24 * 24 and len(r["pairs"]) == tb.n_pairs and r["n_pairs_found"] > 0.9 * tb.n_pairs


def _run_tool(name, *args):
    exe = os.path.join(ROOT, "ptz-calib_amd", "bin", name)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)


def test_run_ptz_ba_gpu_homography_same_output(pkg, tmp_path):
    """run_ptz_ba --gpu_homography writes the byte-identical output JSON of the run without the flag."""
    sc = pkg.synth.add_annotations(pkg.synth.make_scene(1, 20, 100))
    tb = hc.inject_outliers(pkg.synth.make_match_table(sc), 0.05, seed=4)
    paths = pkg.dataset_io.write_rig(str(tmp_path), sc, tb, annotations=sc.obs3d)
    outs = []
    for flag in ([], ["--gpu_homography"]):
        out_dir = str(tmp_path / ("out_gpu" if flag else "out_host"))
        r = _run_tool("run_ptz_ba", "-i", paths["images"], "-f", paths["features"], "-a", paths["annotation"], "--output=" + out_dir, *flag)
        assert r.returncode == 0, r.stderr
        outs.append(open(os.path.join(out_dir, "rig0.json"), "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) > 1000
