"""CPU tests of the RANSAC inlier gating of matches: the host-gated LoadInlierMatchesInfo against the table Python builds from
the ungated loader and the host estimator's masks, the argument checks of the new entries (no device needed), and the bound
table a ptz_match_gate holds.  Every equality is bitwise: the feature selects and moves data, it computes nothing new."""
import ctypes as C
import json

import numpy as np
import pytest

import homography_corpus as hc
import host_util as hu

EINVAL, EUNSUPPORTED, ELIMIT = -1, -4, -5


def _probe(cmd, a="", b=""):
    lib = hu.lib()
    lib.ptzh_io_probe.restype = C.c_void_p
    p = lib.ptzh_io_probe(cmd.encode(), a.encode(), b.encode())
    txt = C.string_at(p).decode()
    lib.ptzh_free(C.c_void_p(p))
    return json.loads(txt)


def expected_gated_cells(tb, ungated_pairs, n_img, min_inliers=0):
    """The gated table from the public pieces: the ungated loader's cells (`load` probe) and ptzh_find_homography's masks.
    A pair passes with a model and at least max(min_inliers, 4) mask ones; it keeps the matches with mask byte 1 in their order."""
    ptr, src, dst = hc.table_arrays(tb)
    _, found, mask = hc.run_per_pair(hu.lib().ptzh_find_homography, ptr, src, dst)
    plain = {(p["src"], p["dst"]): p for p in ungated_pairs}
    cells = {}
    for k in range(tb.n_pairs):
        s, d = int(tb.src[k]), int(tb.dst[k])
        a, b = int(ptr[k]), int(ptr[k + 1])
        m = mask[a:b].astype(bool)
        passes = found[k] == 1 and m.sum() >= max(min_inliers, 4)
        keep = m if passes else np.zeros(b - a, dtype=bool)
        n = int(keep.sum())
        cells[s * n_img + d] = dict(
            src=s, dst=d, matches=[[float(q), float(t)] for q, t in zip(tb.q[a:b][keep], tb.t[a:b][keep])], mask_ones=n, mask_len=n,
            num_inliers=n, H=plain[(s, d)]["H"], H_empty=plain[(s, d)]["H_empty"],
            confidence=float(np.float32(1.0) if n >= 100 else np.float32(n) / np.float32(100)))
        assert plain[(s, d)]["H_empty"] == (found[k] != 1)
    return cells, found, mask


@pytest.mark.parametrize("min_inliers", [0, 6])
def test_host_gated_loader_equals_hand_filtered_table(pkg, tmp_path, min_inliers):
    """LoadInlierMatchesInfo (host estimator) on a written rig with 30 % outlier matches: every cell is the ungated loader's
    cell with `matches` filtered by the host estimator's mask (H, H_empty, indices computed on all matches; mask all ones,
    num_inliers and confidence of the kept count).  min_inliers = 0 is the plain rule (four), 6 what the tools ask for."""
    sc = pkg.synth.make_scene(2, 12, 120)
    tb = hc.inject_outliers(pkg.synth.make_match_table(sc), 0.3)
    paths = pkg.dataset_io.write_rig(str(tmp_path), sc, tb)
    plain = _probe("load", paths["images"], paths["features"])
    got = _probe("load_inliers:%d" % min_inliers, paths["images"], paths["features"])
    assert plain["ok"] and got["ok"] and got["table_cells"] == 12 * 12
    want, found, mask = expected_gated_cells(tb, plain["pairs"], 12, min_inliers)
    cells = {c["cell"]: {k: v for k, v in c.items() if k != "cell"} for c in got["cells"]}
    assert sorted(cells) == sorted(want)
    for c in want:
        assert cells[c] == want[c], c
    # the gate did something: outliers left, most true matches stayed
    kept = sum(c["num_inliers"] for c in cells.values())
    assert 0.5 * len(mask) < kept < 0.8 * len(mask) and kept <= int(mask.sum())


def test_new_entries_check_their_arguments_without_a_device(pkg):
    lib = pkg.api.lib()
    gate = C.c_void_p()
    create = lambda pairs, matches, per, dev=0: lib.ptz_match_gate_create(pairs, C.c_int64(matches), per, dev, C.byref(gate))
    assert lib.ptz_match_gate_create(8, C.c_int64(64), 16, 0, None) == EINVAL
    assert create(0, 64, 16) == EINVAL and create(-1, 64, 16) == EINVAL
    assert create(8, -1, 16) == EINVAL and create(8, 64, -1) == EINVAL and create(8, 64, 16, -1) == EINVAL
    assert create(8, 64, 4097) == ELIMIT and create(8, 2**31, 16) == ELIMIT
    assert gate.value is None
    # run_device / run: no gate
    one = np.zeros(1, dtype=np.int64)
    assert lib.ptz_match_gate_run_device(None, 0, None, None, None, C.c_double(4.0), 0, None, None, None, hc._p(one), None, None, None,
                                         None) == EINVAL
    assert lib.ptz_match_gate_run(None, 0, None, None, None, C.c_double(4.0), 0, None, None, None, hc._p(one), None, None, None,
                                  None) == EINVAL
    # the fused entry: the list of ptz_homography_ransac_batch, min_inliers, the solve's arrays
    rb = pkg.synth.make_reloc_batch(3, 16, seed_id=1, factor_type=0)
    n = rb.n_query
    ptr = np.ascontiguousarray(rb.match_ptr, dtype=np.int64)
    uvr, uvc = np.ascontiguousarray(rb.uv_ref, np.float32), np.ascontiguousarray(rb.uv_cur, np.float32)
    cref, ccur = np.ascontiguousarray(rb.cam_ref, np.float64), np.array(rb.cam_init, dtype=np.float64)
    summ = (pkg.api.LmSummary * n)()
    acc, ninl = np.zeros(n, np.int32), np.zeros(n, np.int32)
    p = hc._p

    def call(n=n, ptr=ptr, uvr=uvr, uvc=uvc, cref=cref, ccur=ccur, ftype=0, thr=4.0, min_inl=0, summ=summ, acc=acc, ninl=ninl):
        return lib.ptz_krt_solve_batch_gated(n, p(ptr), p(uvr), p(uvc), p(cref), p(ccur), ftype, C.c_double(100.0), C.c_double(thr),
                                             min_inl, None, summ, p(acc), p(ninl), None, None, None)

    assert call(n=-1) == EINVAL and call(ptr=None) == EINVAL and call(uvr=None) == EINVAL and call(uvc=None) == EINVAL
    assert call(thr=0.0) == EINVAL and call(thr=float("nan")) == EINVAL and call(thr=float("inf")) == EINVAL
    assert call(min_inl=-1) == EINVAL
    assert call(ptr=ptr + 1) == EINVAL                      # match_ptr[0] != 0
    bad = ptr.copy(); bad[1] = bad[2] + 1
    assert call(ptr=bad) == EINVAL                          # decreasing offsets
    assert call(cref=None) == EINVAL and call(ccur=None) == EINVAL and call(summ=None) == EINVAL
    assert call(acc=None) == EINVAL and call(ninl=None) == EINVAL
    assert call(ftype=7) == EUNSUPPORTED
    assert call(n=0) == 0                                   # nothing to do, no device touched
    assert np.array_equal(ccur, rb.cam_init)


def test_gate_bound_table_is_the_estimators_bounds_size_by_size(pkg):
    """A gate of max_pair_matches = 64 holds ptz_debug_homography_bounds(n) for every n in 5 .. 64, size n at the closed-form
    offset n (n + 1) / 2 - 15; sizes below 5 have no table (the estimator never reads one for them)."""
    tab, off = pkg.api.match_gate_table(64)
    assert len(off) == 65 and len(tab) == sum(n + 1 for n in range(5, 65))
    at = 0
    for n in range(5, 65):
        assert off[n] == at == n * (n + 1) // 2 - 15
        want = np.zeros(n + 1, dtype=np.int32)
        assert pkg.api.lib().ptz_debug_homography_bounds(n, hc._p(want)) == 0
        assert np.array_equal(tab[at:at + n + 1], want), n
        at += n + 1
    assert np.array_equal(off[:5], np.zeros(5, dtype=np.int64))
    for m in (0, 4):
        t, o = pkg.api.match_gate_table(m)
        assert len(t) == 0 and len(o) == m + 1
    n_len = C.c_int64()
    assert pkg.api.lib().ptz_debug_match_gate_table(4097, None, C.byref(n_len), None) == ELIMIT
    assert pkg.api.lib().ptz_debug_match_gate_table(-1, None, C.byref(n_len), None) == EINVAL
