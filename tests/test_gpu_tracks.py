"""GPU tests of the device tracks (ptz_tracks_build / _from_matches / _build_device, ptz_landmark_map_create_from_tracks): every
comparison is array-equal against the numpy restatement of csrc/ptz_tracks.h (tracks_util.restate) on trk_ptr, trk_img, trk_feat,
trk_node, trk_uv and the four counts -- the reference-pinned fixtures, the small and degenerate tables, deep and wide components,
a component that is not a track, the order of the edges, the three forms of the entry point, and the landmark map built from them."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import host_util as hu
import tracks_util as tu
from tracks_util import SHAPES, edge_tables, golden_cases, random_graphs, shape_table

pytestmark = pytest.mark.gpu

LM = dict(max_num_iterations=200)
MATCH = dict(min_matches=8)


def arrays_of(t):
    ptr, img, feat, node, uv = t.download()
    return dict(trk_ptr=ptr, trk_img=img, trk_feat=feat, trk_node=node, trk_uv=uv, counts=t.counts())


def build(pkg, table, min_len):
    with pkg.api.tracks_build(min_len=min_len, **table) as t:
        got = arrays_of(t)
        assert t.n_tracks == len(got["trk_ptr"]) - 1 and t.n_views == len(got["trk_node"]) and t.device_ms >= 0
    return got


# ---- 1. the fixtures
def test_fixture_graphs_give_the_reference_tracks(pkg):
    n_track = n_rep = n_short = 0
    for k, (pairs, ml, want) in enumerate(random_graphs() + golden_cases()):
        tb = tu.table_of_pairs(pairs)
        got = build(pkg, tb, ml)
        ptr, img, feat, node = tu.canonical(want, tb["feat_ptr"])
        assert np.array_equal(got["trk_ptr"], ptr) and np.array_equal(got["trk_img"], img), k
        assert np.array_equal(got["trk_feat"], feat) and np.array_equal(got["trk_node"], node), k
        tu.assert_equal(got, tu.restate(min_len=ml, **tb), where=k)
        if k < 20:
            n_track, n_rep, n_short = n_track + len(ptr) - 1, n_rep + int(got["counts"][2]), n_short + int(got["counts"][3])
    assert (n_track, n_rep, n_short) == (605, 228, 608)


# ---- 2. small and degenerate tables
@pytest.mark.parametrize("name,table", edge_tables(), ids=[n for n, _ in edge_tables()])
def test_small_and_degenerate_tables(pkg, name, table):
    n_img = len(table["feat_ptr"]) - 1
    for ml in (2, 3, 4, max(n_img, 2), n_img + 1):
        tu.assert_equal(build(pkg, table, ml), tu.restate(min_len=ml, **table), where=(name, ml))


def test_min_len_below_two_and_indices_out_of_range(pkg):
    api = pkg.api
    tb = dict(edge_tables())["five-image chain"]
    for ml in (1, 0, -3):
        with pytest.raises(api.PtzError) as e:
            api.tracks_build(min_len=ml, **tb)
        assert e.value.code == -1
    bad_feat = dict(tb, idx_a=tb["idx_a"].copy())
    bad_feat["idx_a"][4] = 3   # a feature past its image's end
    bad_img = dict(tb, img_b=tb["img_b"].copy())
    bad_img["img_b"][3] = 5    # an image past the set's end
    neg = dict(tb, idx_b=tb["idx_b"].copy())
    neg["idx_b"][0] = -1
    for bad in (bad_feat, bad_img, neg):
        with pytest.raises(api.PtzError) as e:  # the host form refuses, before any device work
            api.tracks_build(min_len=2, **bad)
        assert e.value.code == -1


def test_device_form(pkg):
    """ptz_tracks_build_device on torch buffers and a torch stream: the small and degenerate tables with key points, an index out of
    range ignored where the host form refuses it, the order test's table twice on a workspace and outputs filled with 0xFF, and the
    rig's resident table with the set's key points.  Own process with torch initialised first (as
    test_gpu_landmark_map.py::test_device_form_on_the_cases)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "run_tracks_device.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    for what in ("tables", "out of range", "stale workspace", "rig"):
        assert "tracks device ok: " + what in r.stdout, r.stdout


# ---- 3. component shapes
@pytest.mark.parametrize("kind", SHAPES)
def test_component_shapes(pkg, kind):
    for n in (2, 63, 64, 65, 1023, 1024, 1025):
        got = build(pkg, shape_table(n, kind), 2)
        assert np.array_equal(got["trk_ptr"], [0, n]) and np.array_equal(got["trk_node"], np.arange(n)), (kind, n)
        assert np.array_equal(got["trk_img"], np.arange(n)) and not got["trk_feat"].any() and np.array_equal(got["counts"], [n, 1, 0, 0]), (kind, n)


def test_one_track_of_4096_views(pkg):
    for kind in ("chain_down", "star_top"):
        got = build(pkg, shape_table(4096, kind), 2)
        assert np.array_equal(got["trk_ptr"], [0, 4096]) and np.array_equal(got["trk_node"], np.arange(4096))
        assert np.array_equal(got["counts"], [4096, 1, 0, 0])


# ---- 4. a component that is not a track
def test_a_large_component_with_a_repeated_image_is_dropped(pkg):
    """Feature 0 of images 0 .. 4998 is one chain, closed through feature 1 of image 0: 5000 nodes over 4999 of the set's 7100
    images, so the repeat is no pigeonhole case -- the component is laid out and its one repeat shows only between two neighbours
    of its sorted views.  Beside it 300 good tracks of 3 to 7 views over images of their own."""
    rng = np.random.default_rng(4)
    pairs = [(i, i + 1, [(0, 0)]) for i in range(4998)] + [(4998, 0, [(0, 1)])]
    for t in range(300):
        first, length = 5000 + 7 * t, int(rng.integers(3, 8))
        pairs += [(first + k, first + k + 1, [(0, 0)]) for k in range(length - 1)]
    order = rng.permutation(len(pairs))
    tb = tu.table_of_pairs([pairs[k] for k in order], n_img=7100)
    tb["feat_ptr"] = np.concatenate([[0], np.cumsum([2] * 5000 + [1] * 2100)]).astype(np.int64)
    want = tu.restate(min_len=3, **tb)
    got = build(pkg, tb, 3)
    tu.assert_equal(got, want)
    assert len(got["trk_ptr"]) - 1 == 300 and np.array_equal(got["counts"], [5000 + int(got["trk_ptr"][-1]), 301, 1, 0])
    assert (got["trk_img"] >= 5000).all()


# ---- 5. order independence
def test_the_result_depends_on_the_set_of_edges_only(pkg):
    tb, tb2 = tu.order_tables()
    want = tu.restate(min_len=2, **tb)
    assert 3000 < len(tb["idx_a"]) < 6000 and len(want["trk_ptr"]) > 100 and want["counts"][2] > 0
    tu.assert_equal(build(pkg, tb, 2), want)
    tu.assert_equal(build(pkg, tb2, 2), want)


# ---- 6. the three forms agree
@pytest.fixture(scope="module")
def rig(pkg):
    """the 20-view x 100 rig's descriptors, resident, and the table of all 190 pairs, resident and downloaded"""
    sc = pkg.synth.make_scene(0, 20, 100)
    ptr, desc, kp = pkg.synth.make_descriptors(sc, D=128, noise=12, n_distractors=50, seed=1)
    ia, ib = (x.astype(np.int32) for x in np.triu_indices(20, 1))
    ds = pkg.api.DescSet(ptr, desc, kp)
    m = pkg.api.match_descriptors(ds, ds, ia, ib, resident=True)
    yield types.SimpleNamespace(ds=ds, m=m, table=m.download(uv=False), ia=ia, ib=ib, feat_ptr=np.asarray(ptr, dtype=np.int64), kp=np.asarray(kp, dtype=np.float32))
    m.close(); ds.close()


@pytest.mark.parametrize("min_len", [2, 4])
def test_the_three_forms_agree(pkg, rig, min_len):
    tb = dict(feat_ptr=rig.feat_ptr, img_a=rig.ia, img_b=rig.ib, match_ptr=rig.table["match_ptr"], idx_a=rig.table["idx_a"], idx_b=rig.table["idx_b"])
    want = tu.restate(min_len=min_len, kp=rig.kp, **tb)
    assert len(want["trk_ptr"]) > 10
    with pkg.api.tracks_from_matches(rig.ds, rig.m, rig.ia, rig.ib, min_len=min_len) as t:
        tu.assert_equal(arrays_of(t), want, where="resident")
        assert t.device_ms > 0
    host_form = build(pkg, tb, min_len)
    tu.assert_equal(host_form, want, keys=[k for k in tu.KEYS if k != "trk_uv"], where="host arrays")
    assert not host_form["trk_uv"].any()  # (no key points in that form)
    pairs = [(int(a), int(b), list(zip(tb["idx_a"][tb["match_ptr"][p]:tb["match_ptr"][p + 1]].tolist(), tb["idx_b"][tb["match_ptr"][p]:tb["match_ptr"][p + 1]].tolist())))
             for p, (a, b) in enumerate(zip(rig.ia, rig.ib))]
    ptr, img, feat, node = tu.canonical(hu.tracks_build(pairs, min_len), rig.feat_ptr)
    assert np.array_equal(want["trk_ptr"], ptr) and np.array_equal(want["trk_img"], img) and np.array_equal(want["trk_feat"], feat)
    assert np.array_equal(want["trk_node"], node)


# ---- 7. the map
@pytest.mark.parametrize("ft", [0, 1])
def test_the_map_from_device_tracks_is_the_map_from_their_download(pkg, ft):
    api = pkg.api
    cams = pkg.synth.make_scene(0, 20, 100).cam_gt.copy()
    if ft:
        cams[:, 10] = np.random.default_rng(100).uniform(-0.05, 0.05, len(cams))
    sc = pkg.synth_reloc.make_reloc_scene(cams, n_query=24, n_feat=600, visible_share=0.5, noise_px=0.5, factor_type=ft, seed=0)
    (rp, rd, rk), (qp, qd, qk) = pkg.synth_reloc.make_reloc_descriptors(sc, D=128, noise=12, n_distractors=50, seed=0)
    ia, ib = (x.astype(np.int32) for x in np.triu_indices(sc.n_ref, 1))
    keys = ("lm_track", "lm_ray", "lm_home", "lm_views", "lm_desc")
    with api.DescSet(rp, rd, rk) as refs, api.DescSet(qp, qd, qk) as tests, api.Relocalizer(refs, cams) as rl, \
            api.match_descriptors(refs, refs, ia, ib, resident=True, **MATCH) as m, api.tracks_from_matches(refs, m, ia, ib, min_len=2) as t:
        tp, ti, tf, tn, tuv = t.download()
        assert t.n_tracks > 1000
        tb = m.download(uv=False)
        pairs = [(int(a), int(b), list(zip(tb["idx_a"][tb["match_ptr"][p]:tb["match_ptr"][p + 1]].tolist(), tb["idx_b"][tb["match_ptr"][p]:tb["match_ptr"][p + 1]].tolist())))
                 for p, (a, b) in enumerate(zip(ia, ib))]
        hp, hi, hf, hn = tu.canonical(hu.tracks_build(pairs, 2), rp)
        assert np.array_equal(hp, tp) and np.array_equal(hi, ti) and np.array_equal(hf, tf) and np.array_equal(hn, tn)
        with api.LandmarkMap.from_tracks(refs, cams, t, factor_type=ft, min_views=2) as dmap, \
                api.LandmarkMap(refs, cams, tp, ti, tf, factor_type=ft, min_views=2) as hmap, \
                api.LandmarkMap(refs, cams, hp, hi, hf, factor_type=ft, min_views=2) as bmap:
            a, b, c = dmap.arrays(), hmap.arrays(), bmap.arrays()
            assert dmap.n_landmarks == hmap.n_landmarks == bmap.n_landmarks > 1000 and dmap.build_ms > 0
            for k in keys:
                assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
            r0 = rl.run(tests, sc.query_wh, factor_type=ft, landmarks=dmap, match=MATCH, **LM)
            r1 = rl.run(tests, sc.query_wh, factor_type=ft, landmarks=hmap, match=MATCH, **LM)
            for k in ("cam", "accepted", "sel_ref", "n_matches", "n_inliers"):
                assert np.array_equal(np.asarray(r0[k]), np.asarray(r1[k]), equal_nan=True), k
            assert r0["accepted"].sum() >= 20
    # a set of other extents than the tracks' is refused
    with api.DescSet(rp[:2], rd[:int(rp[1])], rk[:int(rp[1])]) as one, api.tracks_build(rp, ia[:0], ib[:0], np.zeros(1, np.int64), ia[:0], ib[:0]) as t0:
        with pytest.raises(api.PtzError) as e:
            api.LandmarkMap.from_tracks(one, cams[:1], t0)
        assert e.value.code == -1
