"""CPU tests of the device tracks' contract (ptz-calib_amd/csrc/ptz_tracks.h): the numpy restatement (tracks_util.restate) against
the reference-pinned fixtures and the host TracksBuilder, canonicalised (tracks sorted by the node of their first view), and the host
instantiation of the header (cpu_harness/tracks_harness.cc) against the restatement, array for array."""
import numpy as np
import pytest

import host_util as hu
import tracks_util as tu
from tracks_util import SHAPES, edge_tables, golden_cases, random_graphs, shape_table


def restate_pairs(pairs, ml):
    tb = tu.table_of_pairs(pairs)
    return tb, tu.restate(min_len=ml, **tb)


def assert_canonical(got, want_dict, feat_ptr):
    ptr, img, feat, node = tu.canonical(want_dict, feat_ptr)
    assert np.array_equal(got["trk_ptr"], ptr) and np.array_equal(got["trk_img"], img)
    assert np.array_equal(got["trk_feat"], feat) and np.array_equal(got["trk_node"], node)


def test_restatement_gives_the_reference_fixtures():
    n_track = n_rep = n_short = 0
    for pairs, ml, want in random_graphs():
        tb, got = restate_pairs(pairs, ml)
        assert_canonical(got, want, tb["feat_ptr"])
        n_track += len(got["trk_ptr"]) - 1
        n_rep += int(got["counts"][2])
        n_short += int(got["counts"][3])
    assert (n_track, n_rep, n_short) == (605, 228, 608)
    for pairs, ml, want in golden_cases():
        tb, got = restate_pairs(pairs, ml)
        assert_canonical(got, want, tb["feat_ptr"])


def test_restatement_gives_the_host_builder():
    for pairs, ml, _ in random_graphs() + golden_cases():
        tb, got = restate_pairs(pairs, ml)
        assert_canonical(got, hu.tracks_build(pairs, ml), tb["feat_ptr"])


@pytest.mark.parametrize("name,table", edge_tables(), ids=[n for n, _ in edge_tables()])
def test_header_on_the_host_gives_the_restatement_edge_cases(name, table):
    n_img = len(table["feat_ptr"]) - 1
    kp = np.arange(2 * int(table["feat_ptr"][-1]), dtype=np.float32).reshape(-1, 2) * 0.5
    for ml in (2, 3, 4, max(n_img, 2), n_img + 1):
        want = tu.restate(min_len=ml, kp=kp, **table)
        for seed in (0, 1):
            tu.assert_equal(tu.host_build(min_len=ml, kp=kp, seed=seed, **table), want, where=(name, ml))


def test_header_on_the_host_gives_the_restatement_on_the_fixture_graphs():
    for k, (pairs, ml, _) in enumerate(random_graphs() + golden_cases()):
        tb, want = restate_pairs(pairs, ml)
        for seed in (0, 1, 2):
            tu.assert_equal(tu.host_build(min_len=ml, seed=seed, **tb), want, where=k)


def test_header_on_the_host_ignores_an_index_out_of_range():
    tb = dict(edge_tables())["five-image chain"]
    bad = dict(tb, idx_a=tb["idx_a"].copy(), img_b=tb["img_b"].copy())
    bad["idx_a"][4] = 3   # a feature past its image's end
    bad["img_b"][3] = 5   # an image past the set's end
    want = tu.restate(min_len=2, **bad)
    assert not np.array_equal(want["trk_ptr"], tu.restate(min_len=2, **tb)["trk_ptr"]) or not np.array_equal(
        want["trk_node"], tu.restate(min_len=2, **tb)["trk_node"])
    tu.assert_equal(tu.host_build(min_len=2, **bad), want)


@pytest.mark.parametrize("kind", SHAPES)
def test_header_on_the_host_component_shapes(kind):
    for n in (2, 63, 64, 65, 1023, 1024, 1025):
        tb = shape_table(n, kind)
        got = tu.host_build(min_len=2, seed=n, **tb)
        assert got is not None  # (None: a bounded loop reached its cap)
        assert np.array_equal(got["trk_ptr"], [0, n]) and np.array_equal(got["trk_node"], np.arange(n))
        assert np.array_equal(got["counts"], [n, 1, 0, 0])
