"""GPU test of run_ptz_reloc --match_descriptors --shortlist R on desc_match_util.chain_reloc's data (24 test images, 24 reference
images, test image q shares 96 features with reference q alone): with every reference listable the records are the --on_device
run's once n_shortlist is removed, with every option the flag composes with; --save_matches writes the blocks of the shortlisted
pairs; without the new flags the tool writes the bytes it wrote before."""
import json
import os
import subprocess

import pytest

import desc_match_util as du

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FLAG_SETS = {"plain": [], "multi_ref": ["--multi_ref", "2"],
             "all": ["--match_guided", "4", "--inlier_matches", "--trim_px", "2", "--uncertainty", "--multi_ref", "3"]}


def _run_tool(*args):
    return subprocess.run([os.path.join(ROOT, "ptz-calib_amd", "bin", "run_ptz_reloc"), *args], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def on_disk(pkg, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("reloc_shortlist_tool"))
    rb, _, _, paths = du.chain_reloc(pkg, root)
    args = ["--ref_images", paths["ref_images"], "--ref_features", paths["ref_features"], "--ref_params", paths["ref_params"],
            "--test_images", paths["test_images"], "--test_features", paths["test_features"]]
    return rb, paths, args, root


def _cameras(out):
    return json.load(open(os.path.join(out, "tests.json")))["cameras"]


@pytest.mark.parametrize("flags", list(FLAG_SETS))
def test_shortlist_of_every_reference_writes_the_on_device_records(on_disk, flags):
    rb, paths, args, root = on_disk
    n_ref = len(paths["ref_names"])
    out_d, out_s = os.path.join(root, flags + "_device"), os.path.join(root, flags + "_shortlist")
    sd, ss = os.path.join(root, flags + "_device.txt"), os.path.join(root, flags + "_shortlist.txt")
    rd = _run_tool(*args, "--match_descriptors", "--on_device", *FLAG_SETS[flags], "--output", out_d, "--save_matches", sd)
    rs = _run_tool(*args, "--match_descriptors", "--shortlist", str(n_ref), *FLAG_SETS[flags], "--output", out_s, "--save_matches", ss)
    assert rd.returncode == 0 and rs.returncode == 0, rd.stderr[-1500:] + rs.stderr[-1500:]
    want, got = _cameras(out_d), _cameras(out_s)
    assert list(got.keys()) == list(want.keys()) and len(want) == rb.n_query
    for k in got:
        assert 1 <= got[k].pop("n_shortlist") <= n_ref, k
        assert "n_shortlist" not in want[k]
    assert got == want
    # the blocks of the shortlisted pairs: the all-pairs run's blocks (a pair without matches has none in either file)
    assert open(ss, "rb").read() == open(sd, "rb").read() and os.path.getsize(ss) > 0


def test_short_list_records_and_flag_errors(on_disk):
    """R = 1 with 64 probes and 8 votes at least: the one reference a test image shares features with; the flags need each other"""
    rb, paths, args, root = on_disk
    out_d, out_1, s1 = os.path.join(root, "r1_device"), os.path.join(root, "r1"), os.path.join(root, "r1.txt")
    assert _run_tool(*args, "--match_descriptors", "--on_device", "--output", out_d).returncode == 0
    r1 = _run_tool(*args, "--match_descriptors", "--shortlist", "1", "--shortlist_probes", "64", "--shortlist_min_votes", "8", "--output", out_1,
                   "--save_matches", s1)
    assert r1.returncode == 0, r1.stderr[-1500:]
    want, got = _cameras(out_d), _cameras(out_1)
    for k in got:
        assert got[k].pop("n_shortlist") == 1
    assert got == want
    blocks = du.read_matches_file(s1)
    assert list(blocks.keys()) == [(paths["ref_names"][q], paths["test_names"][q]) for q in range(rb.n_query)]
    assert _run_tool(*args, "--shortlist", "4", "--output", out_1).returncode == 1                                          # needs --match_descriptors
    assert _run_tool(*args, "--match_descriptors", "--shortlist", "0", "--output", out_1).returncode == 1
    assert _run_tool(*args, "--match_descriptors", "--shortlist_probes", "64", "--output", out_1).returncode == 1           # needs --shortlist
    assert _run_tool(*args, "--match_descriptors", "--shortlist", "4", "--shortlist_probes", "0", "--output", out_1).returncode == 1
    assert _run_tool(*args, "--match_descriptors", "--shortlist", "4", "--shortlist_min_votes", "-1", "--output", out_1).returncode == 1


def test_without_the_flags_the_bytes_are_the_golden_runs(on_disk):
    rb, paths, args, root = on_disk
    out_f, out_m = os.path.join(root, "file"), os.path.join(root, "matched")
    assert _run_tool(*args, "--output", out_f).returncode == 0
    assert open(os.path.join(out_f, "tests.json"), "rb").read() == open(os.path.join(GOLDEN, "desc_chain_run_ptz_reloc.json"), "rb").read()
    assert _run_tool(*args, "--match_descriptors", "--output", out_m).returncode == 0
    assert list(_cameras(out_m).keys()) == list(_cameras(out_f).keys())
