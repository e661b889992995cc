"""GPU tests of run_ptz_reloc --match_descriptors --landmarks --device_tracks on the landmark tool test's data set: the map built
from device tracks has the landmarks and the tracks of the host route's (the "Landmark map:" line), the same test images are
registered, and every focal length and rotation agrees with the host route's within the project's parity bound of 1e-6 relative
(the landmark order differs, so the solve's summation order does); the flag without --landmarks exits 1; and without the flag the
tool writes the bytes of the landmark tool test's golden."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import desc_match_util as du
from test_gpu_run_ptz_reloc_landmarks import FLAG_SETS, GOLDEN, _cameras, _run_tool, on_disk  # noqa: F401  (on_disk: the data set's fixture)

pytestmark = pytest.mark.gpu


def test_device_tracks_give_the_host_routes_map_and_cameras(on_disk):  # noqa: F811
    sc, rig, refs, tests, names, args, root, ref_params, ref_names = on_disk
    outs, lines = {}, {}
    for tag, extra in (("host", []), ("device", ["--device_tracks"])):
        outs[tag] = os.path.join(root, "out_tracks_" + tag)
        r = _run_tool(*args, "--landmarks", *extra, "--output", outs[tag])
        assert r.returncode == 0, r.stderr[-1500:]
        found = re.findall(r"Landmark map: (\d+) landmarks from (\d+) tracks of (\d+) reference images", r.stderr)
        assert len(found) == 1, r.stderr[-1500:]
        lines[tag] = tuple(int(x) for x in found[0])
    assert lines["host"] == lines["device"] and lines["host"][0] > 1000
    host, dev = _cameras(outs["host"]), _cameras(outs["device"])
    assert sorted(host) == sorted(dev) and len(host) == 24  # the same accepted set
    for name in host:
        h, d = host[name], dev[name]
        assert h["n_landmarks"] == d["n_landmarks"] == lines["host"][0] and h["n_matches"] == d["n_matches"], name
        assert abs(d["K"][0] / h["K"][0] - 1) < 1e-6 and abs(d["K"][4] / h["K"][4] - 1) < 1e-6, name
        assert np.abs(np.array(d["R"]) - np.array(h["R"])).max() < 1e-6, name  # (entries of a rotation: relative to 1)


def test_the_flag_needs_landmarks(on_disk):  # noqa: F811
    sc, rig, refs, tests, names, args, root, ref_params, ref_names = on_disk
    out = os.path.join(root, "out_tracks_err")
    r = _run_tool(*args, "--device_tracks", "--output", out)
    assert r.returncode == 1 and "--landmarks" in r.stderr, (r.returncode, r.stderr[-300:])
    assert not os.path.exists(os.path.join(out, "tests.json"))


def test_without_the_flag_the_bytes_are_the_goldens(pkg, tmp_path):
    rb, _, _, paths = du.chain_reloc(pkg, str(tmp_path))
    args = ["--ref_images", paths["ref_images"], "--ref_features", paths["ref_features"], "--ref_params", paths["ref_params"],
            "--test_images", paths["test_images"], "--test_features", paths["test_features"], "--match_descriptors"]
    want = json.load(open(GOLDEN))
    for flags in FLAG_SETS:
        out = str(tmp_path / ("on_device_" + flags))
        r = _run_tool(*args, "--on_device", *FLAG_SETS[flags], "--output", out)
        assert r.returncode == 0, r.stderr[-1500:]
        assert hashlib.sha256(open(os.path.join(out, "tests.json"), "rb").read()).hexdigest() == want["on_device_" + flags], flags
