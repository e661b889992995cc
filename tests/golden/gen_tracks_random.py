#!/usr/bin/env python3
"""Fixture: what the reference's own track builder (oracle/_ref/ref_tracks: union_find.h + flat_pair_map.h of the reference,
compiled by oracle/Makefile where the reference tree lies) makes of 20 seeded random match graphs -- mostly consistent matches
plus noise, 4 to 19 images, minimum track length 2 to 4.  Stored so that the comparison of the oracle's track builder with the
reference's on these graphs needs no reference tree.  Regenerate with `make -C oracle ref && python tests/golden/gen_tracks_random.py`."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "tracks_reference_random.json")


def graphs():
    """The 20 graphs: [(pairs, min_track_length)], pairs = [(src, dst, [(queryIdx, trainIdx), ...]), ...]."""
    rng = np.random.default_rng(7)
    out = []
    for _ in range(20):
        n_img = int(rng.integers(4, 20))
        pairs = []
        for _ in range(int(rng.integers(1, 60))):
            i, j = rng.choice(n_img, 2, replace=False)
            k = int(rng.integers(0, 40))
            # mostly consistent matches (feature id = track id) plus noise
            ms = [(int(t), int(t if rng.random() < 0.9 else rng.integers(0, 50))) for t in rng.integers(0, 50, k)]
            pairs.append((int(i), int(j), ms))
        out.append((pairs, int(rng.integers(2, 5))))
    return out


def graph_hash(pairs, min_len):
    """sha256 of a graph, stored beside its tracks: a change of the generator (or of numpy's stream) shows as such."""
    return hashlib.sha256(json.dumps([pairs, min_len]).encode()).hexdigest()[:16]


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py as orc
    assert orc.ref_tracks_available(), "run `make -C oracle ref` where the reference tree lies first"
    cases = []
    for pairs, min_len in graphs():
        tracks = orc.ref_tracks_build(pairs, min_len)
        cases.append({"graph_sha256": graph_hash(pairs, min_len), "min_track_length": min_len,
                      "tracks": {str(t): {str(img): feat for img, feat in sorted(v.items())} for t, v in sorted(tracks.items())}})
    doc = {"_generator": "tests/golden/gen_tracks_random.py via oracle/_ref/ref_tracks "
                         "(reference src/core/union_find.h + flat_pair_map.h, Build/Filter/ExportToSTL of tracks.cc:19-113)",
           "cases": cases}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(f"{len(cases)} graphs, {sum(len(c['tracks']) for c in cases)} tracks -> {OUT}")


if __name__ == "__main__":
    main()
