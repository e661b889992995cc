"""What ptz_ba_batch_create / ptz_ba_batch_create_views build and what a solve of it returns, case by case, as bits: the batch's
structure hash (ptz_debug_batch_structure_hash), every field of every ptz_lm_summary, and a SHA-256 of the returned cam, ray and
T_l_w bytes.  One case per way through the constructor: the four factor types, 2D-3D observations, shared intrinsics, the batch
sizes at which the launch-shape ladder, the Cholesky form, the look-ahead and the number of scene groups change, the structure and
ordering switches (set in this process between two creates, as the tests do), and view batches with their sort and wide paths.
Run it on two builds (PTZCALIB_LIB picks the library) and compare the files: a refactor of the constructor leaves every case
identical.  A comparison, not a test.

    python tools/probes/probe_ba_create_bits.py --out head.json
    python tools/probes/probe_ba_create_bits.py --compare a.json b.json [c.json ...]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as ge  # noqa: E402


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def solve_bits(pkg, batch, views=None):
    """views: (cams, rays) of a ViewBatch, whose rays have the extents of the whole rigs."""
    out = dict(structure_hash="%016x" % pkg.api.structure_hash(batch))
    if views is None:
        batch.set_state()
    else:
        batch.set_state(cams=views[0], rays=views[1])
    out["summaries"] = batch.solve()
    if views is None:
        cams, rays = batch.get_state()
        out["state_sha256"] = sha(np.concatenate(cams), np.concatenate(rays), batch.last_tlw)
    else:
        n_ray = sum(len(r) for r in views[1])
        cam = np.zeros((int(sum(batch.n_cams)), 15)); ray = np.zeros((n_ray, 3)); tlw = np.zeros((batch.n, 6))
        rc = pkg.api.lib().ptz_ba_batch_get_state(batch.handle, pkg.api._p(cam), pkg.api._p(ray), pkg.api._p(tlw))
        assert rc == 0, rc
        out["state_sha256"] = sha(cam, ray, tlw)
    return out


def run(pkg):
    api, synth = pkg.api, pkg.synth
    scene = lambda seed, **kw: synth.make_scene(seed, 20, 100, **kw)  # the smoke size
    cases = {}

    def batch_case(name, scenes, env=None):
        for k, v in (env or {}).items():
            os.environ[k] = v
        try:
            b = api.BaBatch(scenes)
            cases[name] = solve_bits(pkg, b)
            b.close()
        finally:
            for k in env or {}:
                del os.environ[k]

    for t, tname in enumerate(("PTZRay", "PTZRayDist", "PTZRayFxfyDist", "PTZRayDistDisp")):
        batch_case("n1_" + tname, [scene(0, factor_type=t)])
    batch_case("n1_obs3d", [synth.add_annotations(scene(1))])
    batch_case("n1_shared_intrinsics", [scene(6, factor_type=2, n_intrinsics_groups=3)])
    batch_case("n9", [scene(i) for i in range(9)])     # second ladder shape, left-looking, look-ahead
    batch_case("n33", [scene(i) for i in range(33)])   # two groups, ahead = 3, 1024-ray workgroups
    three = [scene(i) for i in range(3)]
    for env in ({"PTZ_BA_GPU_STRUCT": "0"}, {"PTZ_BA_GPU_STRUCT_CHECK": "1"}, {"PTZ_BA_ORDER": "natural"}, {"PTZ_BA_ORDER": "flat"},
                {"PTZ_BA_DENSE_CHOL": "1"}, {"PTZ_BA_SCHUR_W": "1"}, {"PTZ_BA_BACKSOLVE_HOST_LIST": "0"}):
        (k, v), = env.items()
        batch_case("n3_%s=%s" % (k, v), three, env)

    # three views of one resident rig
    sc = synth.make_scene(1, 40, 120)
    rig = api.Rig.from_scene(sc)
    images = [[0, 1], list(range(0, 40, 3)), list(range(5, 33))]
    probs = [api.view_problem(sc, im) for im in images]
    rays = []
    for p in probs:
        full = np.zeros((sc.n_ray, 3)); full[:p.n_ray] = p.ray_init
        rays.append(full)
    for env in ({}, {"PTZ_BA_VIEW_BLOCK_SORT": "0"}, {"PTZ_BA_DEBUG_VIEW_WIDE": "1"}):
        for k, v in env.items():
            os.environ[k] = v
        try:
            vb = api.ViewBatch([rig] * 3, images)
            cases["views3" + "".join("_%s=%s" % kv for kv in env.items())] = solve_bits(pkg, vb, ([p.cam_init for p in probs], rays))
            vb.close()
        finally:
            for k in env:
                del os.environ[k]
    rig.close()
    return cases


def compare(paths):
    runs = [json.load(open(p))["cases"] for p in paths]
    bad = 0
    for name in runs[0]:
        same = all(r.get(name) == runs[0][name] for r in runs[1:])
        bad += not same
        print("%-40s %s" % (name, "identical" if same else "DIFFERS"))
    print("%d of %d cases differ between %s" % (bad, len(runs[0]), ", ".join(paths)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs="+")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare))
    pkg = ge.load_package()
    cases = run(pkg)
    text = json.dumps(dict(version=pkg.api.version(), cases=cases), indent=1, sort_keys=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print("%d cases" % len(cases))
    for name, c in cases.items():
        print("%-40s %s %s iterations %s" % (name, c["structure_hash"], c["state_sha256"][:16], [s["num_iterations"] for s in c["summaries"]]))


if __name__ == "__main__":
    main()
