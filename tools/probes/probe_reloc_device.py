#!/usr/bin/env python3
"""Measurement of the relocalization assembly on the device (a probe, not a test; no threshold).

Online shape: 1000 queries x 2000 features against 200 references, D = 128, every (reference, query) pair matched once
(ptz_desc_match_pairs, the result resident on the device).  Then, in ONE process with alternating turns:
  host turn    what run_ptz_reloc --match_descriptors does today between the matcher and the cameras: download every match of every
               pair, pick the reference with the most matches per query on the host (first wins a tie), build the query CSR and the
               two cameras, upload and solve (ptz_krt_solve_batch);
  device turn  ptz_reloc_assemble_device on the matcher's own device pointers, ptz_krt_solve_batch_device on its outputs, one
               stream, no host round trip in between; only the cameras and the accept flags come back.
Both turns end with the same cameras (checked, K = 1).  Reports wall times (median over the turns), the device time of the assembly
for K = 1 and K = 4 between events on its stream, and the matcher's device time beside it.
Then the same comparison from the FEATURES on, matcher included, again alternating: api.Relocalizer.run (ptz_relocalizer_run: matcher,
assembly, solve, per-query results) against match_descriptors + the host turn above; and the relocalizer's own stage times.

usage: probe_reloc_device.py [--images 200] [--features 2000] [--queries 1000] [--dim 128] [--turns 5]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def features(rng, n_img, n_feat, D, base, base_xy, noise=12):
    """n_img images of n_feat features; half of every image's rows are noisy copies of rows of `base` at the pixels base_xy (plus a
    pixel of noise), so that there is something to accept; the rest uniform."""
    d = rng.integers(0, 256, (n_img * n_feat, D), dtype=np.uint8)
    xy = rng.uniform([0, 0], [1920, 1080], (n_img * n_feat, 2)).astype(np.float32)
    k = n_feat // 2
    for m in range(n_img):
        pick = rng.integers(0, len(base), k)
        d[m * n_feat:m * n_feat + k] = np.clip(base[pick].astype(np.int16) + rng.integers(-noise, noise + 1, (k, D)), 0, 255).astype(np.uint8)
        xy[m * n_feat:m * n_feat + k] = base_xy[pick] + rng.normal(0, 1.0, (k, 2)).astype(np.float32)
    return d, xy, (np.arange(n_img + 1) * n_feat).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--turns", type=int, default=5)
    a = ap.parse_args()
    pkg = ge.load_package()
    api = pkg.api
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    n_ref, nq = a.images, a.queries
    rig = pkg.synth.make_scene(0, n_ref, 20).cam_gt  # only the cameras matter
    base = rng.integers(0, 256, (4 * a.features, a.dim), dtype=np.uint8)
    base_xy = rng.uniform([100, 100], [1820, 980], (len(base), 2)).astype(np.float32)
    rd, rk, rp = features(rng, n_ref, a.features, a.dim, base, base_xy)
    qd, qk, qp = features(rng, nq, a.features, a.dim, base, base_xy)
    ia = np.tile(np.arange(n_ref, dtype=np.int32), nq)     # query-major, references ascending: the tool's pair order
    ib = np.repeat(np.arange(nq, dtype=np.int32), n_ref)
    qptr = (np.arange(nq + 1, dtype=np.int64) * n_ref)
    wh = np.tile(np.array([1920, 1080], dtype=np.int32), (nq, 1))
    R = api.reloc_ref_rotations(rig)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    out = dict(shape="online: %d queries against %d references" % (nq, n_ref), features=a.features, D=a.dim, pairs=int(len(ia)))
    with api.DescSet(rp, rd, rk) as refs, api.DescSet(qp, qd, qk) as tests:
        api.match_descriptors(refs, tests, ia, ib, resident=True, min_matches=8).close()  # warm-up
        m = api.match_descriptors(refs, tests, ia, ib, resident=True, min_matches=8)
        nm, npair = m.n_matches, len(ia)
        out.update(n_matches=int(nm), matcher_device_ms=m.device_ms)
        d_ptr, _, _, _, d_ua, d_ub = m.device_ptrs()
        d_pref, d_qptr, d_cams, d_R, d_wh = t(ia), t(qptr), t(rig), t(R), t(wh)
        wbytes = api.reloc_assemble_workspace_bytes(nq, nm)
        ws = torch.zeros(wbytes, dtype=torch.uint8, device=dev)
        optr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        oa, ob = torch.zeros((nm, 2), dtype=torch.float32, device=dev), torch.zeros((nm, 2), dtype=torch.float32, device=dev)
        osrc = torch.zeros(nm, dtype=torch.int32, device=dev)
        nsel = torch.zeros(nq, dtype=torch.int32, device=dev)
        cref, ccur = torch.zeros((nq, 15), dtype=torch.float64, device=dev), torch.zeros((nq, 15), dtype=torch.float64, device=dev)
        summ = torch.zeros(nq * 64, dtype=torch.uint8, device=dev)  # (sizeof(ptz_lm_summary) = 64)
        acc = torch.zeros(nq, dtype=torch.int32, device=dev)
        st = torch.cuda.Stream(device=dev)
        out["workspace_mib"] = wbytes / 2.0 ** 20

        def assemble(K, sel):
            api.reloc_assemble_device(nq, npair, nm, n_ref, d_ptr, d_ua, d_ub, d_pref, d_qptr, d_cams, d_R, d_wh, sel, nsel, optr, oa, ob, osrc,
                                      cref, ccur, ws, wbytes, factor_type=0, max_refs=K, stream=st.cuda_stream)

        sels = {K: torch.zeros((nq, K), dtype=torch.int32, device=dev) for K in (1, 4)}
        for K in (1, 4):  # device time of the assembly alone
            ms = []
            for r in range(a.turns + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                assemble(K, sels[K])
                e1.record(st)
                st.synchronize()
                if r:
                    ms.append(e0.elapsed_time(e1))
            out["assemble_device_ms_K%d" % K] = float(np.median(ms))
            out["assembled_matches_K%d" % K] = int(optr[-1])

        def host_turn():
            t0 = time.perf_counter()
            h = m.download()
            t1 = time.perf_counter()
            counts = np.diff(h["match_ptr"]).reshape(nq, n_ref)
            best = counts.argmax(axis=1)  # the first of equal maxima: FindBestMatch's tie
            use = counts[np.arange(nq), best] > 0
            pairs = (np.arange(nq) * n_ref + best)[use]
            idx = np.concatenate([np.arange(h["match_ptr"][p], h["match_ptr"][p + 1]) for p in pairs])
            cr = rig[best[use]]
            ci = cr.copy()
            ci[:, 1] = cr[:, 0]
            ci[:, 2], ci[:, 3] = 0.5 * wh[use, 0], 0.5 * wh[use, 1]
            rb = types.SimpleNamespace(n_query=int(use.sum()), match_ptr=np.concatenate([[0], np.cumsum(counts[np.arange(nq), best][use])]).astype(np.int64),
                                       uv_ref=h["uv_a"][idx], uv_cur=h["uv_b"][idx], cam_ref=cr, cam_init=ci, factor_type=0)
            t2 = time.perf_counter()
            cam, _, ok, _ = api.krt_solve_batch(rb)
            t3 = time.perf_counter()
            return (t3 - t0, t1 - t0, t2 - t1, t3 - t2), cam, ok, use

        def device_turn():
            t0 = time.perf_counter()
            assemble(1, sels[1])
            api.krt_solve_batch_device(nq, optr, oa, ob, cref, ccur, summ, acc, factor_type=0, stream=st.cuda_stream)
            st.synchronize()
            cam, ok = ccur.cpu().numpy(), acc.cpu().numpy()
            return time.perf_counter() - t0, cam, ok

        host_s, dev_s = [], []
        for r in range(a.turns + 1):
            hs, hcam, hok, use = host_turn()
            ds, dcam, dok = device_turn()
            if r:
                host_s.append(hs)
                dev_s.append(ds)
        same = bool(np.array_equal(hok, dok[use]) and np.array_equal(hcam[hok == 1], dcam[use][hok == 1]))
        hs = np.median(np.array(host_s), axis=0)
        out.update(host_turn_ms=1e3 * hs[0], host_download_ms=1e3 * hs[1], host_select_ms=1e3 * hs[2], host_upload_solve_ms=1e3 * hs[3],
                   device_turn_ms=1e3 * float(np.median(dev_s)), accepted=int(dok.sum()), same_cameras=same, turns=a.turns)
        m.close()
        # from the features on: the resident loop against today's sequence, the matcher in both
        with api.Relocalizer(refs, rig) as rl:
            full_h, full_d, stages = [], [], []
            for r in range(min(a.turns, 3) + 1):
                t0 = time.perf_counter()
                m = api.match_descriptors(refs, tests, ia, ib, resident=True, min_matches=8)
                _, hcam, hok, use = host_turn()
                m.close()
                t1 = time.perf_counter()
                got = rl.run(tests, wh, max_refs=1, match=dict(min_matches=8))
                t2 = time.perf_counter()
                if r:
                    full_h.append(t1 - t0)
                    full_d.append(t2 - t1)
                    stages.append(got["stage_ms"])
            same = bool(np.array_equal(hok, got["accepted"][use]) and np.array_equal(hcam[hok == 1], got["cam"][use][hok == 1]))
            out.update(sequence_with_matcher_ms=1e3 * float(np.median(full_h)), relocalizer_run_ms=1e3 * float(np.median(full_d)),
                       relocalizer_stage_ms=[float(x) for x in np.median(np.array(stages), axis=0)], relocalizer_same_cameras=same)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
