#!/usr/bin/env python3
"""Measurement of the descriptor matcher (a probe, not a test; no threshold).

Offline shape: 200 images x 2000 features, D = 128, all 19 900 unordered pairs, both directions (cross_check) -- 2.04e13
multiply-accumulates.  Online shape: 1000 queries x 2000 features against 200 references.  Reports the device time of
ptz_desc_match_pairs (minimum and median of 7 runs after a warm-up) beside two floors:
  matrix-core floor  the multiply-accumulates at the dense I8 rate (twice BF16, about 5 POPS);
  epilogue floor     the vector instructions of the top-2 update: VALU_PER_ELEMENT per output element, counted in the compiled
                     D = 128 kernel's inner loop (69 vector instructions per step of 8 elements per lane: accumulator reads, the
                     shift and subtract that form the key, compare / max / select / min, the addresses of the prefetch), at 256 CUs x 4 SIMDs x 16 lanes per clock and 2.4 GHz.
and, for context, the one-thread time of the host restatement (tests/cpu_harness/desc_match_harness.cc) on a sample of the pairs.

usage: probe_desc_match.py [--images 200] [--features 2000] [--queries 1000] [--runs 7] [--host_sample 0.01] [--host_only] [--no_host]
Prints one JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

I8_OPS_PER_S = 5.0e15          # dense I8, 2 ops per multiply-accumulate
VALU_PER_ELEMENT = 69 / 8      # see above: counted in the assembly of k_desc_top2<2, false>, the inner loop's v_* other than the MFMAs
                               # (profiles/NOTES_desc_sweep.md); recount when the kernel or ptz_desc_sweep.h changes
VALU_LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9


def descriptors(rng, n_img, n_feat, D, base=None, noise=12):
    """n_img images of n_feat features; with `base` half of every image's rows are noisy copies of rows of base (so there is
    something to accept), the rest uniform."""
    d = rng.integers(0, 256, (n_img * n_feat, D), dtype=np.uint8)
    if base is not None:
        k = n_feat // 2
        for m in range(n_img):
            src = base[rng.integers(0, len(base), k)].astype(np.int16)
            d[m * n_feat:m * n_feat + k] = np.clip(src + rng.integers(-noise, noise + 1, (k, D)), 0, 255).astype(np.uint8)
    return d, (np.arange(n_img + 1) * n_feat).astype(np.int64)


def host_seconds(desc_a, ptr_a, desc_b, ptr_b, ia, ib, sample, rng):
    h = C.CDLL(os.path.join(ROOT, "tests", "cpu_harness", "libdesc_match_harness.so"))
    h.h_desc_match_pair.restype = C.c_int64
    n = max(1, int(round(len(ia) * sample)))
    pick = rng.permutation(len(ia))[:n]
    D = desc_a.shape[1]
    t0 = time.perf_counter()
    for p in pick:
        a = np.ascontiguousarray(desc_a[ptr_a[ia[p]]:ptr_a[ia[p] + 1]])
        b = np.ascontiguousarray(desc_b[ptr_b[ib[p]]:ptr_b[ib[p] + 1]])
        o = [np.zeros(len(a) + 1, dtype=np.int32) for _ in range(3)]
        h.h_desc_match_pair(a.ctypes.data_as(C.c_void_p), len(a), b.ctypes.data_as(C.c_void_p), len(b), D, C.c_double(0.8), 0, 1, 8,
                            C.c_uint64(1), 1, None, None, *[x.ctypes.data_as(C.c_void_p) for x in o])
    dt = time.perf_counter() - t0
    return n, dt


def measure(pkg, tag, sa, sb, ia, ib, n_feat, D, runs, host):
    macs = 2.0 * len(ia) * n_feat * n_feat * D  # both directions
    elements = macs / D
    out = dict(shape=tag, pairs=int(len(ia)), features=n_feat, D=D, macs=macs, mfma_floor_ms=1e3 * 2 * macs / I8_OPS_PER_S,
               epilogue_floor_ms=1e3 * elements * VALU_PER_ELEMENT / VALU_LANE_OPS_PER_S, valu_per_element=VALU_PER_ELEMENT)
    if sa is not None:
        ms, n_match, chunks = [], 0, 0
        for r in range(runs + 1):
            m = pkg.api.match_descriptors(sa, sb, ia, ib, resident=True, min_matches=8)
            if r:
                ms.append(m.device_ms)
            n_match, chunks = m.n_matches, m.n_chunks
            m.close()
        out.update(device_ms_min=min(ms), device_ms_median=float(np.median(ms)), n_matches=n_match, n_chunks=chunks,
                   fraction_of_mfma_floor=out["mfma_floor_ms"] / min(ms), fraction_of_epilogue_floor=out["epilogue_floor_ms"] / min(ms),
                   pairs_per_s=len(ia) / (min(ms) * 1e-3))
    if host is not None:
        n, dt = host
        out.update(host_pairs=n, host_s=dt, host_one_thread_s_for_all=dt / n * len(ia))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--host_sample", type=float, default=0.01)
    ap.add_argument("--host_only", action="store_true")
    ap.add_argument("--no_host", action="store_true")
    a = ap.parse_args()
    pkg = ge.load_package()
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (4 * a.features, a.dim), dtype=np.uint8)
    ref, rptr = descriptors(rng, a.images, a.features, a.dim, base)
    ia, ib = np.triu_indices(a.images, k=1)
    ia, ib = ia.astype(np.int32), ib.astype(np.int32)
    host = None if a.no_host else host_seconds(ref, rptr, ref, rptr, ia, ib, a.host_sample, rng)
    sr = None if a.host_only else pkg.api.DescSet(rptr, ref)
    measure(pkg, "offline: all pairs of %d images" % a.images, sr, sr, ia, ib, a.features, a.dim, a.runs, host)
    qry, qptr = descriptors(rng, a.queries, a.features, a.dim, base)
    qa = np.repeat(np.arange(a.images, dtype=np.int32), a.queries)       # reference image
    qb = np.tile(np.arange(a.queries, dtype=np.int32), a.images)         # query image
    host = None if a.no_host else host_seconds(ref, rptr, qry, qptr, qa, qb, a.host_sample * 0.1, rng)  # (ten times the pairs: a tenth of the sample)
    sq = None if a.host_only else pkg.api.DescSet(qptr, qry)
    measure(pkg, "online: %d queries against %d references" % (a.queries, a.images), sr, sq, qa, qb, a.features, a.dim, a.runs, host)


if __name__ == "__main__":
    main()
