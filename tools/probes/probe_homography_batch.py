"""Probe (not a test): the pair homographies of a C2-shaped match table (synth.make_scene(1, 200, 500)) at 0, 30 and 50 %
outlier matches -- the host estimator in a serial one-thread loop (ptzh_find_homography per pair, as LoadMatchesInfo runs it)
against one ptz_homography_ransac_batch call (wall time and device_ms).  Checks that both give the same bits.
Usage: probe_homography_batch.py [outlier fractions, default 0 0.3 0.5]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import __graft_entry__ as ge
import homography_corpus as hc
import host_util as hu

pkg = ge.load_package()
fracs = [float(x) for x in sys.argv[1:]] or [0.0, 0.3, 0.5]
base = pkg.synth.make_match_table(pkg.synth.make_scene(1, 200, 500))
pkg.api.find_homographies(*hc.table_arrays(base)[:3])  # warm-up: context, code object, memory pool
for frac in fracs:
    tb = pkg.synth.make_match_table(pkg.synth.make_scene(1, 200, 500))
    if frac > 0:
        hc.inject_outliers(tb, frac, seed=1)
    ptr, src, dst = hc.table_arrays(tb)
    t = time.perf_counter(); Hh, fh, mh = hc.run_per_pair(hu.lib().ptzh_find_homography, ptr, src, dst); host_s = time.perf_counter() - t
    t = time.perf_counter(); Hd, fd, md, ms = pkg.api.find_homographies(ptr, src, dst); dev_s = time.perf_counter() - t
    same = bool(np.array_equal(fh, fd) and np.array_equal(Hh.view(np.uint64), Hd.view(np.uint64)) and np.array_equal(mh, md))
    print(json.dumps(dict(outliers=frac, pairs=len(ptr) - 1, matches=int(ptr[-1]), host_serial_ms=round(1e3 * host_s, 1),
                          device_call_ms=round(1e3 * dev_s, 2), device_ms=round(ms, 2), speedup_wall=round(host_s / dev_s, 1),
                          found=int(fd.sum()), bit_identical=same)), flush=True)
