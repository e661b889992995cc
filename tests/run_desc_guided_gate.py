"""Helper of test_gpu_desc_guided.py::test_device_h_from_the_gate_equals_the_host_pointer_call (own process: torch first, then the
library).

The first pass's resident CSR goes through MatchGate.run_device; the H and found it leaves ON THE DEVICE go into
ptz_desc_match_pairs_guided_device as they are.  The result equals the host-pointer call on the downloaded H and found, and the
restatement's guided pass under them."""
import os
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as ge  # noqa: E402
import desc_guided_util as gu  # noqa: E402

pkg = ge.load_package()
dev = torch.device("cuda:0")
sc = pkg.synth.make_scene(0, 20, 100)
ptr, desc, kp = pkg.synth.make_repeated_descriptors(sc, seed=3, **gu.REPEAT)
ia = np.concatenate([np.arange(0, 19), np.arange(0, 18)]).astype(np.int32)
ib = np.concatenate([np.arange(1, 20), np.arange(2, 20)]).astype(np.int32)
n = len(ia)
with pkg.api.DescSet(ptr, desc, kp) as s:
    m = pkg.api.match_descriptors(s, s, ia, ib, resident=True, min_matches=8)
    nm = m.n_matches
    assert nm > 0
    d_ptr, _, _, _, d_ua, d_ub = m.device_ptrs()
    found = torch.zeros(n, dtype=torch.int32, device=dev)
    H = torch.eye(3, dtype=torch.float64, device=dev).reshape(1, 9).repeat(n, 1).contiguous()
    out_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    oa = torch.zeros((max(nm, 1), 2), dtype=torch.float32, device=dev)
    ob = torch.zeros((max(nm, 1), 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with pkg.api.MatchGate(n, nm, 1024) as g:
        g.run_device(n, d_ptr, d_ua, d_ub, found, out_ptr, oa, ob, d_H=H, ransac_thresh=4.0, min_inliers=6)
        torch.cuda.synchronize()  # the guided call runs on a stream of its own
        got = pkg.api.match_descriptors_guided(s, s, ia, ib, H, found, 4.0, min_matches=8)
    m.close()
    hH, hf = H.cpu().numpy(), found.cpu().numpy()
    host = pkg.api.match_descriptors_guided(s, s, ia, ib, hH, hf, 4.0, min_matches=8)
want = gu.match_pairs_guided(desc, ptr, kp, desc, ptr, kp, ia, ib, hH, hf, 4.0, min_matches=8)
gu.assert_equal(got, host, "device pointers against host pointers")
gu.assert_equal(got, want, "device against the restatement")
assert 0 < int((hf == 1).sum()) and len(got["idx_a"]) > 0 and (np.diff(got["match_ptr"])[hf != 1] == 0).all()
print("desc guided gate ok", n, "pairs,", int((hf == 1).sum()), "models,", nm, "first-pass matches,", len(got["idx_a"]), "guided")
