"""Helper of test_gpu_desc_match.py::test_device_pointers_feed_the_gate (own process: torch first, then the library).

The matcher's resident CSR (match_ptr, uv_a, uv_b on the device) goes into MatchGate.run_device as it is; the gate's outputs equal
what gate_matches gives on the downloaded arrays."""
import os
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
dev = torch.device("cuda:0")
sc = pkg.synth.make_scene(0, 20, 100)
ptr, desc, kp = pkg.synth.make_descriptors(sc, D=128, noise=12, n_distractors=50, seed=3)
ia = np.arange(0, 19, dtype=np.int32)
ib = ia + 1
with pkg.api.DescSet(ptr, desc, kp) as s:
    m = pkg.api.match_descriptors(s, s, ia, ib, resident=True, min_matches=8)
    host = m.download()
    n, nm = len(ia), m.n_matches
    assert nm > 0
    pair_of = np.repeat(np.arange(n), np.diff(host["match_ptr"]))
    assert np.array_equal(host["uv_a"], kp[ptr[ia[pair_of]] + host["idx_a"]]) and np.array_equal(host["uv_b"], kp[ptr[ib[pair_of]] + host["idx_b"]])
    want = pkg.api.gate_matches(host["match_ptr"], host["uv_a"], host["uv_b"], ransac_thresh=4.0, max_pair_matches=1024)
    d_ptr, _, _, _, d_ua, d_ub = m.device_ptrs()
    found = torch.zeros(n, dtype=torch.int32, device=dev)
    out_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    oa = torch.zeros((nm, 2), dtype=torch.float32, device=dev)
    ob = torch.zeros((nm, 2), dtype=torch.float32, device=dev)
    oi = torch.zeros(nm, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with pkg.api.MatchGate(n, nm, 1024) as g:
        g.run_device(n, d_ptr, d_ua, d_ub, found, out_ptr, oa, ob, d_out_index=oi, ransac_thresh=4.0)
        torch.cuda.synchronize()
    m.close()
k = int(out_ptr[-1])
assert np.array_equal(found.cpu().numpy(), want["found"]) and np.array_equal(out_ptr.cpu().numpy(), want["out_ptr"])
assert k == len(want["out_index"]) and k > 0
assert np.array_equal(oi.cpu().numpy()[:k], want["out_index"])
assert np.array_equal(oa.cpu().numpy()[:k], want["out_uv_a"]) and np.array_equal(ob.cpu().numpy()[:k], want["out_uv_b"])
print("desc gate ok", n, "pairs,", nm, "matches,", k, "kept by the gate")
