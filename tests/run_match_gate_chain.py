"""Helper of test_device_resident_chain_gate_then_solve (own process: torch first, then the library).

MatchGate.run_device and krt_solve_batch_device on one stream with nothing between them on the host; after ONE
synchronisation the results equal krt_solve_batch_gated's (which test_gated_solve_equals_composition_by_hand holds to the
composition by hand).  Two runs on the same gate and the same output tensors -- the second batch smaller, another factor type,
some queries without a chance -- so whatever the first run left in H, mask and the compacted arrays is still there: a leak
between runs would show."""
import ctypes as C
import os
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as ge  # noqa: E402
from test_gpu_match_gate import numpy_gate, outlier_batch  # noqa: E402

pkg = ge.load_package()
dev = torch.device("cuda:0")
MAXQ, MAXM = 96, 96 * 128


def t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)


gate = pkg.api.MatchGate(MAXQ, MAXM, 128)
d_H = torch.zeros((MAXQ, 3, 3), dtype=torch.float64, device=dev)
d_found = torch.full((MAXQ,), 7, dtype=torch.int32, device=dev)
d_mask = torch.zeros(MAXM, dtype=torch.uint8, device=dev)
d_optr = torch.zeros(MAXQ + 1, dtype=torch.int64, device=dev)
d_oa = torch.zeros((MAXM, 2), dtype=torch.float32, device=dev)
d_ob = torch.zeros((MAXM, 2), dtype=torch.float32, device=dev)
d_oi = torch.zeros(MAXM, dtype=torch.int32, device=dev)
st = torch.cuda.Stream()

for rb in (outlier_batch(pkg, 0, 0.3), outlier_batch(pkg, 1, 0.5, n_query=40, n_match=100, seed_id=9, lost=(0, 13, 39))):
    n = rb.n_query
    want_cam, want_summ, want_acc, want_ninl, want_mask, want_H, _ = pkg.api.krt_solve_batch_gated(rb)
    Hh, fh, mh, _ = pkg.api.find_homographies(rb.match_ptr, rb.uv_ref, rb.uv_cur)
    keep, out_ptr, out_index = numpy_gate(np.asarray(rb.match_ptr, np.int64), fh, mh, 0)
    d_ptr, d_ref, d_cur = t(rb.match_ptr, np.int64), t(rb.uv_ref, np.float32), t(rb.uv_cur, np.float32)
    d_cref, d_ccur = t(rb.cam_ref, np.float64), t(rb.cam_init, np.float64)
    d_sum = torch.zeros(n * C.sizeof(pkg.api.LmSummary), dtype=torch.uint8, device=dev)
    d_acc = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # the uploads and fills above ran on torch's own stream
    with torch.cuda.stream(st):
        gate.run_device(n, d_ptr, d_ref, d_cur, d_found, d_optr, d_oa, d_ob, d_H=d_H, d_mask=d_mask, d_out_index=d_oi,
                        stream=st.cuda_stream)
        pkg.api.krt_solve_batch_device(n, d_optr, d_oa, d_ob, d_cref, d_ccur, d_sum, d_acc, factor_type=rb.factor_type,
                                       stream=st.cuda_stream)
    st.synchronize()
    k = int(out_ptr[-1])
    found = d_found.cpu().numpy()[:n]
    assert np.array_equal(found, fh)
    assert np.array_equal(d_optr.cpu().numpy()[:n + 1], out_ptr) and np.array_equal(np.diff(out_ptr), want_ninl)
    assert np.array_equal(d_oi.cpu().numpy()[:k], out_index)
    assert d_oa.cpu().numpy()[:k].tobytes() == np.asarray(rb.uv_ref, np.float32)[keep].tobytes()
    assert d_ob.cpu().numpy()[:k].tobytes() == np.asarray(rb.uv_cur, np.float32)[keep].tobytes()
    ok = found == 1
    assert d_H.cpu().numpy()[:n][ok].tobytes() == Hh[ok].tobytes()
    ok_m = np.repeat(ok, np.diff(rb.match_ptr))
    assert np.array_equal(d_mask.cpu().numpy()[:len(mh)][ok_m], mh[ok_m])
    assert d_ccur.cpu().numpy().tobytes() == want_cam.tobytes()
    assert np.array_equal(d_acc.cpu().numpy(), want_acc)
    summ = (pkg.api.LmSummary * n).from_buffer_copy(d_sum.cpu().numpy().tobytes())
    assert [s.as_dict() for s in summ] == want_summ
    print("gate chain ok", n, "queries,", int(want_acc.sum()), "accepted,", k, "of", len(mh), "matches kept,", int((want_ninl == 0).sum()),
          "queries without inliers")
gate.close()
