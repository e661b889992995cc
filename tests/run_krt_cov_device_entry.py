"""Helper of test_gpu_krt_covariance.py::test_device_form_equals_host_form_bit_for_bit (own process: torch first, then the
library, as run_krt_device_entry.py): the same batch through ptz_krt_covariance_batch and through
ptz_krt_covariance_batch_device enqueued behind ptz_krt_solve_batch_device on one stream, with no host round trip."""
import ctypes as C
import os
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
with_points = len(sys.argv) > 1 and sys.argv[1] == "1"
FT = 1
rb = pkg.synth.make_reloc_batch(48, 96, seed_id=8, factor_type=FT)
a, b = int(rb.match_ptr[3]), int(rb.match_ptr[4])
rb.uv_cur[a:b] = rb.uv_cur[a:b][::-1]  # scrambled matches: query 3 is rejected by the solve, its covariance is skipped
if with_points:
    rb = pkg.synth.add_reloc_points(rb, n_pt=9)
n, nf = rb.n_query, pkg.api.krt_free_dim(FT)
SENT = -12345.0
# host form: solve, then covariance of what the solve returned
want_cam, _, want_acc, _ = pkg.api.krt_solve_batch(rb)
want_cov, want_s0, want_st, _ = pkg.api.krt_covariance_batch(rb, want_cam, accepted=want_acc, cov=np.full((n, nf, nf), SENT),
                                                             sigma0=np.full(n, SENT))
assert want_acc[3] == 0 and want_st[3] == pkg.api.COV_SKIPPED and want_acc.sum() == n - 1
dev = torch.device("cuda:0")


def t(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)


d_ptr, d_ref, d_cur = t(rb.match_ptr, np.int64), t(rb.uv_ref, np.float32), t(rb.uv_cur, np.float32)
d_cref, d_ccur = t(rb.cam_ref, np.float64), t(rb.cam_init, np.float64)
d_sum = torch.zeros(n * C.sizeof(pkg.api.LmSummary), dtype=torch.uint8, device=dev)
d_acc = torch.full((n,), -1, dtype=torch.int32, device=dev)
d_cov = torch.full((n, nf, nf), SENT, dtype=torch.float64, device=dev)
d_s0 = torch.full((n,), SENT, dtype=torch.float64, device=dev)
d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
kw = {}
if with_points:
    kw = dict(d_point_ptr=t(rb.point_ptr, np.int64), d_pts2d=t(rb.pts2d, np.float32), d_pts3d=t(rb.pts3d, np.float64))
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    pkg.api.krt_solve_batch_device(n, d_ptr, d_ref, d_cur, d_cref, d_ccur, d_sum, d_acc, factor_type=FT, stream=st.cuda_stream, **kw)
    pkg.api.krt_covariance_batch_device(n, d_ptr, d_ref, d_cur, d_cref, d_ccur, d_cov, d_s0, d_st, factor_type=FT, d_accepted=d_acc,
                                        stream=st.cuda_stream, **kw)
st.synchronize()
assert np.array_equal(d_acc.cpu().numpy(), want_acc)
assert np.array_equal(d_ccur.cpu().numpy(), want_cam)
assert np.array_equal(d_st.cpu().numpy(), want_st)
assert np.array_equal(d_cov.cpu().numpy().view(np.uint64), want_cov.view(np.uint64))
assert np.array_equal(d_s0.cpu().numpy().view(np.uint64), want_s0.view(np.uint64))
assert (want_cov[3] == SENT).all() and want_s0[3] == SENT  # untouched in both forms
print("covariance device entry ok", int((want_st == 0).sum()), "of", n, "computed")
