"""Helper of test_gpu_krt_residuals.py::test_device_forms_equal_the_host_forms_bit_for_bit (own process: torch first, then the
library, as run_krt_cov_device_entry.py): the same batch through ptz_krt_residuals_batch and through
ptz_krt_residuals_batch_device enqueued behind ptz_krt_solve_batch_device on one stream; then through ptz_krt_solve_batch_trimmed
and ptz_krt_solve_batch_trimmed_device on that stream.  No host round trip in the device forms."""
import ctypes as C
import os
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as ge  # noqa: E402
import krt_trim_util as tu  # noqa: E402

pkg = ge.load_package()
api = pkg.api
FT = 1
SENT = -12345.0
b, wrong = tu.contaminated_batch(FT, 0.1, "displaced")
b = tu.sub_batch(b, list(range(b.n_query)))
a0, a1 = int(b.match_ptr[3]), int(b.match_ptr[4])
b.uv_cur[a0:a1] = b.uv_cur[a0:a1][::-1]  # scrambled matches: query 3 is rejected by the plain solve, its report is skipped
n, nm = b.n_query, int(b.match_ptr[-1])
dev = torch.device("cuda:0")


def t(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- the report: host form on what the host solve returned
want_cam, _, want_acc, _ = api.krt_solve_batch(b)
assert want_acc[3] == 0 and want_acc.sum() == n - 1
poison = dict(err_px=np.full(nm, SENT), rms=np.full(n, SENT), max=np.full(n, SENT), median=np.full(n, SENT), rms3d=np.full(n, SENT),
              count=np.full(n, -77, dtype=np.int32))
want = api.krt_residuals_batch(b, want_cam, accepted=want_acc, out=poison)
d_ptr, d_ref, d_cur = t(b.match_ptr, np.int64), t(b.uv_ref, np.float32), t(b.uv_cur, np.float32)
d_cref, d_ccur = t(b.cam_ref, np.float64), t(b.cam_init, np.float64)
d_sum = torch.zeros(n * C.sizeof(api.LmSummary), dtype=torch.uint8, device=dev)
d_acc = torch.full((n,), -1, dtype=torch.int32, device=dev)
d_err = torch.full((nm,), SENT, dtype=torch.float64, device=dev)
d_stat = {k: torch.full((n,), SENT, dtype=torch.float64, device=dev) for k in ("rms", "max", "median", "rms3d")}
d_cnt = torch.full((n,), -77, dtype=torch.int32, device=dev)
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    api.krt_solve_batch_device(n, d_ptr, d_ref, d_cur, d_cref, d_ccur, d_sum, d_acc, factor_type=FT, stream=st.cuda_stream)
    api.krt_residuals_batch_device(n, d_ptr, d_ref, d_cur, d_cref, d_ccur, factor_type=FT, d_accepted=d_acc, d_err_px=d_err, d_rms=d_stat["rms"],
                                   d_max=d_stat["max"], d_median=d_stat["median"], d_count=d_cnt, d_rms3d=d_stat["rms3d"], stream=st.cuda_stream)
st.synchronize()
assert np.array_equal(d_acc.cpu().numpy(), want_acc) and np.array_equal(bits(d_ccur.cpu().numpy()), bits(want_cam))
assert np.array_equal(bits(d_err.cpu().numpy()), bits(want["err_px"])) and np.array_equal(d_cnt.cpu().numpy(), want["count"])
for k in d_stat:
    assert np.array_equal(bits(d_stat[k].cpu().numpy()), bits(want[k])), k
assert (want["err_px"][a0:a1] == SENT).all() and want["count"][3] == -77  # untouched in both forms
# a median without err_px: refused before any launch
try:
    api.krt_residuals_batch_device(n, d_ptr, d_ref, d_cur, d_cref, d_ccur, factor_type=FT, d_median=d_stat["median"], stream=st.cuda_stream)
    raise SystemExit("d_median without d_err_px was accepted")
except api.PtzError as e:
    assert e.code == -1

# ---- the trimmed solve: host form, then the device form on the stream
mask = np.ones(nm, dtype=np.uint8)
mask[int(b.match_ptr[5]):int(b.match_ptr[6]):2] = 0  # query 5: half a universe
hc, hs, ha, hk, hr, _ = api.krt_solve_batch_trimmed(b, match_mask=mask)
assert ha.sum() >= n - 1 and hk.sum() < mask.sum() and max(r["rounds"] for r in hr) > 1
d_ccur2 = t(b.cam_init, np.float64)
d_sum2 = torch.zeros(n * C.sizeof(api.LmSummary), dtype=torch.uint8, device=dev)
d_acc2 = torch.full((n,), -1, dtype=torch.int32, device=dev)
d_kept = torch.full((nm,), 9, dtype=torch.uint8, device=dev)
d_rep = torch.zeros(n * C.sizeof(api.KrtTrimReport), dtype=torch.uint8, device=dev)
wbytes = api.krt_trim_workspace_bytes(n, nm)
d_work = torch.empty(wbytes + 256, dtype=torch.uint8, device=dev)
w_addr = (d_work.data_ptr() + 255) & ~255
with torch.cuda.stream(st):
    api.krt_solve_batch_trimmed_device(n, nm, d_ptr, d_ref, d_cur, d_cref, d_ccur2, d_sum2, d_acc2, w_addr, wbytes, factor_type=FT,
                                       d_match_mask=t(mask, np.uint8), d_kept=d_kept, d_report=d_rep, stream=st.cuda_stream)
st.synchronize()
assert np.array_equal(d_acc2.cpu().numpy(), ha) and np.array_equal(bits(d_ccur2.cpu().numpy()), bits(hc))
assert np.array_equal(d_kept.cpu().numpy(), hk)
got_sum = (api.LmSummary * n).from_buffer_copy(d_sum2.cpu().numpy().tobytes())
got_rep = (api.KrtTrimReport * n).from_buffer_copy(d_rep.cpu().numpy().tobytes())
for q in range(n):
    assert repr(got_sum[q].as_dict()) == repr(hs[q]), q
    assert repr(got_rep[q].as_dict()) == repr(hr[q]), q
print("residual and trimmed device entries ok", int(ha.sum()), "of", n, "accepted,", int(hk.sum()), "of", nm, "matches kept")
