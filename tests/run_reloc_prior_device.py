"""Helper of test_gpu_reloc_prior.py::test_device_pointer_form_returns_the_host_forms_arrays (own process: torch first, then the
library).

ptz_reloc_prior_pairs_device with device inputs and outputs on a stream returns the host form's arrays whatever bytes its outputs
held before; a missing output is an argument error."""
import os
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
import reloc_prior_harness as ph  # noqa: E402
import reloc_prior_util as pu  # noqa: E402

api = ge.load_package().api
dev = torch.device("cuda:0")
n_ref, n, R = 65, 6, 4
cams = ph.make_cams(n_ref, 11, dist=True)
pri, wh = ph.make_priors(n, 61, away=(2,), dist=True)
Rr, Rq = ph.rotations(cams), ph.rotations(pri)
o = dict(factor_type=3, max_refs=R, min_overlap=12)
want = api.reloc_prior_pairs(cams, pri, wh, ref_R=Rr, prior_R=Rq, **o)
assert want["n_short"].max() == R and want["n_short"][2] == 0
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
ins = [up(cams), up(Rr), up(pri), up(Rq), up(wh)]
st = torch.cuda.Stream(device=dev)
for fill in (7, -1):
    sl, ns = torch.full((n, R), fill, dtype=torch.int32, device=dev), torch.full((n,), fill, dtype=torch.int32, device=dev)
    ov, Hs = torch.full((n, n_ref), fill, dtype=torch.int32, device=dev), torch.full((n, R, 9), float(fill), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    api.reloc_prior_pairs_device(n_ref, ins[0], ins[1], n, ins[2], ins[3], ins[4], sl, ns, ov, Hs, stream=st.cuda_stream, **o)
    st.synchronize()
    got = dict(shortlist=sl.cpu().numpy(), n_short=ns.cpu().numpy(), overlap=ov.cpu().numpy(), H_slot=Hs.cpu().numpy())
    pu.assert_equal(got, want)
    print("reloc prior device ok: outputs filled with %d before, %d references listed" % (fill, int(ns.sum())))
try:
    api.reloc_prior_pairs_device(n_ref, ins[0], ins[1], n, ins[2], ins[3], ins[4], sl, ns, None, Hs, stream=st.cuda_stream, **o)
    raise SystemExit("a missing output was accepted")
except api.PtzError as e:
    assert e.code == -1
print("reloc prior device ok: a missing output is refused")
