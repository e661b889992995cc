"""Helper of test_gpu_landmark_shortlist.py::test_device_forms_and_stale_workspace (own process: torch first, then the library).

ptz_landmark_shortlist_device with device outputs on a stream returns the host form's arrays whatever bytes its workspace and its
outputs held before (0xFF among them); ptz_landmark_view_from_homes_device on those device lists returns the host form's view; a
device list with entries out of range gives the view of the entries in range."""
import os
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
import landmark_shortlist_util as lu  # noqa: E402
from test_gpu_landmark_shortlist import device_map, query_set  # noqa: E402

pkg = ge.load_package()
api = pkg.api
dev = torch.device("cuda:0")
n_ref, n_lm, R = 23, 1025, 4
desc, home = lu.make_map(n_lm, n_ref, 130, seed=21, empty=(3,))
refs, m = device_map(pkg, desc, home, n_ref)
qs, qp, qd, Q = query_set(pkg, desc, sizes=(300, 0, 64, 1, 129), seed=5)
n = len(qs)
o = dict(max_refs=R, n_probes=100, min_votes=1)
want = api.landmark_shortlist(m, Q, **o)
assert want["n_short"].max() == R and (want["votes"] > 0).sum() > 10
with api.landmark_view_from_homes(m, want["shortlist"]) as v:
    want_view = v.arrays()
lu.assert_equal(want_view, lu.view(home, want["shortlist"]), "host view")
ws_bytes = api.landmark_shortlist_workspace_bytes(m, Q, n, n_probes=100)
assert ws_bytes >= 4 * n * n_ref * (1 + 4)
st = torch.cuda.Stream(device=dev)
for fill in (0x7F, 0xFF):
    ws = torch.full((ws_bytes,), fill, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    sl = torch.full((n, R), 12345, dtype=torch.int32, device=dev)
    ns = torch.full((n,), 12345, dtype=torch.int32, device=dev)
    votes = torch.full((n, n_ref), 12345, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    api.landmark_shortlist_device(m, Q, n, sl, ns, ws, ws_bytes, d_votes=votes, stream=st.cuda_stream, **o)
    # the view from the device lists, on the stream that writes them: no synchronisation in between
    with api.landmark_view_from_homes(m, sl, device=True, n_query=n, max_refs=R, stream=st.cuda_stream) as v:
        view = v.arrays()
        assert v.kind == api.VIEW_HOMES
    st.synchronize()
    assert np.array_equal(sl.cpu().numpy(), want["shortlist"]) and np.array_equal(ns.cpu().numpy(), want["n_short"])
    assert np.array_equal(votes.cpu().numpy(), want["votes"])
    lu.assert_equal(view, want_view, "device view")
    print("landmark shortlist device ok: workspace of 0x%02x bytes, %d homes listed, %d landmarks in view" % (fill, int(ns.sum()), len(view["vis_lm"])))
# the device form ignores what the host form refuses
bad = np.array([[0, n_ref, 5, -7], [-1, -1, -1, -1], [2**31 - 1, 22, 22, 4]], dtype=np.int32)
dl = torch.tensor(bad, device=dev)
torch.cuda.synchronize()
with api.landmark_view_from_homes(m, dl, device=True, n_query=3, max_refs=4) as v:
    lu.assert_equal(v.arrays(), lu.view(home, np.where((bad >= 0) & (bad < n_ref), bad, -1)), "entries out of range")
try:
    api.landmark_shortlist_device(m, Q, n, sl, ns, ws, 256, stream=st.cuda_stream, **o)
    raise SystemExit("a workspace that is too small was accepted")
except api.PtzError as e:
    assert e.code == -1
print("landmark shortlist device ok: entries out of range ignored")
Q.close(); m.close(); refs.close()
