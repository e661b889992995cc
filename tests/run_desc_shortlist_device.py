"""Helper of test_gpu_desc_shortlist.py::test_device_form_and_stale_workspace (own process: torch first, then the library).

ptz_desc_shortlist_device with device outputs on a stream returns the host form's arrays whatever bytes its workspace and its
outputs held before, with and without a device list of query images; a workspace that is too small is an argument error."""
import os
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from test_gpu_desc_shortlist import make_sets  # noqa: E402

pkg = ge.load_package()
api = pkg.api
dev = torch.device("cuda:0")
refs, rp, qs, qp = make_sets(13, 130)
n, n_ref, R = len(qs), len(refs), 6
o = dict(max_refs=R, n_probes=100, min_votes=2)
with api.DescSet(rp, np.concatenate(refs)) as Rs, api.DescSet(qp, np.concatenate(qs)) as Q:
    want = api.desc_shortlist(Rs, Q, **o)
    assert want["n_short"].max() > 1 and (want["votes"] > 0).sum() > 10
    ws_bytes = api.desc_shortlist_workspace_bytes(Rs, Q, n, n_probes=100)
    assert ws_bytes >= 4 * n * n_ref * (1 + 4)  # votes and four 32-probe slots of partial counts
    st = torch.cuda.Stream(device=dev)
    for fill in (0x7F, 0xFF):
        ws = torch.full((ws_bytes,), fill, dtype=torch.uint8, device=dev)
        assert ws.data_ptr() % 256 == 0
        sl = torch.full((n, R), 12345, dtype=torch.int32, device=dev)
        ns = torch.full((n,), 12345, dtype=torch.int32, device=dev)
        votes = torch.full((n, n_ref), 12345, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        api.desc_shortlist_device(Rs, Q, n, sl, ns, ws, ws_bytes, d_votes=votes, stream=st.cuda_stream, **o)
        st.synchronize()
        assert np.array_equal(sl.cpu().numpy(), want["shortlist"]) and np.array_equal(ns.cpu().numpy(), want["n_short"])
        assert np.array_equal(votes.cpu().numpy(), want["votes"])
        print("desc shortlist device ok: workspace of 0x%02x bytes, %d references listed" % (fill, int(ns.sum())))
    # a device list of images, no votes asked: the rows of those images
    pick = [8, 2, 2, 5]
    img = torch.tensor(pick, dtype=torch.int32, device=dev)
    sl = torch.zeros((4, R), dtype=torch.int32, device=dev)
    ns = torch.zeros(4, dtype=torch.int32, device=dev)
    ws = torch.full((api.desc_shortlist_workspace_bytes(Rs, Q, 4, n_probes=100),), 0x55, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    api.desc_shortlist_device(Rs, Q, 4, sl, ns, ws, ws.numel(), d_query_img=img, stream=st.cuda_stream, **o)
    st.synchronize()
    assert np.array_equal(sl.cpu().numpy(), want["shortlist"][pick]) and np.array_equal(ns.cpu().numpy(), want["n_short"][pick])
    try:
        api.desc_shortlist_device(Rs, Q, n, sl, ns, ws, 256, stream=st.cuda_stream, **o)
        raise SystemExit("a workspace that is too small was accepted")
    except api.PtzError as e:
        assert e.code == -1
    print("desc shortlist device ok: a device list of images")
