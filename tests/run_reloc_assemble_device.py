"""Helper of test_gpu_reloc_assemble.py::test_device_form_on_the_matchers_pointers (own process: torch first, then the library).

The matcher's resident CSR of every (reference, query) pair (match_ptr, uv_a, uv_b on the device) goes into
ptz_reloc_assemble_device as it is, on a stream, without a host round trip; the outputs equal what the host form gives on the
downloaded arrays, for K = 1 and K = 4."""
import os
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
api = pkg.api
dev = torch.device("cuda:0")
rig = pkg.synth.make_scene(0, 20, 100).cam_gt.copy()
rig[:, 10] = np.random.default_rng(1).uniform(-0.05, 0.05, len(rig))
nq, n_ref = 6, len(rig)
sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=nq, n_feat=120, visible_share=0.5, noise_px=0.5, factor_type=1, seed=4)
(rp, rd, rk), (qp, qd, qk) = pkg.synth_reloc.make_reloc_descriptors(sc, D=64, noise=8, n_distractors=20, seed=2)
ia = np.tile(np.arange(n_ref, dtype=np.int32), nq)       # query-major, references ascending: the tool's pair order
ib = np.repeat(np.arange(nq, dtype=np.int32), n_ref)
R = api.reloc_ref_rotations(rig)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
with api.DescSet(rp, rd, rk) as refs, api.DescSet(qp, qd, qk) as tests:
    m = api.match_descriptors(refs, tests, ia, ib, resident=True, min_matches=8)
    host = m.download()
    nm, npair = m.n_matches, len(ia)
    assert nm > 0 and (np.diff(host["match_ptr"]).reshape(nq, n_ref) > 0).sum(axis=1).min() >= 2
    d_ptr, _, _, _, d_ua, d_ub = m.device_ptrs()
    d_pref, d_qptr, d_cams, d_R, d_wh = t(ia), t(sc.query_ptr), t(rig), t(R), t(sc.query_wh)
    st = torch.cuda.Stream(device=dev)
    for K in (1, 4):
        want = api.reloc_assemble(host["match_ptr"], host["uv_a"], host["uv_b"], ia, sc.query_ptr, rig, sc.query_wh, factor_type=1, max_refs=K, ref_R=R)
        sel = torch.zeros((nq, K), dtype=torch.int32, device=dev)
        nsel = torch.zeros(nq, dtype=torch.int32, device=dev)
        optr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        oa = torch.zeros((nm, 2), dtype=torch.float32, device=dev)
        ob = torch.zeros((nm, 2), dtype=torch.float32, device=dev)
        osrc = torch.zeros(nm, dtype=torch.int32, device=dev)
        cref = torch.zeros((nq, 15), dtype=torch.float64, device=dev)
        ccur = torch.zeros((nq, 15), dtype=torch.float64, device=dev)
        wbytes = api.reloc_assemble_workspace_bytes(nq, nm)
        ws = torch.zeros(wbytes, dtype=torch.uint8, device=dev)
        assert ws.data_ptr() % 256 == 0
        torch.cuda.synchronize()
        api.reloc_assemble_device(nq, npair, nm, n_ref, d_ptr, d_ua, d_ub, d_pref, d_qptr, d_cams, d_R, d_wh, sel, nsel, optr, oa, ob, osrc, cref,
                                  ccur, ws, wbytes, factor_type=1, max_refs=K, stream=st.cuda_stream)
        st.synchronize()
        k = int(optr[-1])
        got = dict(sel_pair=sel.cpu().numpy(), n_sel=nsel.cpu().numpy(), match_ptr=optr.cpu().numpy(), uv_ref=oa.cpu().numpy()[:k],
                   uv_cur=ob.cpu().numpy()[:k], src=osrc.cpu().numpy()[:k], cam_ref=cref.cpu().numpy(), cam_init=ccur.cpu().numpy())
        for key, v in got.items():
            assert np.array_equal(v, want[key]), (K, key)
        assert k > 0 and (K == 1 or k > int(np.diff(host["match_ptr"]).reshape(nq, n_ref).max(axis=1).sum()))
        print("reloc assemble device ok: K = %d, %d of %d matches kept" % (K, k, nm))
    m.close()
