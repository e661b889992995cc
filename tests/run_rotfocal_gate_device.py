"""Helper of test_device_entry_equals_the_host_harness_and_writes_only_its_ranges (own process: torch first, then the library).

RotFocalGate.run_device on torch tensors, three runs on one gate and the SAME output tensors, each pre-filled with a pattern: after one
synchronisation every output equals the host harness's (tests/cpu_harness/rotfocal_harness.cc) and numpy's compaction of its mask, and
every byte outside the documented ranges -- model, H and mask of a query without a model, the compacted arrays beyond the kept count,
the rows beyond n_pair -- still holds the pattern.  The third run's offsets are partly unusable: those queries answer found = -1."""
import os
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as ge  # noqa: E402
import rotfocal_util as ru  # noqa: E402

pkg = ge.load_package()
dev = torch.device("cuda:0")
SIZES = (0, 1, 2, 3, 63, 64, 65, 257, 2048, 2049, 5000)
MAXQ, MAXM = 16, 12000
PAT = 0xAB


def t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)


gate = pkg.api.RotFocalGate(MAXQ, MAXM)
st = torch.cuda.Stream()
runs = [("virtual", ru.VIRTUAL, SIZES, 128, 0, True, None), ("real", ru.REAL, SIZES, 300, 6, False, None),
        ("bad offsets", ru.VIRTUAL, (40, 50, 30, 70), 128, 0, True, [0, 40, 13000, 50, 120])]
for tag, cam, sizes, iters, min_inl, with_opt, bad_ptr in runs:
    ptr, a, b, cr, cc, _ = ru.make_batch(sizes, seed=3, cam_a=cam)
    n = len(sizes)
    if bad_ptr is not None:  # query 1 ends beyond the gate's matches, query 2 ends before it begins; 0 and 3 are served, on disjoint ranges
        ptr = np.array(bad_ptr, dtype=np.int64)
        served = [0, 3]
        want = dict(found=np.full(n, -1, np.int32), model=np.full((n, 10), float(PAT)), H=np.full((n, 9), float(PAT)), mask=np.full(len(a), PAT, np.uint8))
        for q in served:
            s = slice(int(ptr[q]), int(ptr[q + 1]))
            w = ru.harness_batch(np.array([0, s.stop - s.start]), a[s], b[s], cr[q:q + 1], cc[q:q + 1], 4.0, iters, fill=PAT)
            want["found"][q], want["model"][q], want["H"][q] = w["found"][0], w["model"][0], w["H"][0]
            want["mask"][s] = w["mask"]
        cptr = ptr.copy()
        for q in range(n):  # the compaction sees empty ranges where found = -1
            if q not in served:
                want["found"][q] = -1
        out_ptr_w = np.zeros(n + 1, np.int64); keep = []
        for q in range(n):
            k = np.zeros(0, np.int64)
            if want["found"][q] == 1:
                k = ptr[q] + np.flatnonzero(want["mask"][ptr[q]:ptr[q + 1]] == 1)
                k = k if len(k) >= max(min_inl, 4) else k[:0]
            keep.append(k); out_ptr_w[q + 1] = out_ptr_w[q] + len(k)
        oi_w = np.concatenate(keep).astype(np.int32)
        oa_w, ob_w = a[oi_w], b[oi_w]
    else:
        want = ru.harness_batch(ptr, a, b, cr, cc, 4.0, iters, fill=PAT)
        out_ptr_w, oa_w, ob_w, oi_w = ru.compact(ptr, want["found"], want["mask"], a, b, min_inl)
    nm = len(a)
    d_ptr, d_a, d_b, d_cr, d_cc = t(ptr, np.int64), t(a, np.float32), t(b, np.float32), t(cr, np.float64), t(cc, np.float64)
    d_model = torch.full((MAXQ, 10), float(PAT), dtype=torch.float64, device=dev)
    d_H = torch.full((MAXQ, 9), float(PAT), dtype=torch.float64, device=dev)
    d_found = torch.full((MAXQ,), 7, dtype=torch.int32, device=dev)
    d_mask = torch.full((MAXM,), PAT, dtype=torch.uint8, device=dev)
    d_optr = torch.full((MAXQ + 1,), -9, dtype=torch.int64, device=dev)
    d_oa = torch.full((MAXM, 2), -3.0, dtype=torch.float32, device=dev)
    d_ob = torch.full((MAXM, 2), -3.0, dtype=torch.float32, device=dev)
    d_oi = torch.full((MAXM,), -5, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # the uploads and fills above ran on torch's own stream
    with torch.cuda.stream(st):
        gate.run_device(n, d_ptr, d_a, d_b, d_cr, d_cc, d_found, d_optr, d_oa, d_ob, d_model=d_model if with_opt else None,
                        d_H=d_H if with_opt else None, d_mask=d_mask if with_opt else None, d_out_index=d_oi if with_opt else None,
                        thresh=4.0, min_inliers=min_inl, iters=iters, stream=st.cuda_stream)
    st.synchronize()
    k = int(out_ptr_w[-1])
    found, optr = d_found.cpu().numpy(), d_optr.cpu().numpy()
    assert np.array_equal(found[:n], want["found"]) and (found[n:] == 7).all()
    assert np.array_equal(optr[:n + 1], out_ptr_w) and (optr[n + 1:] == -9).all()
    oa, ob = d_oa.cpu().numpy(), d_ob.cpu().numpy()
    assert oa[:k].tobytes() == oa_w.tobytes() and ob[:k].tobytes() == ob_w.tobytes() and (oa[k:] == -3.0).all() and (ob[k:] == -3.0).all()
    model, H, mask, oi = d_model.cpu().numpy(), d_H.cpu().numpy(), d_mask.cpu().numpy(), d_oi.cpu().numpy()
    if with_opt:
        assert model[:n].tobytes() == want["model"].tobytes() and (model[n:] == float(PAT)).all()
        assert H[:n].tobytes() == want["H"].tobytes() and (H[n:] == float(PAT)).all()
        assert np.array_equal(mask[:nm], want["mask"]) and (mask[nm:] == PAT).all()
        assert np.array_equal(oi[:k], oi_w) and (oi[k:] == -5).all()
    else:  # optional outputs not asked for: the tensors were not passed and hold their pattern
        assert (model == float(PAT)).all() and (H == float(PAT)).all() and (mask == PAT).all() and (oi == -5).all()
    print("rotfocal device entry ok:", tag, n, "queries,", int((found[:n] == 1).sum()), "with a model,", int((found[:n] == -1).sum()), "not served,", k, "of", nm,
          "matches kept")
gate.close()
