"""Helper of test_gpu_landmark_visible.py::test_device_form_on_raw_rays (own process: torch first, then the library).  Every call
of ptz_landmark_visible_device here runs on a stream with the workspace and every output filled with a stale pattern (0x5A in every
byte) first, on RAW rays no map would hold (landmark_prior_util.make_case: a quarter pixel inside and outside each margin of query 0,
behind it, NaN, infinite, huge and zero components, then random ones), and is array-equal to the host harness:
n_lm in {0, 1, 63, 64, 65, 255, 256, 257, 1025, 2049} (the tile of a workgroup is 1024 landmarks, the step of a wave 64) x n_query in
{0, 1, 5, 257} (the scan of vis_ptr steps 64 queries at a time), factor types in turn; then a capacity that cuts: vis_ptr complete,
the first `capacity` entries written, the pattern behind them untouched."""
import os
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
import landmark_prior_util as lp  # noqa: E402

pkg = ge.load_package()
api = pkg.api
dev = torch.device("cuda:0")
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
STALE32 = np.frombuffer(b"\x5a" * 4, dtype=np.int32)[0]


def stale(shape, dtype):
    """a tensor whose every byte is 0x5A"""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((n,), 0x5A, dtype=torch.uint8, device=dev).view(dtype).reshape(shape)


def device_form(rays, cams, R, wh, ft, radius, capacity):
    n_lm, nq = len(rays), len(cams)
    st = torch.cuda.Stream(device=dev)
    cap = max(capacity, 1)
    ptr, lm, uv = stale((nq + 1,), torch.int64), stale((cap + 8,), torch.int32), stale((cap + 8, 2), torch.float32)
    wbytes = api.landmark_visible_workspace_bytes(n_lm, nq)
    assert wbytes > 0 and wbytes % 256 == 0
    ws = torch.full((wbytes,), 0x5A, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    d = [t(x if len(x) else np.zeros((1,) + x.shape[1:], dtype=x.dtype)) for x in (rays, cams, R, wh)]
    torch.cuda.synchronize()
    api.landmark_visible_device(n_lm, d[0], nq, d[1], d[2], d[3], ptr, lm, uv, capacity, ws, wbytes, factor_type=ft, radius_px=radius,
                                stream=st.cuda_stream)
    st.synchronize()
    return ptr.cpu().numpy(), lm.cpu().numpy(), uv.cpu().numpy()


def main():
    n_case = 0
    for i, n_lm in enumerate((0, 1, 63, 64, 65, 255, 256, 257, 1025, 2049)):
        for j, nq in enumerate((0, 1, 5, 257)):
            ft, radius = (i + j) % 4, (40.0, 7.5)[(i + j) % 2]
            rays, cams, wh = lp.make_case(n_lm, nq, ft, seed=10 * i + j, radius_px=radius)
            R = api.reloc_ref_rotations(cams) if nq else np.zeros((0, 9))
            want = lp.harness_visible(rays, cams, wh, ft, radius, prior_R=R)
            n = int(want["vis_ptr"][-1])
            ptr, lm, uv = device_form(rays, cams, R, wh, ft, radius, n)
            assert np.array_equal(ptr, want["vis_ptr"]), (n_lm, nq, "vis_ptr")
            assert np.array_equal(lm[:n], want["vis_lm"]) and np.array_equal(uv[:n].view(np.uint32), want["vis_uv"].view(np.uint32)), (n_lm, nq)
            assert (lm[max(n, 1):] == STALE32).all() and (uv[max(n, 1):].view(np.int32) == STALE32).all(), (n_lm, nq, "beyond the view")
            if n_lm >= 255 and nq >= 5:
                assert n > 50 and (np.diff(ptr) == 0).any(), (n_lm, nq, n)
            n_case += 1
    # a capacity that cuts inside a query, at 0, and one short of everything
    rays, cams, wh = lp.make_case(2049, 5, 0, seed=77)
    R = api.reloc_ref_rotations(cams)
    want = lp.harness_visible(rays, cams, wh, 0, 40.0, prior_R=R)
    n = int(want["vis_ptr"][-1])
    for cap in (0, 17, int(want["vis_ptr"][1]) + 3, n - 1):
        ptr, lm, uv = device_form(rays, cams, R, wh, 0, 40.0, cap)
        assert np.array_equal(ptr, want["vis_ptr"]) and np.array_equal(lm[:cap], want["vis_lm"][:cap]), cap
        assert np.array_equal(uv[:cap].view(np.uint32), want["vis_uv"][:cap].view(np.uint32)), cap
        assert (lm[cap:] == STALE32).all() and (uv[cap:].view(np.int32) == STALE32).all(), (cap, "written beyond the capacity")
        n_case += 1
    print("landmark visible device ok: %d cases" % n_case)


if __name__ == "__main__":
    main()
