"""Helper of test_gpu_desc_guided_grid.py::test_equal_to_the_scan_kernel_on_the_rig (own process: torch first, then the library).

The 20-view rig with repeated descriptors, its 190 pairs, H and found from the first pass's matches through the project's host
estimator (desc_guided_util.pair_models), radius 4 and 40: the scan kernel and the grid kernel through the host-array entry points and,
with H and found in torch tensors on the device, through the device-pointer entry points.  All four results are equal arrays."""
import os
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as ge  # noqa: E402
import desc_guided_util as gu  # noqa: E402
import host_util as hu  # noqa: E402

pkg = ge.load_package()
dev = torch.device("cuda:0")
sc, tb, ptr, desc, kp, _ = gu.repeated_rig(pkg)
ia, ib = (x.astype(np.int32) for x in np.triu_indices(tb.n_img, 1))
assert len(ia) == 190
opt = dict(ratio=0.8, cross_check=1, min_matches=8)
n_out = []
with pkg.api.DescSet(ptr, desc, kp) as s:
    first = pkg.api.match_descriptors(s, s, ia, ib, **opt)
    H, found = gu.pair_models(hu.lib(), first, kp, ptr, kp, ptr, ia, ib, 4.0, 6)
    assert int(found.sum()) > 50
    dH, df = torch.from_numpy(H).to(dev).contiguous(), torch.from_numpy(found).to(dev).contiguous()
    torch.cuda.synchronize()  # the guided calls run on a stream of their own
    for radius in (4.0, 40.0):
        scan = pkg.api.match_descriptors_guided(s, s, ia, ib, H, found, radius, **opt)
        grid = pkg.api.match_descriptors_guided(s, s, ia, ib, H, found, radius, grid=True, **opt)
        scan_d = pkg.api.match_descriptors_guided(s, s, ia, ib, dH, df, radius, **opt)
        grid_d = pkg.api.match_descriptors_guided(s, s, ia, ib, dH, df, radius, grid=True, **opt)
        gu.assert_equal(grid, scan, ("host arrays", radius))
        gu.assert_equal(scan_d, scan, ("scan kernel, device pointers", radius))
        gu.assert_equal(grid_d, scan, ("device pointers", radius))
        assert len(scan["idx_a"]) > 1000 and (np.diff(scan["match_ptr"])[found != 1] == 0).all()
        n_out.append(len(scan["idx_a"]))
print("desc grid rig ok", len(ia), "pairs,", int(found.sum()), "models, matches at radius 4 and 40:", n_out)
