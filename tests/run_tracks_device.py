"""Helper of test_gpu_tracks.py::test_device_form (own process: torch first, then the library).  Every call of
ptz_tracks_build_device here runs on a torch stream, on torch buffers, array-equal to the numpy restatement (tracks_util.restate):

`tables`: the small and degenerate tables of tracks_util.edge_tables with key points, min_len in {2, 3, 4, n_img, n_img + 1};
`out of range`: a feature past its image's end, an image past the set's end and a negative index -- the host form refuses each
  (PTZ_EINVAL), the device form ignores the edge;
`stale workspace`: the order test's permuted table twice, the workspace and every output filled with 0xFF first;
`rig`: the resident table of the 20-view x 100 rig through ptz_desc_matches_device_ptrs, with the set's key points, min_len 2 and 4."""
import os
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
import tracks_util as tu  # noqa: E402

pkg = ge.load_package()
api = pkg.api
dev = torch.device("cuda:0")
up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)


def filled(count, dtype, fill):
    """a tensor of `count` elements (at least one) whose every byte is `fill`"""
    return torch.full((max(count, 1) * torch.empty(0, dtype=dtype).element_size(),), fill, dtype=torch.uint8, device=dev).view(dtype)


def run(n_img, d_feat_ptr, n, d_kp, n_pair, d_ia, d_ib, d_mptr, n_match, d_xa, d_xb, min_len, fill=0):
    st = torch.cuda.Stream(device=dev)
    wb = api.tracks_workspace_bytes(n)
    ws = torch.full((wb + 256,), fill, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    tp, ti, tf, tn = filled(n // 2 + 2, torch.int64, fill), filled(n, torch.int32, fill), filled(n, torch.int32, fill), filled(n, torch.int32, fill)
    tuv, sizes = filled(2 * n, torch.float32, fill), filled(8, torch.int64, fill)
    torch.cuda.synchronize()
    api.tracks_build_device(n_img, d_feat_ptr, n, d_kp, n_pair, d_ia, d_ib, d_mptr, n_match, d_xa, d_xb, min_len, tp, ti, tf, tn, tuv, sizes,
                            ws.data_ptr() + off, wb, st.cuda_stream)
    st.synchronize()
    s = sizes.cpu().numpy()
    assert s[6] == 0, "the error word"
    nt, nv = int(s[0]), int(s[1])
    assert 0 <= nt <= n // 2 + 1 and 0 <= nv <= n, (nt, nv, n)
    return dict(trk_ptr=tp.cpu().numpy()[:nt + 1], trk_img=ti.cpu().numpy()[:nv], trk_feat=tf.cpu().numpy()[:nv], trk_node=tn.cpu().numpy()[:nv],
                trk_uv=tuv.cpu().numpy()[:2 * nv].reshape(-1, 2), counts=s[2:6].copy())


def run_table(table, min_len, kp=None, fill=0):
    n_img, n = len(table["feat_ptr"]) - 1, int(table["feat_ptr"][-1])
    n_pair, n_match = len(table["img_a"]), len(table["idx_a"])
    opt = lambda a, dt: up(a, dt) if len(a) else None
    return run(n_img, up(table["feat_ptr"], np.int64), n, None if kp is None or n == 0 else up(kp, np.float32), n_pair, opt(table["img_a"], np.int32),
               opt(table["img_b"], np.int32), up(table["match_ptr"], np.int64), n_match, opt(table["idx_a"], np.int32), opt(table["idx_b"], np.int32),
               min_len, fill)


def main():
    for name, table in tu.edge_tables():
        n_img = len(table["feat_ptr"]) - 1
        kp = np.arange(2 * int(table["feat_ptr"][-1]), dtype=np.float32).reshape(-1, 2) * 0.5
        for ml in (2, 3, 4, max(n_img, 2), n_img + 1):
            tu.assert_equal(run_table(table, ml, kp=kp), tu.restate(min_len=ml, kp=kp, **table), where=(name, ml))
    print("tracks device ok: tables")

    tb = dict(tu.edge_tables())["five-image chain"]
    clean = tu.restate(min_len=2, **tb)
    bad_feat = dict(tb, idx_a=tb["idx_a"].copy())
    bad_feat["idx_a"][4] = 3   # a feature past its image's end
    bad_img = dict(tb, img_b=tb["img_b"].copy())
    bad_img["img_b"][3] = 5    # an image past the set's end
    neg = dict(tb, idx_b=tb["idx_b"].copy())
    neg["idx_b"][0] = -1
    for bad in (bad_feat, bad_img, neg):
        try:
            api.tracks_build(min_len=2, **bad)
            raise AssertionError("the host form took an index out of range")
        except api.PtzError as e:
            assert e.code == -1
        want = tu.restate(min_len=2, **bad)
        tu.assert_equal(run_table(bad, 2), want)
        assert not all(np.array_equal(want[k], clean[k]) for k in tu.KEYS)
    print("tracks device ok: out of range")

    _, tb2 = tu.order_tables()
    want = tu.restate(min_len=2, **tb2)
    for _ in range(2):
        tu.assert_equal(run_table(tb2, 2, fill=0xFF), want)
    print("tracks device ok: stale workspace")

    sc = pkg.synth.make_scene(0, 20, 100)
    ptr, desc, kp = pkg.synth.make_descriptors(sc, D=128, noise=12, n_distractors=50, seed=1)
    ia, ib = (x.astype(np.int32) for x in np.triu_indices(20, 1))
    ptr = np.asarray(ptr, dtype=np.int64)
    with api.DescSet(ptr, desc, kp) as ds, api.match_descriptors(ds, ds, ia, ib, resident=True) as m:
        host = m.download(uv=False)
        d_mptr, d_xa, d_xb, _, _, _ = m.device_ptrs()
        for ml in (2, 4):
            want = tu.restate(ptr, ia, ib, host["match_ptr"], host["idx_a"], host["idx_b"], ml, kp=kp)
            got = run(20, up(ptr, np.int64), int(ptr[-1]), up(kp, np.float32), len(ia), up(ia, np.int32), up(ib, np.int32), d_mptr, m.n_matches, d_xa,
                      d_xb, ml, fill=0x5A)
            tu.assert_equal(got, want, where=("rig", ml))
            assert len(want["trk_ptr"]) > 10
    print("tracks device ok: rig")


if __name__ == "__main__":
    main()
