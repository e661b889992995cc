"""Helper of test_gpu_landmark_map.py::test_device_form_on_the_matchers_pointers and ::test_device_form_on_the_cases (own process:
torch first, then the library).  Every call of ptz_landmark_assemble_device here runs on a stream with the workspace and every
output filled with a stale pattern (0x5A in every byte) first.

`matcher`: the matcher's resident CSR of the (map, query) pairs (match_ptr, idx_a, uv_b on the device) goes in as it is, without a
host round trip; the outputs equal what the host form gives on the downloaded arrays, for F and FDist.

`cases`: the cases of test_cpu_landmark.py (landmark_util.make_queries: queries of 0, 1, 63, 64, 65, 1025, 7 and 0 matches, the
hand-made query of a landmark behind and one far away, the two anchor ties), for F and FDist, array-equal to the host harness and to
the numpy restatement; then the two rules only the device form has, which the host form rejects as PTZ_EINVAL before they can run:
a landmark index out of range (below 0, n_lm, far beyond) neither votes nor is kept -- the harness and the restatement model it
through landmark_vote -- and a malformed range (the last offset beyond n_match) is an empty one."""
import os
import sys

import numpy as np
import torch

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
import landmark_util as lu  # noqa: E402

pkg = ge.load_package()
api = pkg.api
dev = torch.device("cuda:0")
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def stale(shape, dtype):
    """a tensor whose every byte is 0x5A"""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((n,), 0x5A, dtype=torch.uint8, device=dev).view(dtype).reshape(shape)


def device_form(lmap, nq, nm, d_ptr, d_ia, d_ub, d_cams, d_R, d_wh):
    """ptz_landmark_assemble_device on device pointers, stale workspace and outputs: the dict the host form returns"""
    st = torch.cuda.Stream(device=dev)
    n = max(nm, 1)
    anchor, optr = stale((nq,), torch.int32), stale((nq + 1,), torch.int64)
    oa, ob, osrc = stale((n, 2), torch.float32), stale((n, 2), torch.float32), stale((n,), torch.int32)
    cref, ccur = stale((nq, 15), torch.float64), stale((nq, 15), torch.float64)
    wbytes = api.landmark_assemble_workspace_bytes(nq, nm)
    ws = torch.full((wbytes,), 0x5A, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    torch.cuda.synchronize()
    api.landmark_assemble_device(lmap, nq, nm, d_ptr, d_ia, d_ub, d_cams, d_R, d_wh, anchor, optr, oa, ob, osrc, cref, ccur, ws, wbytes,
                                 stream=st.cuda_stream)
    st.synchronize()
    k = int(optr[-1])
    assert 0 <= k <= nm, (k, nm)
    return dict(anchor_ref=anchor.cpu().numpy(), match_ptr=optr.cpu().numpy(), uv_ref=oa.cpu().numpy()[:k], uv_cur=ob.cpu().numpy()[:k],
                src=osrc.cpu().numpy()[:k], cam_ref=cref.cpu().numpy(), cam_init=ccur.cpu().numpy())


def matcher():
    for ft in (0, 1):
        rig = pkg.synth.make_scene(0, 20, 100).cam_gt.copy()
        if ft:
            rig[:, 10] = np.random.default_rng(1).uniform(-0.05, 0.05, len(rig))
        nq = 6
        sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=nq, n_feat=120, visible_share=0.5, noise_px=0.5, factor_type=ft, seed=4)
        (rp, rd, rk), (qp, qd, qk) = pkg.synth_reloc.make_reloc_descriptors(sc, D=64, noise=8, n_distractors=20, seed=2)
        tp, ti, tf, _ = pkg.synth_reloc.scene_tracks(sc, 20)
        R = api.reloc_ref_rotations(rig)
        with api.DescSet(rp, rd, rk) as refs, api.DescSet(qp, qd, qk) as tests, api.LandmarkMap(refs, rig, tp, ti, tf, factor_type=ft) as lmap:
            m = api.match_descriptors(lmap.desc_set(), tests, np.zeros(nq, dtype=np.int32), np.arange(nq, dtype=np.int32), resident=True, min_matches=8)
            host = m.download()
            nm = m.n_matches
            assert nm > 0 and np.diff(host["match_ptr"]).min() >= 8 and 0 < lmap.n_landmarks < len(sc.ref_track)
            want = api.landmark_assemble(lmap, host["match_ptr"], host["idx_a"], host["uv_b"], sc.query_wh, ref_R=R)
            d_ptr, d_ia, _, _, _, d_ub = m.device_ptrs()
            got = device_form(lmap, nq, nm, d_ptr, d_ia, d_ub, t(rig), t(R), t(sc.query_wh))
            for key, v in got.items():
                assert np.array_equal(v, want[key]), (ft, key)
            assert len(got["src"]) > 0 and (got["anchor_ref"] >= 0).all()
            print("landmark assemble device ok: factor %d, %d of %d matches kept, %d landmarks" % (ft, len(got["src"]), nm, lmap.n_landmarks))
            m.close()


def cases():
    n_feat, counts = 80, [0, 1, 63, 64, 65, 1025, 7, 0]
    for ft in (0, 1):
        cams = lu.make_rig(ft, seed=5 + ft)
        feats = lu.make_features(len(cams), 64, n_feat, seed=6 + ft)
        tp, ti, tf, names = lu.make_tracks(len(cams), n_feat, seed=7 + ft)
        R = api.reloc_ref_rotations(cams)
        with api.DescSet(*feats) as refs, api.LandmarkMap(refs, cams, tp, ti, tf, factor_type=ft) as lmap:
            lm = lmap.arrays()
            n_lm = lmap.n_landmarks
            csr = lu.make_queries(lm, names, counts, seed=9 + ft)
            nq, nm = len(csr["match_ptr"]) - 1, len(csr["idx_a"])
            d_cams, d_R, d_wh = t(cams), t(R), t(csr["query_wh"])

            def both(c, what):
                """harness and restatement on the CSR c, held to each other"""
                h = lu.harness_assemble(lm, ref_cams=cams, ref_R=R, **c)
                lu.assert_equal(h, lu.assemble(lm, ref_cams=cams, ref_R=R, **c), lu.ASM_KEYS, (what, ft, "harness against numpy"))
                return h

            # the well-formed cases
            got = device_form(lmap, nq, nm, t(csr["match_ptr"]), t(csr["idx_a"]), t(csr["uv_b"]), d_cams, d_R, d_wh)
            want = both(csr, "cases")
            lu.assert_equal(got, want, lu.ASM_KEYS, ("cases", ft))
            assert got["anchor_ref"][0] == -1 and got["anchor_ref"][7] == -1 and got["anchor_ref"][nq - 3] == 4
            assert got["anchor_ref"][nq - 2] == got["anchor_ref"][nq - 1] == np.unique(lm["lm_home"])[0]
            assert np.diff(got["match_ptr"])[nq - 3] == np.diff(csr["match_ptr"])[nq - 3] - 2 and 0 < len(got["src"]) < nm

            # landmark indices out of range: in the query of one match (it loses its only vote: anchor -1), in the large query, and
            # among a tie's matches (the tie is broken)
            bad = dict(csr, idx_a=csr["idx_a"].copy())
            p = csr["match_ptr"]
            bad["idx_a"][p[1]] = n_lm
            bad["idx_a"][p[5]:p[5] + 300:7] = -1
            bad["idx_a"][p[5] + 3:p[5] + 300:7] = n_lm + 1000000
            bad["idx_a"][p[nq - 1]] = -7
            got = device_form(lmap, nq, nm, t(bad["match_ptr"]), t(bad["idx_a"]), t(bad["uv_b"]), d_cams, d_R, d_wh)
            want_bad = both(bad, "out of range")
            lu.assert_equal(got, want_bad, lu.ASM_KEYS, ("out of range", ft))
            assert got["anchor_ref"][1] == -1 and got["anchor_ref"][nq - 1] != want["anchor_ref"][nq - 1]
            assert ((bad["idx_a"][got["src"]] >= 0) & (bad["idx_a"][got["src"]] < n_lm)).all() and len(got["src"]) < len(want["src"])

            # a malformed range: the last query's end lies beyond n_match; the device takes it for an empty one, the others stand
            mal = csr["match_ptr"].copy()
            mal[nq] = nm + 7
            got = device_form(lmap, nq, nm, t(mal), t(csr["idx_a"]), t(csr["uv_b"]), d_cams, d_R, d_wh)
            emptied = csr["match_ptr"].copy()
            emptied[nq] = emptied[nq - 1]
            k = int(emptied[nq])
            want_mal = both(dict(csr, match_ptr=emptied, idx_a=csr["idx_a"][:k], uv_b=csr["uv_b"][:k]), "malformed")
            lu.assert_equal(got, want_mal, lu.ASM_KEYS, ("malformed", ft))
            assert got["anchor_ref"][nq - 1] == -1 and got["match_ptr"][nq] == got["match_ptr"][nq - 1]
            print("landmark assemble device cases ok: factor %d, %d queries, %d of %d matches kept" % (ft, nq, len(want["src"]), nm))


if __name__ == "__main__":
    {"matcher": matcher, "cases": cases}[sys.argv[1]]()
