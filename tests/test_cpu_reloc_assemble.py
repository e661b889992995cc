"""CPU tests of the relocalization assembly's contract: the shared header (ptz-calib_amd/csrc/ptz_reloc_assemble.h) instantiated on
the host by tests/cpu_harness/reloc_assemble_harness.cc against the numpy restatement (reloc_assemble_util.py), the argument errors
of the C-ABI's host form that need no device, and the invariants of the multi-reference generator (synth_reloc.py)."""
import ctypes as C

import numpy as np
import pytest

import reloc_assemble_util as ru

KS = (1, 2, 4, 7)


def _both(csr, cams, factor_type, K):
    R = ru.harness_rotations(cams)
    got = ru.harness_assemble(ref_cams=cams, factor_type=factor_type, max_refs=K, ref_R=R, **csr)
    want = ru.assemble(ref_cams=cams, factor_type=factor_type, max_refs=K, ref_R=R, **csr)
    ru.assert_equal(got, want, (factor_type, K))
    return got


def test_rotations_on_host_agree_with_numpy():
    """The matrices are an INPUT of the contract (made once, by one host function, and handed to host and device alike), so their
    bits are nobody's yardstick: libm's cos and sin may differ in the last place between a sincos call and two calls."""
    for dist in (0, 1):
        cams = ru.make_rig(dist)
        cams[3, 4:7] = 0.0  # the identity branch
        R = ru.harness_rotations(cams)
        assert np.abs(R - ru.rotations(cams)).max() <= 4 * np.finfo(np.float64).eps
        assert np.array_equal(R[3], np.eye(3).reshape(9))


@pytest.mark.parametrize("factor_type", [0, 1, 2, 3])
@pytest.mark.parametrize("K", KS)
def test_harness_equals_numpy_on_mixed_lists(factor_type, K):
    """Ties, zero-count pairs, empty lists, K above the list length, the same reference twice, references behind the anchor and
    75 degrees away, pixels outside the frame: selection, cameras, kept sets, out_src and the transferred pixels, array-equal."""
    cams = ru.make_rig(factor_type & 1, seed=factor_type)
    lens = [0, 1, 2, 5, 12, 0, 3, 30]
    counts = lambda q, j: [0, 1, 7, 7, 0, 33, 7, 120][(3 * q + j) % 8]
    csr = ru.make_csr(lens, counts, len(cams), seed=K)
    out = _both(csr, cams, factor_type, K)
    assert out["n_sel"][0] == 0 and out["n_sel"][5] == 0 and out["match_ptr"][1] == 0
    assert np.isfinite(out["cam_ref"]).all() and np.isfinite(out["cam_init"]).all()
    assert (out["n_sel"] <= K).all() and out["n_sel"][1] == 1
    if K > 1:
        assert out["match_ptr"][-1] < sum(int(n) for n in np.diff(csr["match_ptr"])), "nothing was dropped: the cases are not covered"


def test_selection_ties_zero_counts_and_short_lists():
    cams = ru.make_rig(0)
    # list 0: counts 5 9 9 0 9 2 -> positions 1, 2, 4, 0, 5 (first wins a tie, the zero never ranks); list 1: all zero; list 2: one pair
    table = [[5, 9, 9, 0, 9, 2], [0, 0, 0], [4]]
    csr = ru.make_csr([6, 3, 1], lambda q, j: table[q][j], len(cams))
    out = _both(csr, cams, 0, 7)
    assert out["sel_pair"][0].tolist() == [1, 2, 4, 0, 5, -1, -1] and out["n_sel"].tolist() == [5, 0, 1]
    assert out["sel_pair"][1].tolist() == [-1] * 7 and out["sel_pair"][2].tolist() == [9] + [-1] * 6
    # the unusable query gets the cameras of the first reference of its list
    r = int(csr["pair_ref"][6])
    assert out["cam_init"][1, 0] == cams[r, 0] and np.array_equal(out["cam_init"][1, 4:], cams[r, 4:])
    one = _both(csr, cams, 0, 1)
    assert one["sel_pair"][:, 0].tolist() == [1, -1, 9]


def test_k1_is_a_copy_and_the_tools_cameras():
    cams = ru.make_rig(1)
    csr = ru.make_csr([4, 2], lambda q, j: [3, 50, 50, 1][j], len(cams), refs_of=lambda q, j: [2, 7, 7, 1][j] if q == 0 else 11)
    out = _both(csr, cams, 1, 1)
    lo, hi = int(csr["match_ptr"][1]), int(csr["match_ptr"][2])
    sl = slice(0, int(out["match_ptr"][1]))
    assert np.array_equal(out["src"][sl], np.arange(lo, hi)) and np.array_equal(out["uv_ref"][sl], csr["uv_ref"][lo:hi])
    assert np.array_equal(out["cam_ref"][0], cams[7])
    w, h = csr["query_wh"][0]
    want = cams[7].copy()
    want[1] = want[0]
    want[2], want[3] = 0.5 * w, 0.5 * h
    assert np.array_equal(out["cam_init"][0], want)


@pytest.mark.parametrize("dist", [0, 1])
def test_geometry_cases_of_the_transfer(dist):
    """Anchor = reference 5 (pan 0).  Reference 11 looks the other way: every match dropped (m_z <= 0).  Reference 10 is 75 degrees
    away: its pixels leave [0, 2S).  A pixel outside view r's own frame is dropped by the border guard only for the distortion
    variants.  The anchor's own matches pass through the identity rotation."""
    cams = ru.make_rig(dist)
    refs = [5, 11, 10, 6]
    csr = ru.make_csr([4], lambda q, j: [40, 30, 20, 10][j], len(cams), refs_of=lambda q, j: refs[j], seed=3)
    out = _both(csr, cams, dist, 4)
    ptr = csr["match_ptr"]
    src = out["src"]
    assert out["sel_pair"][0].tolist() == [0, 1, 2, 3]
    assert not ((src >= ptr[1]) & (src < ptr[2])).any(), "a reference behind the anchor kept a match"
    far = (src >= ptr[2]) & (src < ptr[3])
    R = ru.rotations(cams)
    px, keep = ru.transfer(cams[10], R[10], R[5], cams[5, 0], dist, csr["uv_ref"][ptr[2]:ptr[3]])
    with np.errstate(invalid="ignore"):
        assert (~keep).any() and int(far.sum()) == int(keep.sum()) and ((px[~keep] >= 2 * ru.S) | (px[~keep] < 0) | ~np.isfinite(px[~keep])).any()
    own = csr["uv_ref"][ptr[0]:ptr[1]]
    outside = (own[:, 0] < 0) | (own[:, 0] >= 1920) | (own[:, 1] < 0) | (own[:, 1] >= 1080)
    assert outside.any()
    kept_own = np.isin(np.arange(ptr[0], ptr[1]), src)
    if dist:  # the guard is view r's own: the undistorted pixel outside [0, 2 cx) x [0, 2 cy), exactly the matches the solve would skip
        ou, ov = ru.undistort(cams[5], own[:, 0], own[:, 1])
        guard = (ou < 0) | (ou >= 1920) | (ov < 0) | (ov >= 1080)
        assert guard.any() and not kept_own[guard].any() and kept_own[~guard].all()
    else:
        assert kept_own.all()
        a = out["uv_ref"][:ptr[1]]  # F: the anchor's pixels move by fa / fx = 1 and S - cx up to the float32 rounding at 16384
        assert np.abs(a - (own + np.float32([ru.S - 960, ru.S - 540]))).max() <= 2 * 2.0 ** -10
    assert out["cam_ref"][0].tolist() == [cams[5, 0], cams[5, 0], ru.S, ru.S] + cams[5, 4:10].tolist() + [0.0] * 5


def test_a_query_does_not_depend_on_its_batch():
    cams = ru.make_rig(1)
    csr = ru.make_csr([3, 0, 9, 1, 20], lambda q, j: (7 * q + 3 * j) % 11, len(cams), seed=5)
    full = ru.harness_assemble(ref_cams=cams, factor_type=1, max_refs=4, **csr)
    for qs in ([4, 3, 2, 1, 0], [2], [0, 1], [2, 3, 4]):
        sub, idx = ru.slice_queries(csr, qs)
        part = ru.harness_assemble(ref_cams=cams, factor_type=1, max_refs=4, **sub)
        for k, q in enumerate(qs):
            a, b = ru.per_query(part, k), ru.per_query(full, q)
            assert np.array_equal(idx[a["src"]], b["src"])
            for key in ("n_sel", "uv_ref", "uv_cur", "cam_ref", "cam_init"):
                assert np.array_equal(a[key], b[key]), (qs, q, key)


# --------------------------------------------------------------------------------------------------------------- argument errors
def test_host_form_argument_errors_need_no_device(pkg):
    L = pkg.api.lib()
    cams = ru.make_rig(0)
    R = ru.rotations(cams)
    base = ru.make_csr([2, 1], lambda q, j: 3, len(cams))

    def call(n_query=2, n_pair=3, n_ref=len(cams), factor_type=0, K=2, device_id=0, drop=(), **over):
        c = {k: np.array(v) for k, v in base.items()}
        c.update(over)
        nm = int(max(c["match_ptr"][-1], 1))
        outs = dict(sel=np.zeros(max(K, 1) * 2, np.int32), nsel=np.zeros(2, np.int32), optr=np.zeros(3, np.int64), oa=np.zeros((nm, 2), np.float32),
                    ob=np.zeros((nm, 2), np.float32), osrc=np.zeros(nm, np.int32), cref=np.zeros((2, 15)), ccur=np.zeros((2, 15)))
        ins = dict(ptr=c["match_ptr"], a=c["uv_ref"], b=c["uv_cur"], pref=c["pair_ref"], qptr=c["query_ptr"], cams=cams, R=R, wh=c["query_wh"])
        p = {k: (None if k in drop else v.ctypes.data_as(C.c_void_p)) for k, v in {**ins, **outs}.items()}
        return L.ptz_reloc_assemble(n_query, n_pair, n_ref, p["ptr"], p["a"], p["b"], p["pref"], p["qptr"], p["cams"], p["R"], p["wh"],
                                    factor_type, K, device_id, p["sel"], p["nsel"], p["optr"], p["oa"], p["ob"], p["osrc"], p["cref"],
                                    p["ccur"], None)

    EINVAL, EUNSUPPORTED = -1, -4
    assert call(n_query=-1) == EINVAL and call(n_pair=-1) == EINVAL and call(n_ref=-1) == EINVAL
    assert call(K=0) == EINVAL and call(K=-3) == EINVAL and call(device_id=-1) == EINVAL
    assert call(match_ptr=np.array([0, 3, 2, 9], np.int64)) == EINVAL  # decreasing
    assert call(match_ptr=np.array([1, 3, 6, 9], np.int64)) == EINVAL  # does not start at 0
    assert call(query_ptr=np.array([0, 3, 2], np.int64)) == EINVAL
    assert call(query_ptr=np.array([0, 2, 2], np.int64)) == EINVAL  # does not cover the pairs
    assert call(pair_ref=np.array([0, len(cams), 1], np.int32)) == EINVAL and call(pair_ref=np.array([0, -1, 1], np.int32)) == EINVAL
    assert call(query_wh=np.array([[1920, 0], [1920, 1080]], np.int32)) == EINVAL
    assert call(query_wh=np.array([[1920, 1080], [-5, 1080]], np.int32)) == EINVAL
    for missing in ("ptr", "a", "b", "pref", "qptr", "cams", "R", "wh", "sel", "nsel", "optr", "oa", "ob", "osrc", "cref", "ccur"):
        assert call(drop=(missing,)) == EINVAL, missing
    assert call(n_ref=0) == EINVAL
    assert call(factor_type=4) == EUNSUPPORTED and call(factor_type=-1) == EUNSUPPORTED
    assert call(n_query=0, n_pair=0, query_ptr=np.array([0], np.int64), match_ptr=np.array([0], np.int64)) == 0
    assert pkg.api.reloc_assemble_workspace_bytes(-1, 5) == 0 and pkg.api.reloc_assemble_workspace_bytes(3, 1000) % 256 == 0
    assert np.abs(pkg.api.reloc_ref_rotations(cams) - ru.rotations(cams)).max() <= 4 * np.finfo(np.float64).eps


# -------------------------------------------------------------------------------------------------------------------- generator
@pytest.fixture(scope="module")
def rig20(pkg):
    return pkg.synth.make_scene(0, 20, 100).cam_gt


@pytest.mark.parametrize("factor_type", [0, 1])
def test_generator_invariants(pkg, rig20, factor_type):
    rig = rig20.copy()
    if factor_type:
        rig[:, 10] = np.random.default_rng(1).uniform(-0.05, 0.05, len(rig))
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=6, n_feat=200, visible_share=0.5, noise_px=0.0, factor_type=factor_type, seed=2)
    n_ref = len(rig)
    assert sc.n_ref == n_ref and len(sc.pair_ref) == 6 * n_ref and sc.query_ptr.tolist() == list(range(0, 6 * n_ref + 1, n_ref))
    assert np.array_equal(sc.pair_ref, np.tile(np.arange(n_ref), 6)) and (np.diff(sc.match_ptr) >= 0).all()
    counts = np.diff(sc.match_ptr).reshape(6, n_ref)
    assert ((counts > 0).sum(axis=1) >= 3).all(), "a query should overlap several views"
    # a match joins the two features of one world ray, and its pixels are the features' pixels
    pair_of = np.repeat(np.arange(len(sc.pair_ref)), np.diff(sc.match_ptr))
    fr = sc.ref_ptr[sc.pair_ref[pair_of]] + sc.idx_ref
    fq = sc.query_ptr_feat[pair_of // n_ref] + sc.idx_query
    assert np.array_equal(sc.ref_track[fr], sc.query_track[fq])
    assert np.array_equal(sc.uv_ref, sc.ref_kp[fr]) and np.array_equal(sc.uv_cur, sc.query_kp[fq])
    # without noise both pixels are projections of one ray: the reference pixel, undistorted and rotated, lands on the query's ray
    R = ru.rotations(rig)
    for q in range(6):
        Rq = pkg.synth.rodrigues(sc.cam_gt[q, 4:7])
        for r in np.nonzero(counts[q])[0][:3]:
            sl = slice(int(sc.match_ptr[q * n_ref + r]), int(sc.match_ptr[q * n_ref + r + 1]))
            ou, ov = ru.undistort(rig[r], sc.uv_ref[sl, 0], sc.uv_ref[sl, 1]) if factor_type else (sc.uv_ref[sl, 0], sc.uv_ref[sl, 1])
            n = np.stack([(ou - rig[r, 2]) / rig[r, 0], (ov - rig[r, 3]) / rig[r, 1], np.ones(len(ou))], axis=1)
            m = n @ R[r].reshape(3, 3) @ Rq.T
            x, y = m[:, 0] / m[:, 2], m[:, 1] / m[:, 2]
            rad = 1.0 + sc.cam_gt[q, 10] * (x * x + y * y)
            pred = np.stack([sc.cam_gt[q, 0] * x * rad + 960, sc.cam_gt[q, 0] * y * rad + 540], axis=1)
            assert np.abs(pred - sc.uv_cur[sl]).max() < 0.05, (q, r)
    # visible_share thins the matches; the seed fixes the scene
    fewer = pkg.synth_reloc.make_reloc_scene(rig, n_query=6, n_feat=200, visible_share=0.25, noise_px=0.0, factor_type=factor_type, seed=2)
    assert 0.3 < fewer.match_ptr[-1] / sc.match_ptr[-1] < 0.7
    again = pkg.synth_reloc.make_reloc_scene(rig, n_query=6, n_feat=200, visible_share=0.5, noise_px=0.0, factor_type=factor_type, seed=2)
    assert np.array_equal(again.uv_ref, sc.uv_ref) and np.array_equal(again.match_ptr, sc.match_ptr)
    (rp, rd, rk), (qp, qd, qk) = pkg.synth_reloc.make_reloc_descriptors(sc, D=32, noise=4, n_distractors=5, seed=1)
    assert rp[-1] == len(rd) == len(rk) == sc.ref_ptr[-1] + 5 * n_ref and qp[-1] == len(qd) == sc.query_ptr_feat[-1] + 5 * 6
    # the two features of a match carry one ray's descriptor, up to the noise
    d = np.abs(rd[rp[sc.pair_ref[pair_of]] + sc.idx_ref].astype(int) - qd[qp[pair_of // n_ref] + sc.idx_query].astype(int))
    assert d.max() <= 8 and rd.dtype == np.uint8


# ------------------------------------------------------------------------------------------------------------- the serving loop
def test_relocalizer_defaults_and_argument_errors_need_no_device(pkg):
    api, L = pkg.api, pkg.api.lib()
    o = api.RelocOptions()
    L.ptz_reloc_options_default(C.byref(o))
    assert (o.match.ratio, o.match.cross_check, o.guided_radius, o.ransac_thresh, o.min_inliers) == (0.8, 1, 0.0, 4.0, 6)
    assert (o.inlier_matches, o.trim, o.uncertainty, o.max_refs, o.factor_type, o.max_reproj_error) == (0, 0, 0, 1, 0, 100.0)
    assert (o.trim_options.trim_px, o.trim_options.max_rounds, o.gate_max_pair_matches) == (4.0, 8, 2048) and o.lm.max_num_iterations > 0
    h = C.c_void_p()
    cams = ru.make_rig(0)
    fake = C.c_void_p(1)  # never dereferenced: every call below fails its argument checks first
    EINVAL = -1
    assert L.ptz_relocalizer_create(None, cams.ctypes.data_as(C.c_void_p), 12, 0, C.byref(h)) == EINVAL and not h.value
    assert L.ptz_relocalizer_create(fake, None, 12, 0, C.byref(h)) == EINVAL
    assert L.ptz_relocalizer_create(fake, cams.ctypes.data_as(C.c_void_p), 0, 0, C.byref(h)) == EINVAL
    assert L.ptz_relocalizer_create(fake, cams.ctypes.data_as(C.c_void_p), 12, -1, C.byref(h)) == EINVAL
    assert L.ptz_relocalizer_create(fake, cams.ctypes.data_as(C.c_void_p), 12, 0, None) == EINVAL
    r = api.RelocResult()
    assert L.ptz_relocalizer_run(None, fake, 1, None, C.byref(o), C.byref(r)) == EINVAL
    L.ptz_relocalizer_n_matches.restype = C.c_int64
    L.ptz_relocalizer_table.restype = C.c_void_p
    assert L.ptz_relocalizer_n_matches(None) == 0 and L.ptz_relocalizer_table(None) is None
    assert L.ptz_relocalizer_matches(None, None, None, None, None) == EINVAL
    L.ptz_relocalizer_destroy.restype = None
    L.ptz_relocalizer_destroy(None)
