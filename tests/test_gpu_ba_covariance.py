"""GPU tests of the per-view covariance of bundle-adjusted cameras (ptz_ba_batch_covariance, ptz-calib_amd/csrc/ptz_ba_cov.hip)
through the C-ABI: parity with the independent restatement of ba_cov_util.py at the project's bound for covariances, view
batches, untouched outputs, no side effects, bit-equality across batch position / runs / grouping, the statistics of 400
noisy solves on the device, the C++ class and the tool."""
import copy
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import ba_cov_util as bu
import host_util as hu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-6  # |C_ij - Cref_ij| <= BOUND sqrt(Cref_ii Cref_jj); sigma0 to 1e-9 relative

# (scene id, views, obs per view, factor type, anchors): 6 x 40 of each type with the anchor first, in the middle and last;
# n = 64 (exactly one tile) and n = 65; 20 x 100 of six parameters; one rig of five tiles (72 views, n = 288)
PARITY = [(5, 6, 40, 0, (0, 3, 5)), (5, 6, 40, 1, (0, 3, 5)), (5, 6, 40, 2, (0, 3, 5)), (5, 16, 40, 0, (8,)), (5, 13, 40, 1, (12,)),
          (5, 20, 100, 2, (0,)), (5, 72, 30, 0, (36,))]


@pytest.mark.parametrize("sid,nv,no,ft,anchors", PARITY)
def test_parity_with_the_restatement(pkg, sid, nv, no, ft, anchors):
    sc, cam, ray = bu.solved_scene(sid, nv, no, ft)
    nf = pkg.api.ba_cov_dim(ft)
    assert nf * nv >= 280 or nv < 70
    for g in anchors:
        st, ref, s0, cond = bu.restated(sid, nv, no, ft, g)
        cov, sig, stt = pkg.api.ba_covariance(sc, cam, ray, gauge_cam=g)
        assert st == bu.OK and stt == pkg.api.COV_OK
        d = bu.scaled_diff(cov, ref)
        print(f"type {ft} {nv}x{no} anchor {g}: scaled diff {d:.2e}, sigma0 rel {abs(sig / s0 - 1):.1e}, cond {cond:.1e}")
        assert d <= BOUND
        assert abs(sig / s0 - 1) <= 1e-9
        assert (cov == cov.transpose(0, 2, 1)).all()
        r0 = bu.ROT0[ft]
        assert (cov[g, r0:r0 + 3, :] == 0).all() and (cov[g, :, r0:r0 + 3] == 0).all() and cov[g, 0, 0] > 0
        # a-priori: the same matrix at another scale
        cov_p, sig_p, st_p = pkg.api.ba_covariance(sc, cam, ray, gauge_cam=g, pixel_sigma=0.7)
        assert st_p == pkg.api.COV_OK and sig_p == sig
        assert np.abs(cov_p - cov * (0.7 / sig) ** 2).max() <= 1e-13 * np.abs(cov_p).max()


def test_view_batch_equals_the_restatement_and_single_rays_add_nothing(pkg, orc):
    sc = pkg.synth.make_scene(7, 12, 60)
    images = [1, 2, 4, 5, 6, 9, 10]
    vp = pkg.api.view_problem(sc, images)
    counts = np.bincount(vp.obs_ray, minlength=vp.n_ray)
    assert (vp.ray_weight > counts).any() and (counts == 1).any()  # full track lengths above the candidate counts; single rays exist
    cam, ray, _, summ, _ = orc.ba_solve(vp, jacobian_mode=orc.JAC_ANALYTIC)
    st, ref, s0, _ = bu.restate(vp, cam, ray, 2)
    assert st == bu.OK
    rig = pkg.api.Rig.from_scene(sc)
    vb = pkg.api.ViewBatch([rig], [images], factor_type=0)
    vb.set_state(cams=[cam], rays=[ray])
    covs, sig, stt, _ = vb.covariance(gauge_cam=[2])
    assert stt[0] == pkg.api.COV_OK
    d = bu.scaled_diff(covs[0], ref)
    print(f"view batch: scaled diff {d:.2e}, sigma0 rel {abs(sig[0] / s0 - 1):.1e}")
    assert d <= BOUND and abs(sig[0] / s0 - 1) <= 1e-9
    # the packed problem of the same view gives the same bits
    pb = pkg.api.BaBatch([vp]); pb.set_state(cams=[cam], rays=[ray])
    covp, sigp, stp, _ = pb.covariance(gauge_cam=[2])
    assert stp[0] == 0 and (covp[0] == covs[0]).all() and sigp[0] == sig[0]
    # without the rays of a single candidate observation: S and T are the same sums
    keep_ray = counts >= 2
    keep = keep_ray[vp.obs_ray]
    v2 = copy.copy(vp)
    v2.obs_uv, v2.obs_cam = vp.obs_uv[keep], vp.obs_cam[keep]
    v2.obs_ray = (np.cumsum(keep_ray) - 1)[vp.obs_ray[keep]].astype(np.int32)
    v2.n_ray = int(keep_ray.sum()); v2.ray_weight = vp.ray_weight[keep_ray]
    c1, _, s1 = pkg.api.ba_covariance(vp, cam, ray, gauge_cam=2, pixel_sigma=0.5)
    c2, _, s2 = pkg.api.ba_covariance(v2, cam, ray[keep_ray], gauge_cam=2, pixel_sigma=0.5)
    assert s1 == 0 and s2 == 0
    assert bu.scaled_diff(c2, c1) <= 1e-12
    vb.close(); pb.close(); rig.close()


def _isolate_camera(sc, c):
    """camera c's observations removed from every other view's tracks: each becomes a ray of its own"""
    s = copy.copy(sc)
    mine = np.flatnonzero(sc.obs_cam == c)
    rest = np.flatnonzero(sc.obs_cam != c)
    new_ray = sc.n_ray + np.arange(len(mine))
    s.obs_uv = np.concatenate([sc.obs_uv[rest], sc.obs_uv[mine]])
    s.obs_cam = np.concatenate([sc.obs_cam[rest], sc.obs_cam[mine]]).astype(np.int32)
    s.obs_ray = np.concatenate([sc.obs_ray[rest], new_ray]).astype(np.int32)
    s.n_ray = sc.n_ray + len(mine)
    s.ray_weight = np.concatenate([sc.ray_weight, np.ones(len(mine))])
    return s, np.concatenate([np.arange(sc.n_ray), sc.obs_ray[mine]])


def test_outputs_untouched_unless_ok(pkg):
    sc, cam, ray = bu.solved_scene(5, 6, 40, 0)
    # DOF: two cameras, two shared rays: m = 8 <= p = 8 - 3 + 4
    both = [r for r in range(sc.n_ray) if {0, 1} <= set(sc.obs_cam[sc.obs_ray == r])][:2]
    assert len(both) == 2
    sel = np.flatnonzero(np.isin(sc.obs_ray, both) & (sc.obs_cam <= 1))
    tiny = copy.copy(sc)
    tiny.n_cam, tiny.n_ray = 2, 2
    tiny.obs_uv, tiny.obs_cam = sc.obs_uv[sel], sc.obs_cam[sel]
    tiny.obs_ray = np.searchsorted(both, sc.obs_ray[sel]).astype(np.int32)
    tiny.ray_weight = sc.ray_weight[both]
    iso, ray_map = _isolate_camera(sc, 2)
    bad = cam.copy(); bad[3, 0] = np.nan
    cases = [(tiny, cam[:2], ray[both], pkg.api.COV_DOF), (iso, cam, ray[ray_map], pkg.api.COV_SINGULAR), (sc, bad, ray, pkg.api.COV_SINGULAR)]
    for s, c, r, want in cases:
        cov = np.full((s.n_cam, 4, 4), -7.25)
        cov, sig, st = pkg.api.ba_covariance(s, c, r, cov=cov)
        assert st == want and (cov == -7.25).all() and sig == 0.0
    # in one batch with a problem that is fine: only that one is written
    b = pkg.api.BaBatch([tiny, sc, iso])
    b.set_state(cams=[cam[:2], cam, cam], rays=[ray[both], ray, ray[ray_map]])
    cov = np.full((2 + 6 + 6, 4, 4), -7.25); sig = np.full(3, -1.5)
    covs, sig, st, _ = b.covariance(cov=cov, sigma0=sig)
    assert list(st) == [pkg.api.COV_DOF, pkg.api.COV_OK, pkg.api.COV_SINGULAR]
    assert (covs[0] == -7.25).all() and (covs[2] == -7.25).all() and sig[0] == -1.5 and sig[2] == -1.5
    solo, ssolo, _ = pkg.api.ba_covariance(sc, cam, ray)
    assert (covs[1] == solo).all() and sig[1] == ssolo
    b.close()


def test_a_solve_after_the_call_is_the_solve_without_it(pkg):
    scs = [pkg.synth.make_scene(0, 20, 100), pkg.synth.make_scene(2, 6, 40)]
    a = pkg.api.BaBatch(scs); a.set_state(); sa = a.solve(); ca, ra = a.get_state()
    b = pkg.api.BaBatch(scs); b.set_state()
    _, _, st0, _ = b.covariance()       # at the state last set, before any solve
    sb = b.solve()
    cov1, s1, st1, _ = b.covariance()   # at the minimum-cost point
    cb, rb = b.get_state()
    sb2 = b.solve(); cb2, rb2 = b.get_state()
    assert list(st0) == [0, 0] and list(st1) == [0, 0]
    assert sa == sb == sb2
    for i in range(2):
        assert (ca[i] == cb[i]).all() and (ra[i] == rb[i]).all() and (ca[i] == cb2[i]).all() and (ra[i] == rb2[i]).all()
        one, sone, _ = pkg.api.ba_covariance(scs[i], cb[i], rb[i])
        assert (cov1[i] == one).all() and s1[i] == sone   # evaluated at exactly the state get_state returns
    a.close(); b.close()


def test_bits_do_not_depend_on_position_run_or_grouping(pkg):
    sc, cam, ray = bu.solved_scene(5, 20, 100, 2)
    small, cs, rs = bu.solved_scene(5, 6, 40, 2)
    big, cbg, rbg = bu.solved_scene(6, 30, 60, 2)
    solo, ssolo, st = pkg.api.ba_covariance(sc, cam, ray, gauge_cam=4)
    assert st == 0
    again, sagain, _ = pkg.api.ba_covariance(sc, cam, ray, gauge_cam=4)
    assert (again == solo).all() and sagain == ssolo
    b = pkg.api.BaBatch([sc] * 5); b.set_state(cams=[cam] * 5, rays=[ray] * 5)
    covs, sig, stt, _ = b.covariance(gauge_cam=[4] * 5)
    assert (stt == 0).all()
    for i in (0, 4):  # first and last member of a batch of copies
        assert (covs[i] == solo).all() and sig[i] == ssolo
    old = os.environ.get("PTZ_BA_COV_MAX_MB")
    os.environ["PTZ_BA_COV_MAX_MB"] = "1"  # every problem a group of its own
    try:
        covg, sigg, stg, _ = b.covariance(gauge_cam=[4] * 5)
    finally:
        if old is None:
            del os.environ["PTZ_BA_COV_MAX_MB"]
        else:
            os.environ["PTZ_BA_COV_MAX_MB"] = old
    assert (stg == 0).all() and all((covg[i] == solo).all() for i in range(5)) and (sigg == ssolo).all()
    b.close()
    # mixed sizes in one group: another padded order, the same numbers
    m = pkg.api.BaBatch([small, sc, big]); m.set_state(cams=[cs, cam, cbg], rays=[rs, ray, rbg])
    covm, sigm, stm, _ = m.covariance(gauge_cam=[0, 4, 0])
    assert (stm == 0).all()
    d = bu.scaled_diff(covm[1], solo)
    print(f"mixed batch against solo: scaled diff {d:.2e}")
    assert d <= 1e-10 and abs(sigm[1] / ssolo - 1) <= 1e-12
    m.close()


def test_device_covariance_predicts_the_scatter_of_noisy_solves(pkg):
    """The 400 noisy copies of the CPU test as ONE batch through ptz_ba_batch_solve and ptz_ba_batch_covariance: every ratio
    observed / predicted lies in 1 +- 4 / sqrt(2 N) = [0.86, 1.14]."""
    base, copies = bu.noisy_copies()
    N = len(copies)
    b = pkg.api.BaBatch(copies); b.set_state()
    summ = b.solve()
    assert all(s["termination_type"] == 0 for s in summ)
    cams, _ = b.get_state()
    covs, sig, st, ms = b.covariance()
    assert (st == 0).all()
    ratios = bu.stat_ratios(cams, covs, sig, anchor=0)
    lo, hi = 1 - 4 / np.sqrt(2 * N), 1 + 4 / np.sqrt(2 * N)
    print({k: round(float(v), 3) for k, v in ratios.items()}, f"device {ms:.3f} ms")
    assert len(ratios) == 6 + 5 * 3 + 1
    for k, v in ratios.items():
        assert lo <= v <= hi, (k, v, lo, hi)
    b.close()


def _class_solve_cov(pkg, sc, cand, ftype, gauge_image, annotations=None):
    """PTZRayOptimizer::Solve, Covariance and StdDevs through the host library's test entry"""
    from ctypes import POINTER, byref, c_double, c_float, c_int32, c_int64
    lib = hu.lib()
    kps, plist = hu.scene_to_features_matches(sc)
    _p = hu._p
    n_img = len(kps)
    kp_ptr = np.concatenate([[0], np.cumsum([len(k) for k in kps])]).astype(np.int64)
    kp_xy = np.ascontiguousarray(np.concatenate([np.asarray(k, dtype=np.float32).reshape(-1, 2) for k in kps]), dtype=np.float32)
    src = np.array([p[0] for p in plist], dtype=np.int64); dst = np.array([p[1] for p in plist], dtype=np.int64)
    mptr = np.concatenate([[0], np.cumsum([len(p[2]) for p in plist])]).astype(np.int64)
    q = np.array([m[0] for p in plist for m in p[2]], dtype=np.int32); t = np.array([m[1] for p in plist for m in p[2]], dtype=np.int32)
    cam = np.array(sc.cam_init, dtype=np.float64, order="C").copy()
    cand = np.array(list(cand), dtype=np.int64)
    ann_ptr = ann_uv = ann_xyz = None
    if annotations is not None:
        acam = np.asarray(annotations["cam"])
        ann_ptr = np.searchsorted(acam, np.arange(n_img + 1)).astype(np.int64)
        ann_uv = np.ascontiguousarray(annotations["uv"], dtype=np.float32); ann_xyz = np.ascontiguousarray(annotations["xyz"], dtype=np.float64)
    cov = np.zeros(36 * len(cand)); sd = np.zeros(6 * len(cand)); s0 = c_double(); before = c_int32(-1)
    n_obs = c_int32(); n_ray = c_int32()
    puv = POINTER(c_float)(); pcam = POINTER(c_int32)(); pray = POINTER(c_int32)(); pw = POINTER(c_double)()
    pc15 = POINTER(c_double)(); pr3 = POINTER(c_double)(); pci = POINTER(c_int64)()
    code = lib.ptzh_ptzray_solve_cov(n_img, _p(kp_ptr), _p(kp_xy), len(plist), _p(src), _p(dst), _p(mptr), _p(q), _p(t), _p(cam), _p(ann_ptr),
                                     _p(ann_uv), _p(ann_xyz), _p(cand), len(cand), 200, ftype, c_int64(gauge_image), _p(cov), _p(sd), byref(s0),
                                     byref(before), byref(n_obs), byref(n_ray), byref(puv), byref(pcam), byref(pray), byref(pw), byref(pc15),
                                     byref(pr3), byref(pci))
    no, nr, nc = n_obs.value, n_ray.value, len(cand)
    packed = copy.copy(sc)
    packed.n_cam, packed.n_ray, packed.factor_type = nc, nr, ftype
    packed.obs_uv = np.ctypeslib.as_array(puv, (no, 2)).copy(); packed.obs_cam = np.ctypeslib.as_array(pcam, (no,)).copy()
    packed.obs_ray = np.ctypeslib.as_array(pray, (no,)).copy(); packed.ray_weight = np.ctypeslib.as_array(pw, (nr,)).copy()
    pcams = np.ctypeslib.as_array(pc15, (nc, 15)).copy(); prays = np.ctypeslib.as_array(pr3, (nr, 3)).copy()
    images = np.ctypeslib.as_array(pci, (nc,)).copy()
    for x in (puv, pcam, pray, pw, pc15, pr3, pci):
        lib.ptzh_free(x)
    return code, before.value, cov, sd, s0.value, packed, pcams, prays, images


def test_class_covariance_equals_the_batch_call(pkg):
    sc = pkg.synth.make_scene(3, 12, 60, factor_type=1)
    cand = [0, 1, 2, 3, 5, 6, 7, 8, 10, 11]
    code, before, cov, sd, s0, packed, pcams, prays, images = _class_solve_cov(pkg, sc, cand, 1, 5)
    assert code == 7 and before == 0 and list(images) == cand
    nf = 5
    g = cand.index(5)
    want, swant, st = pkg.api.ba_covariance(packed, pcams, prays, gauge_cam=g)
    assert st == 0
    cov = cov[:nf * nf * len(cand)].reshape(len(cand), nf, nf)
    assert (cov == want).all() and s0 == swant
    assert (sd[:nf * len(cand)].reshape(len(cand), nf) == np.sqrt(np.einsum("cii->ci", want))).all()
    # gauge_image = -1: the lowest candidate image
    code, _, cov0, _, _, _, _, _, _ = _class_solve_cov(pkg, sc, cand, 1, -1)
    want0, _, _ = pkg.api.ba_covariance(packed, pcams, prays, gauge_cam=0)
    assert code == 7 and (cov0[:nf * nf * len(cand)].reshape(len(cand), nf, nf) == want0).all()
    # an image that is no candidate, and an annotated problem: false
    assert _class_solve_cov(pkg, sc, cand, 1, 4)[0] == 1
    ann = pkg.synth.add_annotations(pkg.synth.make_scene(1, 20, 100))
    code, before, *_ = _class_solve_cov(pkg, ann, list(range(20)), 0, -1, annotations=ann.obs3d)
    assert code == 1 and before == 0


def _run_tool(name, *args):
    exe = os.path.join(ROOT, "ptz-calib_amd", "bin", name)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)


def test_run_ptz_ba_uncertainty_side_file(pkg, tmp_path):
    sc = pkg.synth.add_annotations(pkg.synth.make_scene(1, 20, 100))
    tb = pkg.synth.make_match_table(sc)
    paths = pkg.dataset_io.write_rig(str(tmp_path), sc, tb, annotations=sc.obs3d)
    out_a, out_b = str(tmp_path / "out_a"), str(tmp_path / "out_b")
    args = ["-i", paths["images"], "-f", paths["features"], "-a", paths["annotation"]]
    ra = _run_tool("run_ptz_ba", *args, "--output=" + out_a)
    rb = _run_tool("run_ptz_ba", *args, "--output=" + out_b, "--uncertainty")
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr, rb.stderr)
    main_a = open(os.path.join(out_a, "rig0.json"), "rb").read()
    assert main_a == open(os.path.join(out_b, "rig0.json"), "rb").read()
    assert not os.path.exists(os.path.join(out_a, "rig0_uncertainty.json"))
    u = json.load(open(os.path.join(out_b, "rig0_uncertainty.json")))
    assert list(u["images"].keys()) == list(paths["names"]) and u["anchor"] in paths["names"]
    assert 0.3 < u["sigma0"] < 0.8  # 0.5 px of noise on the key points
    anchor = u["anchor"]
    for name, rec in u["images"].items():
        assert rec["sigma_f"] > 0 and "sigma_k1" not in rec
        assert (np.array(rec["sigma_rot_deg"]) == 0).all() if name == anchor else (np.array(rec["sigma_rot_deg"]) > 0).all()
    # the values are the API's: the same 2D-2D problem over the registered views, solved by the class from the same cameras, is
    # what the tool evaluates -- here through the library on the problem the match table packs to, at its own minimum
    cams = np.array([[rec["sigma_f"]] + list(np.radians(rec["sigma_rot_deg"])) for rec in u["images"].values()])
    kps = [tb.kp_xy[tb.kp_ptr[i]:tb.kp_ptr[i + 1]] for i in range(tb.n_img)]
    plist = [(int(tb.src[p]), int(tb.dst[p]), list(zip(tb.q[tb.match_ptr[p]:tb.match_ptr[p + 1]].tolist(), tb.t[tb.match_ptr[p]:tb.match_ptr[p + 1]].tolist())))
             for p in range(tb.n_pairs)]
    ok, _, _, _, packed = hu.ptzray_solve(kps, plist, sc.cam_init, cand_ids=range(tb.n_img), ftype=0)
    assert ok
    ps = copy.copy(sc)
    ps.n_cam, ps.n_ray, ps.factor_type = tb.n_img, len(packed["ray_weight"]), 0
    ps.obs_uv, ps.obs_cam, ps.obs_ray, ps.ray_weight = packed["obs_uv"], packed["obs_cam"], packed["obs_ray"], packed["ray_weight"]
    ps.obs3d = None
    cov, s0, st = pkg.api.ba_covariance(ps, packed["cam"], packed["ray"], gauge_cam=list(paths["names"]).index(anchor))
    assert st == 0
    sd = np.sqrt(np.einsum("cii->ci", cov))
    # the tool starts its bundle adjustment from PTZ-IBA's cameras, this one from the initial guess: the same minimum to the
    # solver's tolerances, so the standard deviations agree to a part in a thousand, not to the bit
    assert np.abs(cams - sd).max() <= 1e-3 * sd.max() and abs(u["sigma0"] / s0 - 1) <= 1e-3
    keep = sd > 0
    assert (np.abs(cams[keep] / sd[keep] - 1) <= 1e-2).all()
