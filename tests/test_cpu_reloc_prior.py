"""CPU tests of the contract of relocalization from a prior camera: the shared header (ptz-calib_amd/csrc/ptz_reloc_prior.h)
instantiated on the host by tests/cpu_harness/reloc_prior_harness.cc against the numpy restatement (reloc_prior_util.py), array-equal
-- no ulp bound, as for the assembly -- and the additions to the multi-reference generator (synth_reloc.py)."""
import hashlib
import math

import numpy as np
import pytest

import reloc_assemble_util as ru
import reloc_prior_harness as ph
import reloc_prior_util as pu


def _both(cams, pri, wh, factor_type, R, min_overlap=8):
    Rr, Rq = ph.rotations(cams), ph.rotations(pri)
    got = ph.harness_prior_pairs(cams, Rr, pri, Rq, wh, factor_type, R, min_overlap)
    want = pu.prior_pairs(cams, Rr, pri, Rq, wh, factor_type, R, min_overlap)
    pu.assert_equal(got, want, (factor_type, R, min_overlap))
    return got


def _cam(f, pan_deg=0.0, tilt_deg=0.0, cx=960.0, cy=540.0, fy=None):
    c = np.zeros(15)
    c[0], c[1], c[2], c[3] = f, f if fy is None else fy, cx, cy
    c[4:7] = [math.radians(tilt_deg), math.radians(pan_deg), 0.0]
    return c


@pytest.mark.parametrize("factor_type", [0, 1, 2, 3])
@pytest.mark.parametrize("R", [1, 4, 8, 70])
def test_harness_equals_numpy_on_mixed_cameras(factor_type, R):
    """Twelve references (ten around pan 0, one 75 degrees away, one behind) and nine priors, one with the rig behind it and one
    looking straight up: H of every slot, scores, lists and counts, array-equal; fy enters H only where the factor type frees it."""
    cams = ru.make_rig(factor_type & 1, seed=factor_type)
    pri, wh = ph.make_priors(9, 10 + factor_type, behind=(3,), away=(6,), pan=(-25.0, 25.0), tilt=(-8.0, 8.0), dist=bool(factor_type & 1))
    out = _both(cams, pri, wh, factor_type, R)
    assert out["n_short"][3] <= 1 and out["n_short"][6] == 0 and (out["overlap"][6] == 0).all()
    assert (out["n_short"] <= min(R, len(cams))).all() and out["n_short"].max() >= min(R, 7) and out["overlap"].max() <= 128
    for q in range(len(pri)):
        n = int(out["n_short"][q])
        assert (np.diff(out["shortlist"][q, :n]) > 0).all() and (out["shortlist"][q, n:] == -1).all() and not out["H_slot"][q, n:].any()
    Kq = ph.harness_query_K(pri[0], wh[0, 0], wh[0, 1], factor_type)
    assert np.array_equal(Kq, pu.query_K(pri[0], wh[0, 0], wh[0, 1], factor_type))
    assert Kq[1] == (pri[0, 0] if factor_type < 2 else pri[0, 1]) and Kq[2] == 0.5 * wh[0, 0] and pri[0, 1] != pri[0, 0]


def test_h_of_the_true_camera_maps_reference_pixels_onto_query_pixels():
    """Rays seen by both cameras: a -> K_q R_q R_r^T K_r^-1 a in plain float64 matrix algebra is where H puts a, within the rounding
    of the float32 pixel the warp returns (pixels below 4096: spacing 2^-12, so half of it plus float64 noise)."""
    rng = np.random.default_rng(5)
    ref, qry = _cam(2400.0, 3.0, -2.0), _cam(3100.0, 7.0, 1.0, fy=3150.0)
    Rr, Rq = ph.rotations(ref[None])[0], ph.rotations(qry[None])[0]
    for factor_type in (0, 2):
        Kq = pu.query_K(qry, 1920, 1080, factor_type)
        H = ph.harness_homography(ref, Rr, Kq, Rq)
        assert np.array_equal(H, pu.homography(ref, Rr, Kq, Rq))
        a = rng.uniform([0, 0], [1920, 1080], (200, 2)).astype(np.float32)
        n = np.stack([(a[:, 0].astype(np.float64) - ref[2]) / ref[0], (a[:, 1].astype(np.float64) - ref[3]) / ref[1], np.ones(len(a))], axis=1)
        m = n @ Rr.reshape(3, 3) @ Rq.reshape(3, 3).T
        want = np.stack([Kq[0] * m[:, 0] / m[:, 2] + Kq[2], Kq[1] * m[:, 1] / m[:, 2] + Kq[3]], axis=1)
        wx, wy, ok = pu.gu.warp(H, a)
        inside = (np.abs(want) < 4096).all(axis=1)
        assert ok.all() and inside.sum() > 100
        assert np.abs(np.stack([wx, wy], axis=1)[inside] - want[inside]).max() <= 2.0 ** -12
        # the other direction comes from the same M transposed: H(q -> r) H(r -> q) is the identity up to scale
        Hb = ph.harness_homography(Kq, Rq, ref, Rr)
        P = Hb.reshape(3, 3) @ H.reshape(3, 3)
        assert np.abs(P / P[2, 2] - np.eye(3)).max() < 1e-9


def test_a_reference_behind_the_query_scores_zero_and_is_never_listed():
    cams = np.stack([_cam(2000.0, 0.0), _cam(2000.0, 180.0), _cam(2000.0, 95.0)])
    out = _both(cams, _cam(2000.0, 1.0)[None], np.array([[1920, 1080]], dtype=np.int32), 0, 8, min_overlap=0)
    assert out["overlap"][0].tolist()[1:] == [0, 0] and out["overlap"][0, 0] > 100
    assert out["shortlist"][0].tolist() == [0] + [-1] * 7 and out["n_short"][0] == 1  # (min_overlap 0 still needs one point)


def test_a_query_inside_a_wide_reference_and_the_converse():
    """Same axis, focal 1000 against 4000 on 1920 x 1080: every point of the narrow frame's lattice lands in the wide one (64), and of
    the wide frame's lattice the four central points (120 and 67.5 px off the centre -> 480 and 270 px) land in the narrow one."""
    wide, narrow = _cam(1000.0), _cam(4000.0)
    wh = np.array([[1920, 1080]], dtype=np.int32)
    assert _both(wide[None], narrow[None], wh, 0, 1)["overlap"].tolist() == [[68]]
    assert _both(narrow[None], wide[None], wh, 0, 1)["overlap"].tolist() == [[68]]
    assert _both(wide[None], wide[None], wh, 0, 1)["overlap"].tolist() == [[128]]


def test_equal_scores_pick_the_lower_index_and_min_overlap_cuts():
    a, b, far = _cam(2500.0, 0.0), _cam(2500.0, 4.0), _cam(2500.0, 30.0)
    cams = np.stack([far, b, a, b, a, far])
    pri, wh = _cam(2500.0, 0.5)[None], np.array([[1920, 1080]], dtype=np.int32)
    out = _both(cams, pri, wh, 0, 1)
    s = out["overlap"][0]
    assert s[2] == s[4] > s[1] == s[3] > s[0] == s[5] and out["shortlist"][0].tolist() == [2]
    assert _both(cams, pri, wh, 0, 3)["shortlist"][0].tolist() == [1, 2, 4]  # both a, and the first b; written ascending
    cut = _both(cams, pri, wh, 0, 6, min_overlap=int(s[1]) + 1)
    assert cut["shortlist"][0].tolist() == [2, 4, -1, -1, -1, -1] and cut["n_short"][0] == 2
    assert _both(cams, pri, wh, 0, 6, min_overlap=int(s[1]))["n_short"][0] == 4
    assert s[2] == 128 and _both(cams, pri, wh, 0, 6, min_overlap=128)["n_short"][0] == 2  # (the bound is inclusive)
    assert _both(cams[[0, 1, 3, 5]], pri, wh, 0, 6, min_overlap=128)["n_short"][0] == 0


def test_more_slots_than_references():
    cams = ph.make_cams(3, 1, pan=(-3.0, 3.0), tilt=(-2.0, 2.0))
    pri, wh = ph.make_priors(4, 2, pan=(-3.0, 3.0), tilt=(-2.0, 2.0))
    out = _both(cams, pri, wh, 2, 70)
    assert (out["n_short"] == 3).all() and (out["shortlist"][:, :3] == np.arange(3)).all() and (out["shortlist"][:, 3:] == -1).all()


@pytest.mark.parametrize("factor_type", [0, 1, 2, 3])
def test_prior_camera_rule(factor_type):
    rng = np.random.default_rng(factor_type)
    cur, pri = rng.uniform(-1, 1, (5, 15)), rng.uniform(1, 2, (5, 15))
    got = ph.harness_prior_camera(cur, pri, factor_type)
    assert np.array_equal(got, pu.prior_camera(cur, pri, factor_type))
    assert np.array_equal(got[:, [2, 3, 7, 8, 9]], cur[:, [2, 3, 7, 8, 9]]) and np.array_equal(got[:, 4:7], pri[:, 4:7])
    assert np.array_equal(got[:, 10:], pri[:, 10:]) and np.array_equal(got[:, 0], pri[:, 0])
    assert np.array_equal(got[:, 1], pri[:, 0] if factor_type < 2 else pri[:, 1])


# ------------------------------------------------------------------------------------------------------------------ the generator
def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_descriptor_generator_draws_its_earlier_bytes_without_repeats(pkg):
    """The digest was taken from make_reloc_descriptors before it had the repeat_* arguments."""
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt
    sc = pkg.synth_reloc.make_reloc_scene(rig, n_query=3, n_feat=40, seed=2)
    (rp, rd, rk), (qp, qd, qk) = pkg.synth_reloc.make_reloc_descriptors(sc, D=32, noise=12, n_distractors=5, seed=4)
    assert _digest((rp, rd, rk, qp, qd, qk)) == "cc1b45108a17e6405ea5391ea70b9a6a268b959bbbe3fc9d7f8b268f7cf8d6c1"
    (_, r2, _), (_, q2, _) = pkg.synth_reloc.make_reloc_descriptors(sc, D=32, noise=12, n_distractors=5, seed=4, repeat_share=0.7)
    assert r2.shape == rd.shape and q2.shape == qd.shape and not np.array_equal(q2, qd)
    # groups of four rays of one query share a base: their descriptors are within repeat_noise + 2 noise of each other
    d = np.abs(q2[:40, None, :].astype(np.int64) - q2[None, :40, :].astype(np.int64)).max(axis=2)
    near = (d <= 2 * 6 + 2 * 12).sum(axis=1) - 1
    assert (near == 3).sum() == int(0.7 * 40) // 4 * 4 and (near == 0).sum() == 40 - int(0.7 * 40) // 4 * 4


def test_perturb_cameras_turns_by_the_angle_and_scales_the_focal(pkg):
    cams = ph.make_cams(6, 3)
    out = pkg.synth_reloc.perturb_cameras(cams, 0.3, 0.02, seed=1)
    assert np.array_equal(out[:, [2, 3]], cams[:, [2, 3]]) and np.array_equal(out[:, 7:], cams[:, 7:])
    assert np.allclose(np.abs(out[:, 0] / cams[:, 0] - 1), 0.02) and np.allclose(out[:, 1] / cams[:, 1], out[:, 0] / cams[:, 0])
    for a, b in zip(cams, out):
        Ra, Rb = ru.rodrigues(a[4:7]).reshape(3, 3), ru.rodrigues(b[4:7]).reshape(3, 3)
        ang = math.degrees(math.acos(min(1.0, (np.trace(Rb @ Ra.T) - 1) / 2)))
        assert abs(ang - 0.3) < 1e-6
    assert np.array_equal(out, pkg.synth_reloc.perturb_cameras(cams, 0.3, 0.02, seed=1))


def test_sequence_pans_zooms_and_cuts(pkg):
    rig = pkg.synth.make_scene(0, 20, 100).cam_gt
    sc = pkg.synth_reloc.make_reloc_sequence(rig, n_frames=6, step_deg=0.4, zoom_rate=0.01, cut_at=4, n_feat=60, seed=1)
    assert sc.n_query == 6 and (np.diff(sc.query_ptr_feat) == 60).all() and (np.diff(sc.match_ptr).reshape(6, -1).sum(axis=1) > 60).all()
    R = [ru.rodrigues(c[4:7]).reshape(3, 3) for c in sc.cam_gt]
    ang = [math.degrees(math.acos(min(1.0, (np.trace(R[t + 1] @ R[t].T) - 1) / 2))) for t in range(5)]
    assert np.allclose(ang, [0.4, 0.4, 0.4, 45.4, 0.4], atol=1e-6) and np.allclose(sc.cam_gt[1:, 0] / sc.cam_gt[:-1, 0], 1.01)
