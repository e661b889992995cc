"""The prior's contract (ptz-calib_amd/csrc/ptz_reloc_prior.h) restated in numpy: the pair homography in float64 with every product
and sum rounded on its own and in the header's order, the overlap score over the two 8 x 8 lattices through the guided matcher's
restated warp (desc_guided_util.warp), the list as a sort, the prior's part of the initial camera.  The yardstick of the CPU harness
(tests/cpu_harness/reloc_prior_harness.cc) and, through it, of the device; nothing here is shared with either."""
from __future__ import annotations

import numpy as np

import desc_guided_util as gu

LATTICE = 8
KEYS = ("shortlist", "n_short", "overlap", "H_slot")


def one_focal(factor_type):
    return (int(factor_type) & 2) == 0


def query_K(prior, w, h, factor_type):
    """[fx, fy, cx, cy] of a query from its prior and its image size."""
    prior = np.asarray(prior, dtype=np.float64)
    return np.array([prior[0], prior[0] if one_focal(factor_type) else prior[1], 0.5 * float(w), 0.5 * float(h)])


def homography(cam_from, R_from, cam_to, R_to):
    """H [9] row-major, b ~ H a for a pixel a of `from`: K_to (R_to R_from^T) K_from^-1, the inverse written out."""
    cf, ct = np.asarray(cam_from, dtype=np.float64), np.asarray(cam_to, dtype=np.float64)
    Rf, Rt = np.asarray(R_from, dtype=np.float64).reshape(9), np.asarray(R_to, dtype=np.float64).reshape(9)
    N = np.zeros(9)
    with np.errstate(all="ignore"):
        for i in range(3):
            m0 = Rt[3 * i] * Rf[0] + Rt[3 * i + 1] * Rf[1] + Rt[3 * i + 2] * Rf[2]
            m1 = Rt[3 * i] * Rf[3] + Rt[3 * i + 1] * Rf[4] + Rt[3 * i + 2] * Rf[5]
            m2 = Rt[3 * i] * Rf[6] + Rt[3 * i + 1] * Rf[7] + Rt[3 * i + 2] * Rf[8]
            N[3 * i] = m0 / cf[0]
            N[3 * i + 1] = m1 / cf[1]
            N[3 * i + 2] = (m2 - N[3 * i] * cf[2]) - N[3 * i + 1] * cf[3]
        H = np.zeros(9)
        for j in range(3):
            H[j] = ct[0] * N[j] + ct[2] * N[6 + j]
            H[3 + j] = ct[1] * N[3 + j] + ct[3] * N[6 + j]
            H[6 + j] = N[6 + j]
    return H


def lattice(W, H):
    """The 64 float32 cell centres of [0, W) x [0, H), row by row."""
    k = np.arange(LATTICE, dtype=np.float64) + 0.5
    x = (k * float(W) / 8.0).astype(np.float32)
    y = (k * float(H) / 8.0).astype(np.float32)
    return np.stack([np.tile(x, LATTICE), np.repeat(y, LATTICE)], axis=1)


def lattice_count(H, W, Hh, w_to, h_to):
    wx, wy, ok = gu.warp(H, lattice(W, Hh))
    with np.errstate(all="ignore"):
        return int((ok & (wx >= 0) & (wx < np.float32(w_to)) & (wy >= 0) & (wy < np.float32(h_to))).sum())


def overlap(cam_r, R_r, Kq, R_q, w_q, h_q):
    """(score in 0 .. 128, H(reference -> query))."""
    cam_r = np.asarray(cam_r, dtype=np.float64)
    H_rq = homography(cam_r, R_r, Kq, R_q)
    H_qr = homography(Kq, R_q, cam_r, R_r)
    Wr, Hr = cam_r[2] * 2.0, cam_r[3] * 2.0
    return lattice_count(H_rq, Wr, Hr, np.float32(w_q), np.float32(h_q)) + lattice_count(H_qr, float(w_q), float(h_q), np.float32(Wr), np.float32(Hr)), H_rq


def shortlist(scores, R, min_overlap):
    """The references of one query in ascending index: ranked by (score descending, index ascending), below max(min_overlap, 1) never."""
    scores = np.asarray(scores, dtype=np.int64)
    order = np.argsort(-scores, kind="stable")
    ranked = [int(r) for r in order if scores[r] >= max(int(min_overlap), 1)]
    return sorted(ranked[:int(R)])


def prior_pairs(ref_cams, ref_R, prior_cams, prior_R, query_wh, factor_type=0, max_refs=8, min_overlap=8):
    """The dict api.reloc_prior_pairs returns (without device_ms)."""
    cams = np.asarray(ref_cams, dtype=np.float64).reshape(-1, 15)
    pri = np.asarray(prior_cams, dtype=np.float64).reshape(-1, 15)
    Rr, Rq = np.asarray(ref_R, dtype=np.float64).reshape(-1, 9), np.asarray(prior_R, dtype=np.float64).reshape(-1, 9)
    wh = np.asarray(query_wh).reshape(-1, 2)
    nq, n_ref, R = len(pri), len(cams), int(max_refs)
    sl = np.full((nq, R), -1, dtype=np.int32)
    ns = np.zeros(nq, dtype=np.int32)
    ov = np.zeros((nq, n_ref), dtype=np.int32)
    Hs = np.zeros((nq, R, 9))
    for q in range(nq):
        Kq = query_K(pri[q], wh[q, 0], wh[q, 1], factor_type)
        H = []
        for r in range(n_ref):
            s, h = overlap(cams[r], Rr[r], Kq, Rq[q], int(wh[q, 0]), int(wh[q, 1]))
            ov[q, r] = s
            H.append(h)
        take = shortlist(ov[q], R, min_overlap)
        ns[q] = len(take)
        sl[q, :len(take)] = take
        for s, r in enumerate(take):
            Hs[q, s] = H[r]
    return dict(shortlist=sl, n_short=ns, overlap=ov, H_slot=Hs)


def prior_camera(cam_cur, prior_cams, factor_type):
    """reloc_prior_camera on [n, 15] arrays: a copy of cam_cur with the prior's focal, rotation vector and distortion."""
    out = np.array(cam_cur, dtype=np.float64).reshape(-1, 15).copy()
    pri = np.asarray(prior_cams, dtype=np.float64).reshape(-1, 15)
    out[:, 0] = pri[:, 0]
    out[:, 1] = pri[:, 0] if one_focal(factor_type) else pri[:, 1]
    out[:, 4:7] = pri[:, 4:7]
    out[:, 10:15] = pri[:, 10:15]
    return out


def assert_equal(got, want, what=""):
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, k)
