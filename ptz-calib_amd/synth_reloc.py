"""Synthetic relocalization against SEVERAL reference views: queries that observe world rays, every reference that sees a ray gets
the feature (with a probability), so a query has matches in all the views it overlaps -- the input of the assembly
(csrc/ptz_reloc_assemble.h).  A module of its own: synth.py hashes its source into the names of its scene caches."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .synth import _rot_x, _rot_y, rodrigues, rodrigues_inv


@dataclass
class RelocScene:
    """Queries against a rig of references.  The pairs are query-major, the references of a query in ascending order (the order
    run_ptz_reloc lists them in), pairs without matches included."""

    n_query: int
    n_ref: int
    factor_type: int
    ref_cams: np.ndarray     # float64 [n_ref, 15]
    query_wh: np.ndarray     # int32 [n_query, 2]
    cam_gt: np.ndarray       # float64 [n_query, 15]
    pair_ref: np.ndarray     # int32 [n_pair]
    query_ptr: np.ndarray    # int64 [n_query + 1]
    match_ptr: np.ndarray    # int64 [n_pair + 1]
    uv_ref: np.ndarray       # float32 [n_match, 2]
    uv_cur: np.ndarray       # float32 [n_match, 2]
    idx_ref: np.ndarray      # int32 [n_match] feature index in the reference image
    idx_query: np.ndarray    # int32 [n_match] feature index in the query image
    ref_ptr: np.ndarray      # int64 [n_ref + 1] features of the references
    ref_kp: np.ndarray       # float32 [n_ref_feat, 2]
    ref_track: np.ndarray    # int64 [n_ref_feat] world ray of the feature
    query_ptr_feat: np.ndarray  # int64 [n_query + 1]
    query_kp: np.ndarray     # float32 [n_query_feat, 2]
    query_track: np.ndarray  # int64 [n_query_feat]
    width: int = 1920
    height: int = 1080


def _project(cam, R, X, width, height):
    """Pixels of world rays X [n, 3] in camera (cam 15, R 3x3) with the generator's radial model, and their visibility."""
    pc = X @ R.T
    z = pc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        x = pc[:, 0] / z
        y = pc[:, 1] / z
        r2 = x * x + y * y
        rad = 1.0 + cam[10] * r2
        u = cam[0] * x * rad + cam[2]
        v = cam[1] * y * rad + cam[3]
    vis = (z > 0.1) & (u >= 8) & (u <= width - 8) & (v >= 8) & (v <= height - 8) & (r2 < 1.5)
    return u, v, vis


def make_reloc_scene(rig, n_query: int = 24, n_feat: int = 600, visible_share: float = 0.5, noise_px: float = 0.5,
                     factor_type: int = 0, seed: int = 0, f_range=(1500.0, 4000.0), width: int = 1920, height: int = 1080,
                     query_cams=None) -> RelocScene:
    """rig: the references' cameras [n_ref, 15] (one projection centre).  Every query looks near one of the references (pan within
    +-6 degrees, tilt within +-4 of it) with f ~ U(f_range) and, for factor_type & 1, k1 ~ U(-0.05, 0.05); it observes n_feat world
    rays, uniform over its frame.  A reference that sees a ray (8 px inside its frame) gets the feature with probability
    visible_share; both pixels carry Gaussian noise of noise_px.  Features of an image are in ascending ray order.
    query_cams [n_query, 15]: the queries' cameras (focal, rotation vector, k1) instead of drawn ones -- make_reloc_sequence."""
    rng = np.random.default_rng(seed)
    rig = np.asarray(rig, dtype=np.float64)
    n_ref = rig.shape[0]
    Rref = np.stack([rodrigues(c[4:7]) for c in rig])
    cx, cy = 0.5 * width, 0.5 * height
    cam_gt = np.zeros((n_query, 15))
    ref_feats = [[] for _ in range(n_ref)]   # (track, u, v)
    q_ptr, q_kp, q_track = [0], [], []
    obs = []  # per query: list over refs of (track ids seen, pixels)
    for q in range(n_query):
        if query_cams is None:
            near = int(rng.integers(0, n_ref))
            R = _rot_x(math.radians(rng.uniform(-4, 4))) @ _rot_y(math.radians(rng.uniform(-6, 6))) @ Rref[near]
            f = rng.uniform(*f_range)
            k1 = rng.uniform(-0.05, 0.05) if (factor_type & 1) else 0.0
        else:
            R, f, k1 = rodrigues(np.asarray(query_cams[q], dtype=np.float64)[4:7]), float(query_cams[q][0]), float(query_cams[q][10])
        cam = np.zeros(15)
        cam[0] = cam[1] = f
        cam[2], cam[3] = cx, cy
        cam[4:7] = rodrigues_inv(R)
        cam[10] = k1
        cam_gt[q] = cam
        # rays uniform over the frame's normalised extent, kept where the distorted pixel is inside
        xn = rng.uniform(-1.1 * cx / f, 1.1 * cx / f, 4 * n_feat)
        yn = rng.uniform(-1.1 * cy / f, 1.1 * cy / f, 4 * n_feat)
        X = np.stack([xn, yn, np.ones_like(xn)], axis=1) @ R
        u, v, vis = _project(cam, R, X, width, height)
        keep = np.nonzero(vis)[0][:n_feat]
        X, u, v = X[keep], u[keep], v[keep]
        base = q * n_feat  # world ray ids of this query
        q_kp.append(np.stack([u + rng.normal(0, noise_px, len(u)), v + rng.normal(0, noise_px, len(u))], axis=1))
        q_track.append(base + np.arange(len(u)))
        q_ptr.append(q_ptr[-1] + len(u))
        per_ref = []
        for r in range(n_ref):
            ur, vr, visr = _project(rig[r], Rref[r], X, width, height)
            got = np.nonzero(visr & (rng.random(len(ur)) < visible_share))[0]
            pix = np.stack([ur[got] + rng.normal(0, noise_px, len(got)), vr[got] + rng.normal(0, noise_px, len(got))], axis=1)
            first = len(ref_feats[r])
            ref_feats[r].extend(zip((base + got).tolist(), pix[:, 0].tolist(), pix[:, 1].tolist()))
            per_ref.append((got, first))
        obs.append(per_ref)
    # reference features in the order they were added (ascending query, ascending ray): already ascending track id
    ref_ptr = np.concatenate([[0], np.cumsum([len(f) for f in ref_feats])]).astype(np.int64)
    flat = [t for f in ref_feats for t in f]
    ref_track = np.array([t[0] for t in flat], dtype=np.int64)
    ref_kp = np.array([[t[1], t[2]] for t in flat], dtype=np.float32).reshape(-1, 2)
    query_kp = np.concatenate(q_kp).astype(np.float32) if q_kp else np.zeros((0, 2), np.float32)
    query_track = np.concatenate(q_track).astype(np.int64) if q_track else np.zeros(0, np.int64)
    qf_ptr = np.asarray(q_ptr, dtype=np.int64)
    match_ptr, pair_ref, ia, ib = [0], [], [], []
    for q in range(n_query):
        for r in range(n_ref):
            got, first = obs[q][r]
            ia.append(first + np.arange(len(got)))
            ib.append(got)
            match_ptr.append(match_ptr[-1] + len(got))
            pair_ref.append(r)
    idx_ref = np.concatenate(ia).astype(np.int32) if ia else np.zeros(0, np.int32)
    idx_query = np.concatenate(ib).astype(np.int32) if ib else np.zeros(0, np.int32)
    pair_ref = np.asarray(pair_ref, dtype=np.int32)
    match_ptr = np.asarray(match_ptr, dtype=np.int64)
    pair_of = np.repeat(np.arange(len(pair_ref)), np.diff(match_ptr))
    uv_ref = ref_kp[ref_ptr[pair_ref[pair_of]] + idx_ref]
    uv_cur = query_kp[qf_ptr[pair_of // max(n_ref, 1)] + idx_query]
    return RelocScene(n_query=n_query, n_ref=n_ref, factor_type=factor_type, ref_cams=rig.copy(),
                      query_wh=np.tile(np.array([width, height], dtype=np.int32), (n_query, 1)), cam_gt=cam_gt, pair_ref=pair_ref,
                      query_ptr=(np.arange(n_query + 1, dtype=np.int64) * n_ref), match_ptr=match_ptr,
                      uv_ref=np.ascontiguousarray(uv_ref, dtype=np.float32), uv_cur=np.ascontiguousarray(uv_cur, dtype=np.float32),
                      idx_ref=idx_ref, idx_query=idx_query, ref_ptr=ref_ptr, ref_kp=ref_kp, ref_track=ref_track, query_ptr_feat=qf_ptr,
                      query_kp=query_kp, query_track=query_track, width=width, height=height)


def make_reloc_descriptors(scene: RelocScene, D: int = 128, noise: int = 12, n_distractors: int = 50, seed: int = 0,
                           repeat_share: float = 0, repeat_group: int = 4, repeat_noise: int = 6):
    """Descriptors as synth.make_descriptors draws them: one uniform random descriptor per world ray, every feature a copy with
    uniform integer noise in [-noise, noise], clipped; n_distractors unmatched random features are appended to every reference and
    every query image, so the scene's feature indices stay valid.
    repeat_share > 0: texture that repeats -- of every query's rays that share (at random) is put in groups of repeat_group whose
    base descriptors are one descriptor, each member with a perturbation of its own in [-repeat_noise, repeat_noise].  With
    repeat_share = 0 no further random number is drawn.
    Returns ((feat_ptr, desc, kp) of the references, (feat_ptr, desc, kp) of the queries)."""
    rng = np.random.default_rng(seed)
    n_track = int(max(scene.ref_track.max(initial=-1), scene.query_track.max(initial=-1))) + 1
    base = rng.integers(0, 256, (n_track, D), dtype=np.int64)
    if repeat_share > 0:
        for q in range(len(scene.query_ptr_feat) - 1):
            tracks = scene.query_track[int(scene.query_ptr_feat[q]):int(scene.query_ptr_feat[q + 1])]
            n_rep = int(repeat_share * len(tracks)) // repeat_group * repeat_group
            groups = tracks[rng.permutation(len(tracks))[:n_rep]].reshape(-1, repeat_group)
            if len(groups):
                base[groups] = np.clip(base[groups[:, 0]][:, None, :] + rng.integers(-repeat_noise, repeat_noise + 1, (len(groups), repeat_group, D)), 0, 255)
    out = []
    for ptr, kp, track in ((scene.ref_ptr, scene.ref_kp, scene.ref_track), (scene.query_ptr_feat, scene.query_kp, scene.query_track)):
        obs = np.clip(base[track] + rng.integers(-noise, noise + 1, (len(track), D)), 0, 255).astype(np.uint8)
        descs, kps = [], []
        n_img = len(ptr) - 1
        for i in range(n_img):
            sl = slice(int(ptr[i]), int(ptr[i + 1]))
            descs += [obs[sl], rng.integers(0, 256, (n_distractors, D), dtype=np.uint8)]
            kps += [kp[sl], rng.uniform([0, 0], [scene.width, scene.height], (n_distractors, 2)).astype(np.float32)]
        feat_ptr = (np.asarray(ptr, dtype=np.int64) + n_distractors * np.arange(n_img + 1)).astype(np.int64)
        out.append((feat_ptr, np.concatenate(descs) if descs else np.zeros((0, D), np.uint8),
                    np.concatenate(kps).astype(np.float32) if kps else np.zeros((0, 2), np.float32)))
    return out[0], out[1]


def scene_tracks(scene: RelocScene, n_distractors: int = 0):
    """The tracks of the references' features as CSR, from RelocScene.ref_track: one track per world ray some reference sees, in
    ascending ray order, its views in ascending image order.  trk_feat is the feature's index inside its image -- the index it keeps
    in the sets of make_reloc_descriptors(scene, n_distractors=...), whose distractor features come after an image's own and belong
    to no track (n_distractors is taken for the signature's sake: it moves no index).
    Returns (trk_ptr int64 [n_track + 1], trk_img int32, trk_feat int32, trk_ray int64 [n_track]: the world ray of each track)."""
    del n_distractors
    img = np.repeat(np.arange(scene.n_ref), np.diff(scene.ref_ptr)).astype(np.int64)
    feat = np.arange(len(scene.ref_track), dtype=np.int64) - scene.ref_ptr[img]
    order = np.lexsort((img, scene.ref_track))  # by ray, then by image
    rays, counts = np.unique(scene.ref_track[order], return_counts=True)
    trk_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return trk_ptr, img[order].astype(np.int32), feat[order].astype(np.int32), rays.astype(np.int64)


def perturb_cameras(cam, angle_deg: float, f_rel: float, seed: int = 0) -> np.ndarray:
    """Prior cameras from true ones [n, 15]: every camera turned by angle_deg about an axis drawn uniformly on the sphere, its
    focal lengths scaled by 1 + f_rel or 1 - f_rel (a fair coin); everything else is copied."""
    rng = np.random.default_rng(seed)
    out = np.array(cam, dtype=np.float64).reshape(-1, 15).copy()
    for c in out:
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        c[4:7] = rodrigues_inv(rodrigues(axis * math.radians(angle_deg)) @ rodrigues(c[4:7]))
        c[0:2] *= 1.0 + (f_rel if rng.random() < 0.5 else -f_rel)
    return out


def make_reloc_sequence(rig, n_frames: int = 12, step_deg: float = 0.4, zoom_rate: float = 0.01, cut_at=None, cut_deg: float = 45.0,
                        start_pan_deg: float = -45.0, start_f: float = 2200.0, **scene) -> RelocScene:
    """A broadcast sweep over the rig: frame t pans step_deg on from frame t - 1 and zooms in by zoom_rate (f_t = f_(t-1) (1 + zoom_rate)),
    starting at pan start_pan_deg (tilt 0) and focal start_f; at frame cut_at, if given, the pan jumps by a further cut_deg -- a cut
    to another camera position of the same rig.  The frames observe world rays as make_reloc_scene's queries do (its keyword
    arguments pass through); cam_gt holds the frames' cameras in order."""
    cams = np.zeros((n_frames, 15))
    pan, f = start_pan_deg, start_f
    for t in range(n_frames):
        if t > 0:
            pan, f = pan + step_deg, f * (1.0 + zoom_rate)
        if cut_at is not None and t == cut_at:
            pan += cut_deg
        cams[t, 0] = cams[t, 1] = f
        cams[t, 4:7] = rodrigues_inv(_rot_y(math.radians(pan)))
    return make_reloc_scene(rig, n_query=n_frames, query_cams=cams, **scene)
