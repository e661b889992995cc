"""The reference shortlist's contract (ptz-calib_amd/csrc/ptz_desc_shortlist.h) restated in numpy on top of desc_match_util's
brute-force top-2: the probe rule, the vote rule, the ranking and the ascending output.  The yardstick of the CPU harness and of
the device kernels; nothing here is shared with either."""
from __future__ import annotations

import numpy as np

import desc_match_util as du


def probes(n, M):
    """The features [min(n, M)] (int64) of a query image with n features that vote under a budget of M."""
    n, M = int(n), int(M)
    if n <= M:
        return np.arange(n, dtype=np.int64)
    return np.array([k * n // M for k in range(M)], dtype=np.int64)  # Python integers: exact


def dist2(a, b):
    """desc_match_util.dist2's values, the product through float64: every term and sum is an integer below 2^53, so it is exact
    (and the matrix product is the fast one)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)).astype(np.int64)


def vote_mask(d, j, s, ratio=0.8, max_dist2=0):
    """Which probes vote, from their top-2 (d, j, s) over all features of one reference."""
    ok = j != du.INT32_MAX
    if ratio > 0:
        ok &= d.astype(np.float64) < (float(ratio) * float(ratio)) * s.astype(np.float64)
    if max_dist2 != 0:
        ok &= d <= max_dist2
    return ok


def votes_of(query, refs, M, ratio=0.8, max_dist2=0):
    """votes [n_ref] int32 of one query image (uint8 [n, D]) against a list of reference images."""
    p = probes(len(query), M)
    out = np.zeros(len(refs), dtype=np.int32)
    if len(p) == 0:
        return out
    a = np.asarray(query)[p]
    for r, b in enumerate(refs):
        if len(b) == 0:
            continue
        d, j, s = du.top2(dist2(a, b))
        out[r] = int(vote_mask(d, j, s, ratio, max_dist2).sum())
    return out


def select(votes, R, min_votes=1):
    """(row [R] with -1 in unused slots, n_short) of one query: ranked by (votes descending, index ascending), at least
    max(min_votes, 1) votes, the first R, written in ascending index."""
    votes = np.asarray(votes, dtype=np.int64)
    order = sorted(range(len(votes)), key=lambda r: (-int(votes[r]), r))
    ranked = [r for r in order if votes[r] >= max(int(min_votes), 1)]
    take = sorted(ranked[:int(R)])
    row = np.full(int(R), -1, dtype=np.int32)
    row[:len(take)] = take
    return row, len(take)


def images(desc, ptr):
    return [desc[int(ptr[m]):int(ptr[m + 1])] for m in range(len(ptr) - 1)]


def shortlist(ref_desc, ref_ptr, q_desc, q_ptr, query_img=None, max_refs=8, n_probes=256, min_votes=1, ratio=0.8, max_dist2=0, cache=None):
    """dict(shortlist [n_query, R], n_short [n_query], votes [n_query, n_ref]) in the layout api.desc_shortlist returns.  cache: a
    dict that keeps a query image's votes between calls on the same sets and the same (n_probes, ratio, max_dist2)."""
    refs = images(ref_desc, ref_ptr)
    qs = images(q_desc, q_ptr)
    query_img = list(range(len(qs))) if query_img is None else [int(x) for x in query_img]
    V = np.zeros((len(query_img), len(refs)), dtype=np.int32)
    S = np.full((len(query_img), int(max_refs)), -1, dtype=np.int32)
    N = np.zeros(len(query_img), dtype=np.int32)
    for k, img in enumerate(query_img):
        key = (img, int(n_probes), float(ratio), int(max_dist2))
        if cache is not None and key in cache:
            V[k] = cache[key]
        else:
            V[k] = votes_of(qs[img], refs, n_probes, ratio, max_dist2)
            if cache is not None:
                cache[key] = V[k].copy()
        S[k], N[k] = select(V[k], max_refs, min_votes)
    return dict(shortlist=S, n_short=N, votes=V)


def rank_of(votes, r):
    """0-based position of reference r in the vote ranking of one query (len(votes) if it has no vote)."""
    votes = np.asarray(votes, dtype=np.int64)
    if votes[r] < 1:
        return len(votes)
    return int(((votes > votes[r]) | ((votes == votes[r]) & (np.arange(len(votes)) < r))).sum())
