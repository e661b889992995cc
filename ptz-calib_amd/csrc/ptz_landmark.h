// ptz_landmark.h -- the contract of the landmark map (ptz_landmark.hip): one unit ray and one descriptor per TRACK of the reference
// images, and the assembly that turns the matches of (map, query) pairs into the CSR, cam_ref and cam_cur the single-view solve, the
// gate, the trimming loop and the covariance take as they are.  One header for host and device, in the style of
// ptz_reloc_assemble.h: integers, and + - * / and sqrt in double with every operation rounded on its own (sqrt is correctly rounded
// on both sides).  The rotation matrices of the references are an INPUT (ptz_reloc_ref_rotations), so a host build of this header
// (tests/cpu_harness/landmark_harness.cc) gives the device's bits and numpy restates it exactly (tests/landmark_util.py).
//
// Model: all references share one projection centre, so a track -- the pixels of one world point in several references -- has ONE
// 3-D quantity, a unit ray from that centre.
//
// MAP BUILD.  Inputs: the references' descriptors (uint8 [n_feat, D], image m owning features feat_ptr[m] ..) and key points,
// ref_cams [15 n_ref], ref_R [9 n_ref] row-major, tracks as CSR (trk_ptr [n_track + 1], trk_img, trk_feat: the feature's index
// INSIDE its image), dist = factor_type & 1, min_views >= 1.  Per track, over its views in CSR order:
//   - a view (r, f) is VALID iff 0 <= r < n_ref, 0 <= f < the features of image r and, with dist, its undistorted pixel lies inside
//     r's frame [0, 2cx) x [0, 2cy) (steps 1 - 2 of reloc_transfer);
//   - n = ((ou - cx_r) / fx_r, (ov - cy_r) / fy_r, 1), w = R_r^T n (sums left to right), ray = w / sqrt(w . w);
//   - s = the sum of ray over the valid views, left to right from (0, 0, 0); L = s / sqrt(s . s);
//   - the track is a LANDMARK iff it has at least min_views valid views and L is finite (opposite rays that cancel give 0 / 0);
//   - descriptor byte k = (2 S_k + n) / (2 n) in integer division, S_k the int32 sum of byte k over the n valid views: the mean,
//     rounded, halves up;
//   - home = the valid view with the largest z = (R_r L)_z = R_r[6] L_x + R_r[7] L_y + R_r[8] L_z: the best z starts at -inf, a
//     view takes over iff its z is GREATER (the first in CSR order wins a tie); if none does, the first valid view.  lm_home is
//     that view's reference image.
// Landmarks are compacted in ascending track order: n_lm, lm_track, lm_ray [3 n_lm], lm_home, lm_views (the n above), lm_desc.
//
// ASSEMBLY.  Pair q is (map, query q).  Inputs: the matcher's CSR of those n_query pairs (match_ptr, idx_a: the landmark index,
// uv_b: the query's pixel), the map's lm_ray / lm_home, ref_cams, ref_R, query_wh, factor_type.
//   - a match VOTES for lm_home[idx_a] iff 0 <= idx_a < n_lm and the home is in [0, n_ref); the ANCHOR of a query is the reference
//     with the most votes, the lowest index on a tie (integer counts: the order of counting cannot matter); no vote: anchor = -1,
//     an empty range, and the finite cameras of reference 0;
//   - cam_ref, cam_cur = reloc_cameras(anchor, w, h, 2, ..): the virtual anchor [fa, fa, S, S, rvec_a, t_a, 0 x 5] and the tool's
//     initial camera;
//   - a voting match is transferred: m = R_a L (sums left to right), kept iff m_z > 0 and m finite; u' = (float)(fa (m_x / m_z) + S),
//     v' likewise, kept iff 0 <= u', v' < 2S (steps 4 - 5 of reloc_transfer, restated here: that header stays as it is);
//   - outputs in the layout of ptz_reloc_assemble: anchor_ref [n_query], out_ptr, out_uv_ref (u', v'), out_uv_cur (uv_b copied),
//     out_src (index in the input arrays), cam_ref, cam_cur.  A query's output depends on its own matches and the map only.
#pragma once

#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)  // every product and sum rounds on its own; include this header BEFORE ptz_factor.h's other users
#endif

#include "ptz_reloc_assemble.h"

namespace ptz {

constexpr int32_t kLandmarkMaxRefs = 8192;  // the anchor vote keeps one int32 counter per reference in LDS: 32 KB

// the unit ray of pixel (u, v) of reference r; false: the view is not valid (dist only: the undistorted pixel leaves r's frame)
PTZ_HD bool landmark_view_ray(const double* cam_r, const double* R_r, int dist, float u, float v, double* ray)
{
  float ou = u, ov = v;
  if (dist) {
    undistort_point(cam_r[0], cam_r[1], cam_r[2], cam_r[3], cam_r + 10, u, v, ou, ov);
    if (ou < 0 || ou >= cam_r[2] * 2 || ov < 0 || ov >= cam_r[3] * 2) return false;
  }
  const double nx = ((double)ou - cam_r[2]) / cam_r[0], ny = ((double)ov - cam_r[3]) / cam_r[1];
  const double w0 = R_r[0] * nx + R_r[3] * ny + R_r[6];
  const double w1 = R_r[1] * nx + R_r[4] * ny + R_r[7];
  const double w2 = R_r[2] * nx + R_r[5] * ny + R_r[8];
  const double len = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
  ray[0] = w0 / len; ray[1] = w1 / len; ray[2] = w2 / len;
  return true;
}

// L = s / |s|; false: not finite
PTZ_HD bool landmark_unit(const double* s, double* L)
{
  const double len = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
  L[0] = s[0] / len; L[1] = s[1] / len; L[2] = s[2] / len;
  return reloc_finite(L[0]) && reloc_finite(L[1]) && reloc_finite(L[2]);
}

// the home search's score of a view of reference r
PTZ_HD double landmark_home_z(const double* R_r, const double* L) { return R_r[6] * L[0] + R_r[7] * L[1] + R_r[8] * L[2]; }

// the rounded mean of n >= 1 bytes whose sum is S, halves up
PTZ_HD uint8_t landmark_desc_byte(int32_t S, int32_t n) { return (uint8_t)((2 * S + n) / (2 * n)); }

// a landmark's ray as a pixel of the virtual anchor (R_a row-major, fa the anchor's fx)
PTZ_HD RelocPixel landmark_transfer(const double* R_a, double fa, const double* L)
{
  RelocPixel o = {0.f, 0.f, false};
  const double mx = R_a[0] * L[0] + R_a[1] * L[1] + R_a[2] * L[2];
  const double my = R_a[3] * L[0] + R_a[4] * L[1] + R_a[5] * L[2];
  const double mz = R_a[6] * L[0] + R_a[7] * L[1] + R_a[8] * L[2];
  if (!(mz > 0.0) || !reloc_finite(mx) || !reloc_finite(my) || !reloc_finite(mz)) return o;
  o.u = (float)(fa * (mx / mz) + kRelocS);
  o.v = (float)(fa * (my / mz) + kRelocS);
  const float lim = (float)(2.0 * kRelocS);
  o.keep = o.u >= 0.f && o.u < lim && o.v >= 0.f && o.v < lim;
  return o;
}

// does match i vote, and for which reference (-1: it does not)
PTZ_HD int32_t landmark_vote(const int32_t* idx_a, const int32_t* lm_home, int32_t n_lm, int32_t n_ref, int64_t i)
{
  const int32_t l = idx_a[i];
  if (l < 0 || l >= n_lm) return -1;
  const int32_t r = lm_home[l];
  return (r >= 0 && r < n_ref) ? r : -1;
}

// rank of a reference in the anchor vote: larger is better, 0 never ranks.  count < 2^31, r < 2^31.
PTZ_HD uint64_t landmark_anchor_key(int32_t count, int32_t r) { return reloc_key((int64_t)count, r); }

}  // namespace ptz
