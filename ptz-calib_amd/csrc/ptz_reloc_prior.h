// ptz_reloc_prior.h -- the contract of relocalization from a PRIOR camera (ptz_reloc_prior_pairs, ptz_relocalizer_run_tracked): which
// references a query is worth matching against when its camera is roughly known, the homography each such pair is matched under, and
// what of the prior enters the solve's initial camera.  One header for host and device, in the manner of ptz_reloc_assemble.h:
// integers, and + - * / in double with every product and sum rounded on its own.  The rotation matrices are INPUTS: ref_R is
// ptz_reloc_ref_rotations of the references, prior_R the same function called on the prior cameras, once per run, on the host.  A
// host build of this header (tests/cpu_harness/reloc_prior_harness.cc) therefore gives the device's bits.
//
// Model: rotation-only cameras on one projection centre.  A pixel a of image `from` is the pixel b ~ H a of image `to` with
//   M = R_to R_from^T                     M[i][j] = R_to[3i] R_from[3j] + R_to[3i+1] R_from[3j+1] + R_to[3i+2] R_from[3j+2], left to right
//   N = M K_from^-1, K^-1 written out     N[i][0] = M[i][0] / fx, N[i][1] = M[i][1] / fy, N[i][2] = (M[i][2] - N[i][0] cx) - N[i][1] cy
//   H = K_to N                            H[0][j] = fx' N[0][j] + cx' N[2][j], H[1][j] = fy' N[1][j] + cy' N[2][j], H[2][j] = N[2][j]
// No matrix is inverted.  Swapping the roles gives the other direction: its M is this M transposed bit for bit (the same products,
// summed in the same order).  With reference r as `from` and the query as `to`, H is what ptz_desc_match_pairs_guided takes for the
// relocalizer's pairs (A = reference image, B = query image).
// A reference contributes fx, fy, cx, cy of its 15 doubles.  The query contributes its image centre (0.5 w, 0.5 h), the prior's fx,
// and fy = fx for PTZ_KRT_F / PTZ_KRT_FDist or the prior's fy otherwise: the conventions of reloc_cameras (ptz_reloc_assemble.h).
// DISTORTION DOES NOT ENTER H, of either camera: the matcher's radius absorbs it.
//
// Overlap of (reference r, query q), an int in 0 .. 128: an 8 x 8 lattice of cell centres of the frame [0, W) x [0, H) of r,
// W = 2 cx_r, H = 2 cy_r, point (i, j) the float pixel ((float)(((double)i + 0.5) * W / 8.0), (float)(((double)j + 0.5) * H / 8.0)),
// is warped by desc_guide_warp (the matcher's own function) under H(r -> q); a point counts when ok and 0 <= wx < (float)w_q and
// 0 <= wy < (float)h_q.  To that the count of the query frame's lattice (W = w_q, H = h_q as doubles) under H(q -> r) against
// [0, (float)(2 cx_r)) x [0, (float)(2 cy_r)) is added.  Two directions, because a zoomed-in query inside a wide reference scores
// 64 + few and the converse few + 64: either is a pair worth matching.
//
// Shortlist: sl_takes of ptz_desc_shortlist.h on the overlap scores, min_overlap in the place of min_votes -- references ranked by
// (score descending, index ascending), a score below max(min_overlap, 1) never ranks, the first min(R, ranked) are taken and WRITTEN
// IN ASCENDING INDEX (the order the assembly's first-wins tie depends on).  H_slot [9 R n_query] holds H(r -> q) of each listed slot
// and zeros in the unused ones.
//
// Initial camera: reloc_prior_camera overwrites, in the cam_cur the assembly wrote, the focal (0, 1; fy = fx for F / FDist), the
// rotation vector (4 .. 6) and the distortion (10 .. 14) with the prior's; the image centre (2, 3) and the anchor's t (7 .. 9) stay.
//
// WHY THE TRACKED RUN ALWAYS GATES.  With a radius of tens of pixels a feature whose true partner is absent often has exactly ONE
// admissible candidate: second = INT32_MAX passes the ratio test, and the cross check passes as well.  On repeated texture about
// 4 % of the matches are such neighbours, and the solve's accuracy drops tenfold.  The matcher's contract is right for the 4 px radius
// it was made for and does not change; ptz_relocalizer_run_tracked instead forces the gate on the assembled query (stage 4) on,
// whatever options->inlier_matches says.  options->match.max_dist2, if set, comes on top.
#pragma once

#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)  // every product and sum rounds on its own; include this header BEFORE ptz_factor.h's other users
#endif

#include "ptz_desc_shortlist.h"

namespace ptz {

constexpr int kPriorLattice = 8;
constexpr int32_t kPriorOverlapMax = 2 * kPriorLattice * kPriorLattice;

// F and FDist share one focal; Fxfy and FxfyDist carry fy of their own
PTZ_HD bool prior_one_focal(int32_t factor_type) { return (factor_type & 2) == 0; }

// [fx, fy, cx, cy] of a query from its prior and its image size
PTZ_HD void prior_query_K(const double* prior, int32_t w, int32_t h, int32_t factor_type, double* K4)
{
  K4[0] = prior[0];
  K4[1] = prior_one_focal(factor_type) ? prior[0] : prior[1];
  K4[2] = 0.5 * (double)w;
  K4[3] = 0.5 * (double)h;
}

// cam_from / cam_to: [fx, fy, cx, cy, ..]; R_from / R_to row-major; H row-major, b ~ H a for a in `from`, b in `to`
PTZ_HD void prior_homography(const double* cam_from, const double* R_from, const double* cam_to, const double* R_to, double* H)
{
  double N[9];
  for (int i = 0; i < 3; ++i) {
    const double m0 = R_to[3 * i] * R_from[0] + R_to[3 * i + 1] * R_from[1] + R_to[3 * i + 2] * R_from[2];
    const double m1 = R_to[3 * i] * R_from[3] + R_to[3 * i + 1] * R_from[4] + R_to[3 * i + 2] * R_from[5];
    const double m2 = R_to[3 * i] * R_from[6] + R_to[3 * i + 1] * R_from[7] + R_to[3 * i + 2] * R_from[8];
    N[3 * i] = m0 / cam_from[0];
    N[3 * i + 1] = m1 / cam_from[1];
    N[3 * i + 2] = (m2 - N[3 * i] * cam_from[2]) - N[3 * i + 1] * cam_from[3];
  }
  for (int j = 0; j < 3; ++j) {
    H[j] = cam_to[0] * N[j] + cam_to[2] * N[6 + j];
    H[3 + j] = cam_to[1] * N[3 + j] + cam_to[3] * N[6 + j];
    H[6 + j] = N[6 + j];
  }
}

// lattice points of the frame [0, W) x [0, Hh) that H puts inside [0, w_to) x [0, h_to)
PTZ_HD int32_t prior_lattice_count(const double* H, double W, double Hh, float w_to, float h_to)
{
  int32_t n = 0;
  for (int j = 0; j < kPriorLattice; ++j) {
    const float y = (float)(((double)j + 0.5) * Hh / 8.0);
    for (int i = 0; i < kPriorLattice; ++i) {
      const float x = (float)(((double)i + 0.5) * W / 8.0);
      const DescWarp p = desc_guide_warp(H, x, y);
      n += (p.ok && p.x >= 0.f && p.x < w_to && p.y >= 0.f && p.y < h_to) ? 1 : 0;
    }
  }
  return n;
}

// the score of (reference, query); H_rq: H(reference -> query), the matrix of the listed slot
PTZ_HD int32_t prior_overlap(const double* cam_r, const double* R_r, const double* Kq, const double* R_q, int32_t w_q, int32_t h_q, double* H_rq)
{
  double H_qr[9];
  prior_homography(cam_r, R_r, Kq, R_q, H_rq);
  prior_homography(Kq, R_q, cam_r, R_r, H_qr);
  const double Wr = cam_r[2] * 2.0, Hr = cam_r[3] * 2.0;
  return prior_lattice_count(H_rq, Wr, Hr, (float)w_q, (float)h_q) + prior_lattice_count(H_qr, (double)w_q, (double)h_q, (float)Wr, (float)Hr);
}

// reference r is on the overlap list of a query with these scores
PTZ_HD bool prior_takes(const int32_t* overlap, int32_t n_ref, int32_t r, int32_t R, int32_t min_overlap)
{
  return sl_takes(overlap, n_ref, r, R, min_overlap);
}

// the solve's initial camera: the assembly's cam_cur with the prior's focal, rotation and distortion
PTZ_HD void reloc_prior_camera(double* cam_cur, const double* prior, int32_t factor_type)
{
  cam_cur[0] = prior[0];
  cam_cur[1] = prior_one_focal(factor_type) ? prior[0] : prior[1];
  for (int k = 4; k < 7; ++k) cam_cur[k] = prior[k];
  for (int k = 10; k < 15; ++k) cam_cur[k] = prior[k];
}

}  // namespace ptz
