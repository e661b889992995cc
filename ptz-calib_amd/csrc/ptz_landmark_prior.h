// ptz_landmark_prior.h -- the contract of the landmark VIEW (ptz_landmark_prior.hip): which landmarks of a map a query can see when
// its camera is roughly known, and where.  One header for host and device, in the style of ptz_landmark.h: + - * / in double with
// every operation rounded on its own.  The rotation matrices are an INPUT: prior_R is ptz_reloc_ref_rotations of the prior cameras,
// once per run, on the host.  A host build of this header (tests/cpu_harness/landmark_prior_harness.cc) therefore gives the device's
// bits and numpy restates it exactly (tests/landmark_prior_util.py).
//
// Model: a landmark is a unit ray L from the shared projection centre, so under a prior (K_q, R_q) its pixel in the query is
// K_q R_q L.  No homography, no reference image and no reference-side distortion enter.
//
// PREDICTION.  m = R_q L, every row summed left to right as in landmark_transfer; ok = m_z > 0 and m finite;
//   px = fx (m_x / m_z) + 0.5 w,  py = fy (m_y / m_z) + 0.5 h
// with [fx, fy, 0.5 w, 0.5 h] = prior_query_K (ptz_reloc_prior.h): the prior's fx, fy = fx for F / FDist and the prior's fy
// otherwise, the image centre from the query's size.  THE PRIOR'S DISTORTION DOES NOT ENTER: the radius absorbs it, as it does in
// the tracked run.
//
// VISIBILITY.  Landmark l is visible in query q iff ok, -radius_px <= px < w + radius_px and -radius_px <= py < h + radius_px, the
// comparisons on the doubles (w + radius_px one rounded sum).  Its position is ((float)px, (float)py).
//
// VIEW.  The view of query q is its visible landmarks in ASCENDING landmark index: vis_ptr [n_query + 1], vis_lm [n_vis],
// vis_uv [n_vis, 2].  A query's view depends on its own prior, its image size and the map only.
//
// MATCHES.  The matches of (map, q) are those of ptz_desc_match.h's guided contract for the pair (view image q, query image q)
// with H = identity, radius_px and found = NULL: the identity warp returns a float pixel unchanged.  The lowest view-local index on
// a tie is the lowest landmark index.  The visibility rule is part of the contract: a landmark outside it is never a candidate,
// wherever the query's key points are.
#pragma once

#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)  // every product and sum rounds on its own; include this header BEFORE ptz_factor.h's other users
#endif

#include "ptz_landmark.h"
#include "ptz_reloc_prior.h"

namespace ptz {

struct LandmarkSeen {
  float u, v;
  bool visible;
};

// K4 = prior_query_K of the query; R_q row-major; L the landmark's ray
PTZ_HD LandmarkSeen landmark_predict(const double* K4, const double* R_q, int32_t w, int32_t h, double radius_px, const double* L)
{
  LandmarkSeen o = {0.f, 0.f, false};
  const double mx = R_q[0] * L[0] + R_q[1] * L[1] + R_q[2] * L[2];
  const double my = R_q[3] * L[0] + R_q[4] * L[1] + R_q[5] * L[2];
  const double mz = R_q[6] * L[0] + R_q[7] * L[1] + R_q[8] * L[2];
  if (!(mz > 0.0) || !reloc_finite(mx) || !reloc_finite(my) || !reloc_finite(mz)) return o;
  const double px = K4[0] * (mx / mz) + K4[2];
  const double py = K4[1] * (my / mz) + K4[3];
  const double lo = -radius_px, hx = (double)w + radius_px, hy = (double)h + radius_px;
  o.visible = px >= lo && px < hx && py >= lo && py < hy;
  o.u = (float)px;
  o.v = (float)py;
  return o;
}

}  // namespace ptz
