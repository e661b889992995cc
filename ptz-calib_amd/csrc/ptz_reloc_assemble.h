// ptz_reloc_assemble.h -- the contract of the relocalization assembly (ptz_reloc.hip): from the match table of every (reference, query)
// pair to the CSR, cam_ref and cam_cur that the single-view solve, the gate, the trimming loop and the covariance take as they are.
// One header for host and device: integers, and + - * / in double with every product and sum rounded on its own.  The rotation
// matrices of the references are an INPUT (ref_R, Rodrigues of every reference, computed once on the host and uploaded), so a host
// build of this header (tests/cpu_harness/reloc_assemble_harness.cc) gives the device's bits.
//
// Model: all references share one projection centre (this library's rotation-only camera); a pixel of reference r is then a pixel of
// any other pinhole at that centre, whatever the scene's depth.  Translations are carried along and never enter the transfer.
//
// Inputs: a match CSR over n_pair pairs (match_ptr, uv_ref, uv_cur: the layout of ptz_desc_matches_device_ptrs), pair_ref [n_pair]
// the reference image of each pair, query_ptr [n_query + 1] the contiguous pair list of each query, ref_cams [15 n_ref], ref_R [9 n_ref]
// row-major, query_wh [2 n_query], factor_type, K = max_refs >= 1.
//
// Selection.  The pairs of a query are ranked by the unique key (match count descending, position in the list ascending): the
// first-wins tie of FindBestMatch (run_ptz_reloc.cc).  A pair without matches never ranks.  Slots 0 .. n_sel - 1, n_sel <= K, take the
// first K pairs; slot 0 is the ANCHOR.  n_sel = 0: the query is unusable, its output range is empty, and it still gets finite
// cameras -- those of the first reference of its list, or of reference 0 for an empty list.
//
// cam_cur, for every K: what run_ptz_reloc.cc builds -- [f, f, 0.5 w, 0.5 h, rvec, t, dist] with f = fx, rvec, t, dist of the anchor.
//
// K = 1: the output CSR is a copy of the anchor pair's matches, cam_ref the anchor's 15 doubles.
//
// K > 1: cam_ref is the VIRTUAL ANCHOR [fa, fa, S, S, rvec_a, t_a, 0, 0, 0, 0, 0], fa the anchor's fx, S = 8192: a pinhole without
// distortion whose frame [0, 2S)^2 has room for its neighbours' pixels (the distortion variants skip a reference pixel outside
// [0, 2cx) x [0, 2cy), ptz_krt_device.h: with the real anchor they would skip the very matches this is for).  Every match (u, v) of
// every selected pair, the anchor's own included, is transferred:
//   1. factor_type & 1: (ou, ov) = undistort_point(K_r, dist_r, u, v), dropped if outside r's own frame (the solve would have
//      skipped it); otherwise (ou, ov) = (u, v) -- that functor ignores the reference's distortion;
//   2. n = ((ou - cx_r) / fx_r, (ov - cy_r) / fy_r, 1);
//   3. w = R_r^T n, m = R_a w, sums left to right;
//   4. kept iff m_z > 0 and m_x, m_y, m_z finite;
//   5. u' = (float)(fa (m_x / m_z) + S), v' likewise; kept iff 0 <= u', v' < 2S.
// The output holds the kept matches slot after slot, each pair's in their order; out_src their index in the input arrays; uv_cur is
// copied.  For K > 1 the border test of step 1 is the ONLY one a match of view r meets: the solve sees the virtual anchor, whose
// guard is the frame [0, 2S)^2, never view r's.  It is this header's arithmetic (no contraction); the solve's guard on the real
// reference (K = 1, where nothing is transferred) is compiled with the kernels' contraction, so the two may judge a pixel within an
// ulp of the border differently -- such a match is kept by one path and skipped by the other, each consistently.
#pragma once

#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)  // every product and sum rounds on its own; include this header BEFORE ptz_factor.h's other users
#endif

#include "ptz_factor.h"

namespace ptz {

constexpr double kRelocS = 8192.0;

// rank of a pair: larger is better, 0 never ranks.  count < 2^31, pos < 2^31.
PTZ_HD uint64_t reloc_key(int64_t count, int32_t pos)
{
  return count > 0 ? ((uint64_t)count << 31) | (uint64_t)(0x7fffffff - pos) : 0ull;
}
PTZ_HD int32_t reloc_key_pos(uint64_t key) { return 0x7fffffff - (int32_t)(key & 0x7fffffffull); }
PTZ_HD int64_t reloc_key_count(uint64_t key) { return (int64_t)(key >> 31); }

PTZ_HD bool reloc_finite(double v) { return v - v == 0.0; }

struct RelocPixel {
  float u, v;
  bool keep;
};

// steps 1 - 5 for one match of reference r (cam_r its 15 doubles, R_r / R_a row-major), dist = factor_type & 1
PTZ_HD RelocPixel reloc_transfer(const double* cam_r, const double* R_r, const double* R_a, double fa, int dist, float u, float v)
{
  RelocPixel o = {0.f, 0.f, false};
  float ou = u, ov = v;
  if (dist) {
    undistort_point(cam_r[0], cam_r[1], cam_r[2], cam_r[3], cam_r + 10, u, v, ou, ov);
    if (ou < 0 || ou >= cam_r[2] * 2 || ov < 0 || ov >= cam_r[3] * 2) return o;
  }
  const double nx = ((double)ou - cam_r[2]) / cam_r[0], ny = ((double)ov - cam_r[3]) / cam_r[1];
  const double w0 = R_r[0] * nx + R_r[3] * ny + R_r[6];
  const double w1 = R_r[1] * nx + R_r[4] * ny + R_r[7];
  const double w2 = R_r[2] * nx + R_r[5] * ny + R_r[8];
  const double mx = R_a[0] * w0 + R_a[1] * w1 + R_a[2] * w2;
  const double my = R_a[3] * w0 + R_a[4] * w1 + R_a[5] * w2;
  const double mz = R_a[6] * w0 + R_a[7] * w1 + R_a[8] * w2;
  if (!(mz > 0.0) || !reloc_finite(mx) || !reloc_finite(my) || !reloc_finite(mz)) return o;
  o.u = (float)(fa * (mx / mz) + kRelocS);
  o.v = (float)(fa * (my / mz) + kRelocS);
  const float lim = (float)(2.0 * kRelocS);
  o.keep = o.u >= 0.f && o.u < lim && o.v >= 0.f && o.v < lim;
  return o;
}

// the two cameras of a query from the 15 doubles of its anchor (or of its fallback reference, n_sel = 0)
PTZ_HD void reloc_cameras(const double* anchor, int32_t w, int32_t h, int max_refs, double* cam_ref, double* cam_cur)
{
  cam_cur[0] = anchor[0]; cam_cur[1] = anchor[0];
  cam_cur[2] = 0.5 * (double)w; cam_cur[3] = 0.5 * (double)h;
  for (int k = 4; k < 15; ++k) cam_cur[k] = anchor[k];
  if (max_refs == 1) {
    for (int k = 0; k < 15; ++k) cam_ref[k] = anchor[k];
    return;
  }
  cam_ref[0] = anchor[0]; cam_ref[1] = anchor[0];
  cam_ref[2] = kRelocS; cam_ref[3] = kRelocS;
  for (int k = 4; k < 10; ++k) cam_ref[k] = anchor[k];
  for (int k = 10; k < 15; ++k) cam_ref[k] = 0.0;
}

// match count of pair p as the selection sees it: 0 for a malformed range or a reference outside [0, n_ref)
PTZ_HD int64_t reloc_pair_count(const int64_t* match_ptr, const int32_t* pair_ref, int32_t n_ref, int64_t p)
{
  const int64_t c = match_ptr[p + 1] - match_ptr[p];
  const int32_t r = pair_ref[p];
  return (c > 0 && c <= 0x7fffffff && r >= 0 && r < n_ref) ? c : 0;
}

// candidate i of a query (0 <= i < sum of the selected pairs' counts) -> its pair and its index in the input arrays
PTZ_HD void reloc_locate(const int64_t* match_ptr, const int32_t* sel_pair, int32_t n_sel, int64_t i, int32_t* pair, int64_t* src)
{
  int32_t p = sel_pair[0];
  for (int s = 0; s < n_sel; ++s) {
    p = sel_pair[s];
    const int64_t c = match_ptr[p + 1] - match_ptr[p];
    if (i < c || s == n_sel - 1) break;
    i -= c;
  }
  *pair = p;
  *src = match_ptr[p] + i;
}

}  // namespace ptz
