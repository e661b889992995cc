// ptz_desc_match.h -- the contract of the descriptor matcher (ptz_desc_match_pairs): what a nearest neighbour is, how two partial
// answers combine, and when a pair of features is a match.  All integer but one fp64 multiply on exactly representable integers.
//
// PTZ_HD like ptz_ba_trim.h: the kernels of ptz_desc_match.hip and the host (tests/cpu_harness/desc_match_harness.cc, the host
// library's writer of the transposed pairs) instantiate the same functions.
//
// Descriptors are uint8, D per feature.  d2(i, j) = sum_k (a_ik - b_jk)^2 in int32 (at most 512 * 255^2).
//   best(i)    the j of smallest d2, the lowest j on a tie -- the smallest KEY (d2, j), and keys are unique;
//   second(i)  the smallest d2 over j != best(i) (may equal the best), INT32_MAX if there is no other j.
// A top-2 state is (best d2, best j, second d2); the state of no candidate at all is (INT32_MAX, INT32_MAX, INT32_MAX).  Two states
// over DISJOINT candidate sets merge to the state of the union in any order:
//   best = min(b1, b2) by key, second = min(max(b1, b2).d2, s1, s2).
// (i, j) is a match when j = best_A(i); with cross_check, i = best_B(j); with ratio > 0, (double)d2 < r2 * (double)second_A(i), and
// with cross_check as well (double)d2 < r2 * (double)second_B(j); and max_dist2 == 0 or d2 <= max_dist2.  r2 = ratio * ratio is
// computed once, on the host.
#pragma once

#include <stdint.h>

#if !defined(PTZ_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PTZ_HD __host__ __device__ __forceinline__
#else
#define PTZ_HD inline
#endif
#endif

namespace ptz {

constexpr int32_t kDescNone = INT32_MAX;
constexpr int kDescMaxDim = 512;

struct DescTop2 {
  int32_t d;  // best d2
  int32_t j;  // its feature
  int32_t s;  // second d2
};

struct DescRule {
  double r2;          // ratio^2, 0: no ratio test
  int32_t max_dist2;  // 0: no bound
  int32_t cross_check;
};

PTZ_HD DescTop2 desc_top2_empty() { return DescTop2{kDescNone, kDescNone, kDescNone}; }
PTZ_HD DescTop2 desc_top2_one(int32_t d2, int32_t j) { return DescTop2{d2, j, kDescNone}; }
PTZ_HD bool desc_key_less(int32_t d1, int32_t j1, int32_t d2, int32_t j2) { return d1 < d2 || (d1 == d2 && j1 < j2); }
PTZ_HD int32_t desc_min(int32_t a, int32_t b) { return a < b ? a : b; }

PTZ_HD DescTop2 desc_top2_merge(const DescTop2& a, const DescTop2& b)
{
  const bool a_first = desc_key_less(a.d, a.j, b.d, b.j);
  DescTop2 r;
  r.d = a_first ? a.d : b.d;
  r.j = a_first ? a.j : b.j;
  r.s = desc_min(a_first ? b.d : a.d, desc_min(a.s, b.s));
  return r;
}

PTZ_HD bool desc_ratio_ok(double r2, int32_t d2, int32_t second) { return !(r2 > 0.0) || (double)d2 < r2 * (double)second; }

// feature i of A with its state ta; tb: the state of B's feature ta.j (read only when ta.j is a feature, i.e. B is not empty)
PTZ_HD bool desc_accept(const DescRule& r, int32_t i, const DescTop2& ta, const DescTop2& tb)
{
  if (ta.j == kDescNone) return false;
  if (r.cross_check && tb.j != i) return false;
  if (!desc_ratio_ok(r.r2, ta.d, ta.s)) return false;
  if (r.cross_check && !desc_ratio_ok(r.r2, ta.d, tb.s)) return false;
  return r.max_dist2 == 0 || ta.d <= r.max_dist2;
}

// ---- guided matching (ptz_desc_match_pairs_guided): the same rule over the candidates a pair homography admits -------------------
// The pair (i of A, j of B) is ADMISSIBLE under H (b ~ H a, row-major) and a radius when H puts a_i in front of the camera and within
// the radius of b_j, the error measured in B's image:
//   warp        X = H0 x + H1 y + H2 in double, left to right, every product and sum rounded on its own (no fma); Y and Z likewise;
//               ok = Z > 0 and X, Y, Z finite; wx = (float)(X / Z), wy = (float)(Y / Z);
//   admissible  dx = wx - bx, dy = wy - by, e2 = dx dx + dy dy in float (three roundings, no fma), e2 <= r2f -- inclusive, false for
//               a NaN; r2f = (float)(radius_px * radius_px), computed once on the host.
// ONE predicate serves both directions: B's features ask A over the same admissible set (A's warped points against b_j), so
//   * best, second, ties, the ratio test, cross_check, max_dist2 and min_matches are the rules above over the admissible candidates
//     only (second = INT32_MAX with fewer than two of them);
//   * the matches of (B, A) under the SAME H and roles are the transposed matches of (A, B); a call with the roles swapped and
//     H^-1 measures the error in the other image, is another predicate and need not be;
//   * a pair's result depends on its two images and its H only;
//   * a radius that admits every candidate gives the unguided result, array-equal.
#if defined(__clang__)
#pragma clang fp contract(off)  // every product and sum rounds on its own, as numpy's
#endif

struct DescWarp {
  float x, y;
  bool ok;
};

PTZ_HD bool desc_finite(double v) { return v - v == 0.0; }  // (inf - inf and NaN - NaN are NaN)

PTZ_HD DescWarp desc_guide_warp(const double* H, float x, float y)
{
  const double ax = x, ay = y;
  const double X = H[0] * ax + H[1] * ay + H[2];
  const double Y = H[3] * ax + H[4] * ay + H[5];
  const double Z = H[6] * ax + H[7] * ay + H[8];
  DescWarp w;
  w.ok = Z > 0.0 && desc_finite(X) && desc_finite(Y) && desc_finite(Z);
  w.x = (float)(X / Z);
  w.y = (float)(Y / Z);
  return w;
}

PTZ_HD float desc_guide_err2(float wx, float wy, float bx, float by)
{
  const float dx = wx - bx, dy = wy - by;
  return dx * dx + dy * dy;
}

PTZ_HD bool desc_guide_admissible(float wx, float wy, float bx, float by, float r2f) { return desc_guide_err2(wx, wy, bx, by) <= r2f; }

// d2 of two packed rows (ptz_desc_match.hip's pack: bytes are a - 128 as int8, zero padding) from their norms: |a'|^2 + |b'|^2 - 2 a'.b'
PTZ_HD int32_t desc_dot_i8x4(uint32_t a, uint32_t b)
{
  int32_t s = 0;
  for (int k = 0; k < 4; ++k) s += (int32_t)(int8_t)(a >> (8 * k)) * (int32_t)(int8_t)(b >> (8 * k));
  return s;
}

}  // namespace ptz
