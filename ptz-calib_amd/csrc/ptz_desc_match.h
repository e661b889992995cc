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

}  // namespace ptz
