// ptz_desc_shortlist.h -- the contract of the reference shortlist (ptz_desc_shortlist): which features of a query are its probes,
// when a probe votes for a reference, and which references the votes select.  All integer but the one fp64 multiply of
// desc_ratio_ok (ptz_desc_match.h), whose top-2 state and merge rule this header builds on.
//
// PTZ_HD like ptz_desc_match.h: the kernels of ptz_desc_shortlist.hip and the host (tests/cpu_harness/desc_shortlist_harness.cc)
// instantiate the same functions.
//
//   probes     a query image with n features and a budget M >= 1 has m = min(n, M) probes; probe k is feature k if n <= M, else
//              feature floor(k n / M) in int64: strictly increasing, in file order (the set carries no scale or response to sort by).
//   vote       probe i votes for reference r when its top-2 over ALL features of r (the state of ptz_desc_match.h: lowest j on a
//              tie, second = INT32_MAX with one candidate) has a feature, passes the ratio test and, with max_dist2 != 0, the bound.
//              One direction: cross_check and min_matches do not enter.  votes[q, r] counts the voting probes.
//   shortlist  references ranked by (votes descending, index ascending); fewer than max(min_votes, 1) votes never rank; the first
//              min(R, ranked) are taken and WRITTEN IN ASCENDING INDEX (the order ptz_reloc_assemble's first-wins tie depends on).
// A query's result depends on its own image, the reference set and the options only.
#pragma once

#include "ptz_desc_match.h"

namespace ptz {

PTZ_HD int32_t sl_probe_count(int32_t n, int32_t M) { return n < M ? n : M; }

// feature of probe k, 0 <= k < sl_probe_count(n, M)
PTZ_HD int32_t sl_probe_feature(int32_t k, int32_t n, int32_t M) { return n <= M ? k : (int32_t)((int64_t)k * (int64_t)n / (int64_t)M); }

// t: the probe's top-2 over all features of one reference
PTZ_HD bool sl_votes_for(double r2, int32_t max_dist2, const DescTop2& t)
{
  if (t.j == kDescNone) return false;
  if (!desc_ratio_ok(r2, t.d, t.s)) return false;
  return max_dist2 == 0 || t.d <= max_dist2;
}

PTZ_HD int32_t sl_need(int32_t min_votes) { return min_votes > 1 ? min_votes : 1; }

// (va, ra) ranks before (vb, rb); keys are unique
PTZ_HD bool sl_ranks_before(int32_t va, int32_t ra, int32_t vb, int32_t rb) { return va > vb || (va == vb && ra < rb); }

// reference r is on the shortlist of a query with these votes: it ranks, and fewer than R references rank before it (counting:
// whatever ranks before a reference with enough votes has enough votes itself)
PTZ_HD bool sl_takes(const int32_t* votes, int32_t n_ref, int32_t r, int32_t R, int32_t min_votes)
{
  const int32_t v = votes[r];
  if (v < sl_need(min_votes)) return false;
  int32_t before = 0;
  for (int32_t o = 0; o < n_ref; ++o) before += sl_ranks_before(votes[o], o, v, r) ? 1 : 0;
  return before < R;
}

#if defined(__HIPCC__)
// One wave writes a query's list: the references sl_takes takes on v [n_ref] go to out [R] in ascending index (a ballot prefix per
// group of 64), -1 to the unused slots; each(slot, r) runs in the lane that owns a taken reference.  Returns the count, one value in
// the wave (at most R: keys are unique).  The ranking of k_desc_shortlist (votes) and of k_reloc_prior (overlap scores).
template <class Each>
__device__ __forceinline__ int sl_wave_list(const int32_t* v, int n_ref, int R, int min_votes, int lane, int32_t* out, Each each)
{
  int taken = 0;
  for (int r0 = 0; r0 < n_ref; r0 += 64) {
    const int r = r0 + lane;
    const bool take = r < n_ref && sl_takes(v, n_ref, r, R, min_votes);
    const unsigned long long mask = __ballot(take);
    if (take) {
      const int s = taken + __popcll(mask & ((1ull << lane) - 1ull));
      out[s] = r;
      each(s, r);
    }
    taken += __popcll(mask);
  }
  for (int s = taken + lane; s < R; s += 64) out[s] = -1;
  return taken;
}
#endif

}  // namespace ptz
