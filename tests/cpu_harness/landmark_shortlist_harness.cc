// landmark_shortlist_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of the landmark shortlist's contract in
// ptz-calib_amd/csrc/ptz_landmark_shortlist.h (what ptz_landmark_shortlist.hip spreads over lanes, tiles and queries): the home
// groups, the votes and lists of ptz_desc_shortlist.h over the grouped rows (a top-2 per probe and home merged from partial states
// in a scrambled order), and the view of a list through the bitmap over homes -- so it can be held to a numpy restatement without a
// GPU.  Never part of the product library.  With LANDMARK_SHORTLIST_HARNESS_MAIN it is a stand-alone program (for a sanitizer
// build): generated maps and lists against a plain scan; returns 0 if they agree.
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../ptz-calib_amd/csrc/ptz_landmark_shortlist.h"

using namespace ptz;

namespace {

int32_t d2_of(const uint8_t* a, const uint8_t* b, int D)
{
  int32_t s = 0;
  for (int k = 0; k < D; ++k) { const int32_t d = (int32_t)a[k] - (int32_t)b[k]; s += d * d; }
  return s;
}

}  // namespace

extern "C" {
// home [n_lm] -> home_ptr [n_ref + 1], home_lm [n_lm]; 0, or -1 for a home outside [0, n_ref)
int32_t h_lm_home_groups(const int32_t* home, int32_t n_lm, int32_t n_ref, int64_t* home_ptr, int32_t* home_lm)
{
  return lm_home_groups(home, n_lm, n_ref, home_ptr, home_lm) ? 0 : -1;
}

// One query image q [n, D] against the home set of the map (lm_desc [n_lm, D], home [n_lm]).  votes [n_ref], shortlist [R] (-1 in
// unused slots).  Returns n_short, or -1 for a home out of range.
int32_t h_lm_shortlist(const uint8_t* lm_desc, const int32_t* home, int32_t n_lm, int32_t n_ref, const uint8_t* q, int32_t n, int32_t D, int32_t M,
                       int32_t R, int32_t min_votes, double ratio, int32_t max_dist2, uint64_t seed, int32_t parts, int32_t* votes,
                       int32_t* shortlist)
{
  uint64_t s = seed * 2862933555777941757ull + 3037000493ull;
  auto next = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
  std::vector<int64_t> ptr((size_t)n_ref + 1);
  std::vector<int32_t> lm((size_t)(n_lm > 0 ? n_lm : 1));
  if (!lm_home_groups(home, n_lm, n_ref, ptr.data(), lm.data())) return -1;
  if (parts < 1) parts = 1;
  const int32_t m = sl_probe_count(n, M);
  const double r2 = ratio * ratio;
  for (int32_t r = 0; r < n_ref; ++r) {
    int32_t count = 0;
    for (int32_t k = 0; k < m; ++k) {
      const uint8_t* a = q + (size_t)sl_probe_feature(k, n, M) * D;
      // image-local feature j of home r is landmark lm[ptr[r] + j]; the candidates are dealt to `parts` partial states
      std::vector<DescTop2> part((size_t)parts, desc_top2_empty());
      for (int64_t j = 0; j < ptr[r + 1] - ptr[r]; ++j) {
        const DescTop2 one = desc_top2_one(d2_of(a, lm_desc + (size_t)lm[ptr[r] + j] * D, D), (int32_t)j);
        DescTop2& p = part[next() % parts];
        p = (next() & 1) ? desc_top2_merge(p, one) : desc_top2_merge(one, p);
      }
      DescTop2 t = desc_top2_empty();
      for (int p = 0; p < parts; ++p) t = (next() & 1) ? desc_top2_merge(t, part[p]) : desc_top2_merge(part[p], t);
      count += sl_votes_for(r2, max_dist2, t) ? 1 : 0;
    }
    votes[r] = count;
  }
  int32_t taken = 0;
  for (int32_t r = 0; r < n_ref; ++r)
    if (sl_takes(votes, n_ref, r, R, min_votes)) shortlist[taken++] = r;
  for (int32_t k = taken; k < R; ++k) shortlist[k] = -1;
  return taken;
}

// The views of lists [n_query, R]: vis_ptr [n_query + 1], vis_lm (room for n_query n_lm).  device_form = 0: an entry that is
// neither -1 nor a home is -1 (PTZ_EINVAL) and nothing is written; 1: it is ignored.  n_ref <= 32 kLmHomeWords.
int32_t h_lm_view(const int32_t* home, int32_t n_lm, int32_t n_ref, int32_t n_query, int32_t R, const int32_t* lists, int32_t device_form,
                  int64_t* vis_ptr, int32_t* vis_lm)
{
  if (n_ref > 32 * kLmHomeWords) return -5;
  if (!device_form)
    for (int64_t k = 0; k < (int64_t)n_query * R; ++k)
      if (!lm_home_entry_ok(lists[k], n_ref)) return -1;
  vis_ptr[0] = 0;
  for (int32_t q = 0; q < n_query; ++q) {
    uint32_t bits[kLmHomeWords];
    for (int32_t w = 0; w < kLmHomeWords; ++w) bits[w] = 32 * w < n_ref ? lm_home_word(lists + (int64_t)q * R, R, n_ref, w) : 0u;
    int64_t o = vis_ptr[q];
    for (int32_t l = 0; l < n_lm; ++l)
      if (lm_home_listed(bits, n_ref, home[l])) vis_lm[o++] = l;
    vis_ptr[q + 1] = o;
  }
  return 0;
}
}

#ifdef LANDMARK_SHORTLIST_HARNESS_MAIN
int main()
{
  uint64_t s = 11;
  auto next = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
  int bad = 0;
  for (int n_ref : {1, 5, 23, 40, 8192})
    for (int n_lm : {0, 1, 17, 257, 1025}) {
      std::vector<int32_t> home((size_t)n_lm + 1);
      for (int l = 0; l < n_lm; ++l) home[l] = (int32_t)(next() % n_ref) / 2 * 2 % n_ref;  // (odd homes mostly empty)
      std::vector<int64_t> ptr((size_t)n_ref + 1);
      std::vector<int32_t> lm((size_t)n_lm + 1);
      if (h_lm_home_groups(home.data(), n_lm, n_ref, ptr.data(), lm.data()) != 0) { printf("groups failed\n"); ++bad; continue; }
      // a plain scan: group r is the landmarks of home r in order
      int64_t at = 0;
      for (int r = 0; r < n_ref; ++r) {
        if (ptr[r] != at) { printf("home_ptr differs at n_ref = %d, n_lm = %d\n", n_ref, n_lm); ++bad; break; }
        for (int l = 0; l < n_lm; ++l)
          if (home[l] == r && lm[at++] != l) { printf("home_lm differs at n_ref = %d, n_lm = %d\n", n_ref, n_lm); ++bad; break; }
      }
      if (ptr[n_ref] != n_lm) { printf("home_ptr does not close at n_ref = %d, n_lm = %d\n", n_ref, n_lm); ++bad; }
      for (int R : {1, 3, 9}) {
        const int nq = 4;
        std::vector<int32_t> lists((size_t)nq * R);
        for (auto& e : lists) e = (next() % 4 == 0) ? -1 : (int32_t)(next() % n_ref);
        lists[0] = lists[R - 1];  // a duplicate
        std::vector<int64_t> vp(nq + 1);
        std::vector<int32_t> vl((size_t)nq * n_lm + 1);
        if (h_lm_view(home.data(), n_lm, n_ref, nq, R, lists.data(), 0, vp.data(), vl.data()) != 0) { printf("view failed\n"); ++bad; continue; }
        int64_t o = 0;
        for (int q = 0; q < nq; ++q) {
          for (int l = 0; l < n_lm; ++l) {
            bool in = false;
            for (int k = 0; k < R; ++k) in = in || lists[(size_t)q * R + k] == home[l];
            if (in && vl[o++] != l) { printf("vis_lm differs at n_ref = %d, n_lm = %d, R = %d\n", n_ref, n_lm, R); ++bad; break; }
          }
          if (vp[q + 1] != o) { printf("vis_ptr differs at n_ref = %d, n_lm = %d, R = %d\n", n_ref, n_lm, R); ++bad; break; }
        }
        lists[1 % lists.size()] = n_ref;  // out of range: the host form refuses, the device form ignores
        if (h_lm_view(home.data(), n_lm, n_ref, nq, R, lists.data(), 0, vp.data(), vl.data()) != -1) { printf("bad entry accepted\n"); ++bad; }
        if (h_lm_view(home.data(), n_lm, n_ref, nq, R, lists.data(), 1, vp.data(), vl.data()) != 0) { printf("bad entry not ignored\n"); ++bad; }
      }
      // votes against a plain scan (small maps only)
      if (n_ref <= 40 && n_lm <= 257) {
        const int D = 16, n = 20, M = 7, R = 3;
        std::vector<uint8_t> desc((size_t)n_lm * D + 1), q((size_t)n * D);
        for (auto& v : desc) v = (uint8_t)next();
        for (auto& v : q) v = (uint8_t)next();
        for (int l = 0; l < n_lm; l += 2) std::copy(q.begin() + (size_t)(l % n) * D, q.begin() + (size_t)(l % n + 1) * D, desc.begin() + (size_t)l * D);
        std::vector<int32_t> votes(n_ref), list(R), want(n_ref, 0);
        const int32_t got = h_lm_shortlist(desc.data(), home.data(), n_lm, n_ref, q.data(), n, D, M, R, 1, 0.8, 0, next(), 1 + next() % 4, votes.data(),
                                           list.data());
        for (int k = 0; k < M; ++k) {
          const int f = k * n / M;
          for (int r = 0; r < n_ref; ++r) {
            int32_t bd = INT32_MAX, sd = INT32_MAX;
            bool any = false;
            for (int l = 0; l < n_lm; ++l) {
              if (home[l] != r) continue;
              any = true;
              const int32_t d = d2_of(q.data() + (size_t)f * D, desc.data() + (size_t)l * D, D);
              if (d < bd) { sd = bd; bd = d; }
              else if (d < sd) sd = d;
            }
            if (any && (double)bd < 0.8 * 0.8 * (double)sd) ++want[r];
          }
        }
        if (want != votes) { printf("votes differ at n_ref = %d, n_lm = %d\n", n_ref, n_lm); ++bad; }
        if (got < 0 || got > R) { printf("n_short out of range\n"); ++bad; }
      }
    }
  printf("landmark_shortlist_harness: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
#endif
