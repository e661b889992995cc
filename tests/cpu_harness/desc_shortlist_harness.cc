// desc_shortlist_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of the reference shortlist's contract in
// ptz-calib_amd/csrc/ptz_desc_shortlist.h (what k_desc_votes / k_desc_shortlist of ptz_desc_shortlist.hip spread over lanes, tiles
// and reference groups): the probe rule, a top-2 per probe and reference built by merging partial states in a scrambled order, the
// vote rule, the ranking by counting -- so it can be held to a numpy restatement without a GPU.  Never part of the product library.
// With DESC_SHORTLIST_HARNESS_MAIN it is a stand-alone program (for a sanitizer build): generated queries against a plain scan and
// a sort; returns 0 if they agree.
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../ptz-calib_amd/csrc/ptz_desc_shortlist.h"

using namespace ptz;

namespace {

int32_t d2_of(const uint8_t* a, const uint8_t* b, int D)
{
  int32_t s = 0;
  for (int k = 0; k < D; ++k) { const int32_t d = (int32_t)a[k] - (int32_t)b[k]; s += d * d; }
  return s;
}

// the top-2 of one row against b: candidates dealt to `parts` partial states, both orders scrambled by the generator
template <class Next>
DescTop2 top2_scrambled(const uint8_t* a, const uint8_t* b, int nb, int D, int parts, Next& next)
{
  std::vector<int> order(nb), pord(parts);
  std::vector<DescTop2> part(parts, desc_top2_empty());
  for (int j = 0; j < nb; ++j) order[j] = j;
  for (int j = nb - 1; j > 0; --j) std::swap(order[j], order[next() % (j + 1)]);
  for (int x = 0; x < nb; ++x) {
    const int j = order[x], p = next() % parts;
    const DescTop2 one = desc_top2_one(d2_of(a, b + (size_t)j * D, D), j);
    part[p] = (next() & 1) ? desc_top2_merge(part[p], one) : desc_top2_merge(one, part[p]);
  }
  for (int p = 0; p < parts; ++p) pord[p] = p;
  for (int p = parts - 1; p > 0; --p) std::swap(pord[p], pord[next() % (p + 1)]);
  DescTop2 t = desc_top2_empty();
  for (int p = 0; p < parts; ++p) t = (next() & 1) ? desc_top2_merge(t, part[pord[p]]) : desc_top2_merge(part[pord[p]], t);
  return t;
}

}  // namespace

extern "C" {
// One query image q [n, D] against the references ref [ref_ptr[n_ref], D].  probes [min(n, M)], votes [n_ref], shortlist [R] (-1 in
// unused slots).  *n_probe: the number of probes.  Returns n_short.
int32_t h_desc_shortlist(const uint8_t* ref, const int64_t* ref_ptr, int32_t n_ref, const uint8_t* q, int32_t n, int32_t D, int32_t M, int32_t R,
                         int32_t min_votes, double ratio, int32_t max_dist2, uint64_t seed, int32_t parts, int32_t* n_probe, int32_t* probes,
                         int32_t* votes, int32_t* shortlist)
{
  uint64_t s = seed * 2862933555777941757ull + 3037000493ull;
  auto next = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
  const int32_t m = sl_probe_count(n, M);
  *n_probe = m;
  for (int32_t k = 0; k < m; ++k) probes[k] = sl_probe_feature(k, n, M);
  const double r2 = ratio * ratio;
  for (int32_t r = 0; r < n_ref; ++r) {
    const int nb = (int)(ref_ptr[r + 1] - ref_ptr[r]);
    int32_t count = 0;
    for (int32_t k = 0; k < m; ++k) {
      const DescTop2 t = top2_scrambled(q + (size_t)probes[k] * D, ref + (size_t)ref_ptr[r] * D, nb, D, parts < 1 ? 1 : parts, next);
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
}

#ifdef DESC_SHORTLIST_HARNESS_MAIN
int main()
{
  uint64_t s = 7;
  auto next = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
  int bad = 0;
  const int ns[] = {0, 1, 15, 16, 17, 49};
  const int Ms[] = {1, 16, 17, 100};
  for (int D : {1, 32, 130})
    for (int n : ns)
      for (int M : Ms)
        for (int R : {1, 3, 9}) {
          const int n_ref = 6;
          std::vector<int64_t> ptr(n_ref + 1, 0);
          for (int r = 0; r < n_ref; ++r) ptr[r + 1] = ptr[r] + (r == 2 ? 0 : 1 + next() % 40);
          std::vector<uint8_t> ref((size_t)ptr[n_ref] * D + 1), q((size_t)n * D + 1);
          for (auto& v : ref) v = (uint8_t)(D == 1 ? next() % 4 : next());
          for (auto& v : q) v = (uint8_t)(D == 1 ? next() % 4 : next());
          // near copies, so that something passes the ratio test; reference 4 is reference 1 again where it fits (tied votes)
          for (int r = 0; r < n_ref && n > 0; ++r)
            for (int64_t j = ptr[r]; j < ptr[r + 1]; j += 3) std::copy(q.begin() + (size_t)(j % n) * D, q.begin() + (size_t)(j % n + 1) * D, ref.begin() + (size_t)j * D);
          const int min_votes = next() % 3;
          const double ratio = (next() & 1) ? 0.8 : 0.0;
          std::vector<int32_t> probes(M + 1), votes(n_ref), list(R);
          int32_t m = 0;
          const int32_t got = h_desc_shortlist(ref.data(), ptr.data(), n_ref, q.data(), n, D, M, R, min_votes, ratio, 0, next(), 1 + next() % 5, &m,
                                               probes.data(), votes.data(), list.data());
          // a plain scan and a sort
          std::vector<int32_t> want(n_ref, 0);
          const int wm = n < M ? n : M;
          if (m != wm) { printf("probe count differs at n = %d, M = %d\n", n, M); ++bad; continue; }
          for (int k = 0; k < wm; ++k) {
            const int f = n <= M ? k : (int)((long long)k * n / M);
            if (probes[k] != f || f >= n || (k > 0 && probes[k] <= probes[k - 1])) { printf("probe differs at n = %d, M = %d\n", n, M); ++bad; break; }
            for (int r = 0; r < n_ref; ++r) {
              int32_t bd = INT32_MAX, sd = INT32_MAX;
              for (int64_t j = ptr[r]; j < ptr[r + 1]; ++j) {
                const int32_t d = d2_of(q.data() + (size_t)f * D, ref.data() + (size_t)j * D, D);
                if (d < bd) { sd = bd; bd = d; }
                else if (d < sd) sd = d;
              }
              if (ptr[r + 1] > ptr[r] && (!(ratio > 0) || (double)bd < ratio * ratio * (double)sd)) ++want[r];
            }
          }
          if (want != votes) { printf("votes differ at D = %d, n = %d, M = %d\n", D, n, M); ++bad; }
          std::vector<int> order(n_ref);
          for (int r = 0; r < n_ref; ++r) order[r] = r;
          std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return want[a] > want[b]; });
          std::vector<int32_t> take;
          for (int r : order)
            if (want[r] >= (min_votes > 1 ? min_votes : 1) && (int)take.size() < R) take.push_back(r);
          std::sort(take.begin(), take.end());
          if (got != (int32_t)take.size() || !std::equal(take.begin(), take.end(), list.begin())) { printf("list differs at D = %d, n = %d, M = %d, R = %d\n", D, n, M, R); ++bad; }
          for (int k = got; k < R; ++k)
            if (list[k] != -1) { printf("unused slot written at R = %d\n", R); ++bad; }
        }
  printf("desc_shortlist_harness: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
#endif
