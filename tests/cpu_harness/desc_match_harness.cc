// desc_match_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of the descriptor matcher's contract in
// ptz-calib_amd/csrc/ptz_desc_match.h (what k_desc_top2 / k_desc_join of ptz_desc_match.hip spread over lanes and tiles): brute-force
// d2, a top-2 built by merging single candidates and partial states in a scrambled order, then the acceptance rule -- so it can be
// held to a numpy restatement without a GPU.  Never part of the product library.  With DESC_MATCH_HARNESS_MAIN it is a stand-alone
// program (for a sanitizer build): generated pairs with ties, one-feature images and every option against a plain scan; returns 0 if
// they agree.
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../ptz-calib_amd/csrc/ptz_desc_match.h"

using namespace ptz;

namespace {

int32_t d2_of(const uint8_t* a, const uint8_t* b, int D)
{
  int32_t s = 0;
  for (int k = 0; k < D; ++k) { const int32_t d = (int32_t)a[k] - (int32_t)b[k]; s += d * d; }
  return s;
}

// the top-2 of every row of a against b: the candidates are dealt to `parts` partial states in an order scrambled by `seed`, the
// partial states merged in another scrambled order
void top2_scrambled(const uint8_t* a, int na, const uint8_t* b, int nb, int D, uint64_t seed, int parts, std::vector<DescTop2>& out)
{
  out.assign(na, desc_top2_empty());
  uint64_t s = seed * 2862933555777941757ull + 3037000493ull;
  auto next = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
  std::vector<int> order(nb), pord(parts);
  std::vector<DescTop2> part(parts);
  for (int i = 0; i < na; ++i) {
    for (int j = 0; j < nb; ++j) order[j] = j;
    for (int j = nb - 1; j > 0; --j) std::swap(order[j], order[next() % (j + 1)]);
    for (int p = 0; p < parts; ++p) { part[p] = desc_top2_empty(); pord[p] = p; }
    for (int x = 0; x < nb; ++x) {
      const int j = order[x], p = next() % parts;
      part[p] = (next() & 1) ? desc_top2_merge(part[p], desc_top2_one(d2_of(a + (size_t)i * D, b + (size_t)j * D, D), j))
                             : desc_top2_merge(desc_top2_one(d2_of(a + (size_t)i * D, b + (size_t)j * D, D), j), part[p]);
    }
    for (int p = parts - 1; p > 0; --p) std::swap(pord[p], pord[next() % (p + 1)]);
    DescTop2 t = desc_top2_empty();
    for (int p = 0; p < parts; ++p) t = (next() & 1) ? desc_top2_merge(t, part[pord[p]]) : desc_top2_merge(part[pord[p]], t);
    out[i] = t;
  }
}

}  // namespace

extern "C" {
// One pair.  top_a [3 na] / top_b [3 nb] (nullable): the states (d, j, s); idx_a / idx_b / dist2 [na]: the matches, ascending idx_a.
// Returns their number (0 if fewer than min_matches).
int64_t h_desc_match_pair(const uint8_t* a, int32_t na, const uint8_t* b, int32_t nb, int32_t D, double ratio, int32_t max_dist2,
                          int32_t cross_check, int32_t min_matches, uint64_t seed, int32_t parts, int32_t* top_a, int32_t* top_b,
                          int32_t* idx_a, int32_t* idx_b, int32_t* dist2)
{
  std::vector<DescTop2> ta, tb;
  top2_scrambled(a, na, b, nb, D, seed, parts < 1 ? 1 : parts, ta);
  top2_scrambled(b, nb, a, na, D, seed + 1, parts < 1 ? 1 : parts, tb);
  if (top_a)
    for (int i = 0; i < na; ++i) { top_a[3 * i] = ta[i].d; top_a[3 * i + 1] = ta[i].j; top_a[3 * i + 2] = ta[i].s; }
  if (top_b)
    for (int j = 0; j < nb; ++j) { top_b[3 * j] = tb[j].d; top_b[3 * j + 1] = tb[j].j; top_b[3 * j + 2] = tb[j].s; }
  const DescRule r = {ratio * ratio, max_dist2, cross_check ? 1 : 0};
  int64_t n = 0;
  for (int i = 0; i < na; ++i) {
    const DescTop2 other = ta[i].j != kDescNone ? tb[ta[i].j] : desc_top2_empty();
    if (!desc_accept(r, i, ta[i], other)) continue;
    idx_a[n] = i; idx_b[n] = ta[i].j; dist2[n] = ta[i].d;
    ++n;
  }
  return n < min_matches ? 0 : n;
}
}

#ifdef DESC_MATCH_HARNESS_MAIN
int main()
{
  uint64_t s = 99;
  auto next = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
  int bad = 0;
  const int sizes[] = {0, 1, 2, 15, 16, 17, 63, 65, 130};
  const int dims[] = {1, 32, 130, 512};
  for (int D : dims)
    for (int na : sizes)
      for (int nb : sizes) {
        std::vector<uint8_t> a((size_t)na * D + 1), b((size_t)nb * D + 1);
        for (auto& v : a) v = (uint8_t)(D == 1 ? next() % 4 : next());
        for (auto& v : b) v = (uint8_t)(D == 1 ? next() % 4 : next());
        if (na > 2 && nb > 3) {  // ties: two equal rows in b that are a's row 1, two equal rows in a
          std::copy(a.begin() + D, a.begin() + 2 * D, b.begin());
          std::copy(a.begin() + D, a.begin() + 2 * D, b.begin() + 3 * (size_t)D);
          std::copy(a.begin(), a.begin() + D, a.begin() + 2 * (size_t)D);
        }
        for (int opt = 0; opt < 6; ++opt) {
          const double ratio = opt % 3 == 0 ? 0.8 : (opt % 3 == 1 ? 0.0 : 1.0);
          const int cross = opt < 3;
          std::vector<int32_t> ta(3 * na + 1), tb(3 * nb + 1), ia(na + 1), ib(na + 1), dd(na + 1);
          const int64_t n = h_desc_match_pair(a.data(), na, b.data(), nb, D, ratio, 0, cross, 0, next(), 1 + next() % 7, ta.data(), tb.data(),
                                              ia.data(), ib.data(), dd.data());
          // a plain scan
          auto scan = [&](const uint8_t* x, int nx, const uint8_t* y, int ny, std::vector<int32_t>& o) {
            o.assign(3 * nx + 1, 0);
            for (int i = 0; i < nx; ++i) {
              int32_t bd = INT32_MAX, bj = INT32_MAX, sd = INT32_MAX;
              for (int j = 0; j < ny; ++j) {
                const int32_t d = d2_of(x + (size_t)i * D, y + (size_t)j * D, D);
                if (d < bd) { sd = bd; bd = d; bj = j; }
                else if (d < sd) sd = d;
              }
              o[3 * i] = bd; o[3 * i + 1] = bj; o[3 * i + 2] = sd;
            }
          };
          std::vector<int32_t> wa, wb;
          scan(a.data(), na, b.data(), nb, wa);
          scan(b.data(), nb, a.data(), na, wb);
          if (!std::equal(wa.begin(), wa.begin() + 3 * na, ta.begin()) || !std::equal(wb.begin(), wb.begin() + 3 * nb, tb.begin())) {
            printf("top-2 differs at D = %d, %d x %d\n", D, na, nb);
            ++bad;
          }
          int64_t m = 0;
          const double r2 = ratio * ratio;
          for (int i = 0; i < na && nb > 0; ++i) {
            const int32_t d = wa[3 * i], j = wa[3 * i + 1];
            bool ok = !cross || wb[3 * j + 1] == i;
            if (ratio > 0) ok = ok && (double)d < r2 * (double)wa[3 * i + 2] && (!cross || (double)d < r2 * (double)wb[3 * j + 2]);
            if (!ok) continue;
            if (m >= n || ia[m] != i || ib[m] != j || dd[m] != d) { printf("match differs at D = %d, %d x %d, option %d\n", D, na, nb, opt); ++bad; break; }
            ++m;
          }
          if (m != n) { printf("count differs at D = %d, %d x %d, option %d: %lld, expected %lld\n", D, na, nb, opt, (long long)n, (long long)m); ++bad; }
        }
      }
  printf("desc_match_harness: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
#endif
