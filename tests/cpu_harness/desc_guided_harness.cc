// desc_guided_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of the guided part of ptz-calib_amd/csrc/ptz_desc_match.h
// (desc_guide_warp, desc_guide_admissible, desc_dot_i8x4) in the order k_desc_top2_guided of ptz_desc_match.hip uses them: rows
// packed as k_desc_pack packs them, one query at a time, the candidates in ascending index, d2 from the packed rows and their norms
// on an admissible hit, the dense kernel's three-line update -- so it can be held to the numpy restatement
// (tests/desc_guided_util.py) without a GPU.  Never part of the product library.  With DESC_GUIDED_HARNESS_MAIN it is a
// stand-alone program (for a sanitizer build): generated pairs at three radii against a plain masked scan; returns 0 if they agree.
#include <stdint.h>

#include <cstdio>
#include <vector>

#include "../../ptz-calib_amd/csrc/ptz_desc_match.h"

using namespace ptz;

namespace {

struct Packed {
  int W;  // words per row
  std::vector<uint32_t> rows;
  std::vector<int32_t> norm;
};

Packed pack(const uint8_t* x, int n, int D)
{
  Packed P;
  P.W = (D + 63) / 64 * 16;
  P.rows.assign((size_t)n * P.W, 0u);
  P.norm.assign(n, 0);
  for (int r = 0; r < n; ++r)
    for (int k = 0; k < D; ++k) {
      const int v = (int)x[(size_t)r * D + k] - 128;
      P.rows[(size_t)r * P.W + k / 4] |= (uint32_t)(v & 255) << (8 * (k % 4));
      P.norm[r] += v * v;
    }
  return P;
}

int32_t d2_packed(const Packed& A, int i, const Packed& B, int j)
{
  int32_t dot = 0;
  for (int w = 0; w < A.W; ++w) dot += desc_dot_i8x4(A.rows[(size_t)i * A.W + w], B.rows[(size_t)j * B.W + w]);
  return A.norm[i] + B.norm[j] - 2 * dot;
}

void update(DescTop2& t, int32_t key, int32_t j)
{
  t.s = desc_min(t.s, t.d > key ? t.d : key);
  t.j = key < t.d ? j : t.j;
  t.d = desc_min(t.d, key);
}

}  // namespace

extern "C" {
void h_desc_guide_warp(const double* H, int32_t n, const float* xy, float* wx, float* wy, uint8_t* ok)
{
  for (int i = 0; i < n; ++i) {
    const DescWarp w = desc_guide_warp(H, xy[2 * i], xy[2 * i + 1]);
    wx[i] = w.x; wy[i] = w.y; ok[i] = w.ok ? 1 : 0;
  }
}

int32_t h_desc_guide_admissible(float wx, float wy, float bx, float by, double radius_px)
{
  return desc_guide_admissible(wx, wy, bx, by, (float)(radius_px * radius_px)) ? 1 : 0;
}

// One pair under H (b ~ H a).  top_a [3 na] / top_b [3 nb]: the states (d, j, s); idx_a / idx_b / dist2 [na]: the matches, ascending
// idx_a.  Returns their number (0 if fewer than min_matches).
int64_t h_desc_match_pair_guided(const uint8_t* a, int32_t na, const uint8_t* b, int32_t nb, int32_t D, const float* kp_a, const float* kp_b,
                                 const double* H, double radius_px, double ratio, int32_t max_dist2, int32_t cross_check,
                                 int32_t min_matches, int32_t* top_a, int32_t* top_b, int32_t* idx_a, int32_t* idx_b, int32_t* dist2)
{
  const float r2f = (float)(radius_px * radius_px);
  const Packed A = pack(a, na, D), B = pack(b, nb, D);
  std::vector<DescTop2> ta(na, desc_top2_empty()), tb(nb, desc_top2_empty());
  std::vector<DescWarp> wa(na);
  for (int i = 0; i < na; ++i) wa[i] = desc_guide_warp(H, kp_a[2 * i], kp_a[2 * i + 1]);
  for (int i = 0; i < na; ++i) {  // direction 0: A's warped point asks B's key points
    if (!wa[i].ok) continue;
    for (int j = 0; j < nb; ++j)
      if (desc_guide_admissible(wa[i].x, wa[i].y, kp_b[2 * j], kp_b[2 * j + 1], r2f)) update(ta[i], d2_packed(A, i, B, j), j);
  }
  for (int j = 0; j < nb; ++j)  // direction 1: B's key point asks A's warped points
    for (int i = 0; i < na; ++i)
      if (wa[i].ok && desc_guide_admissible(wa[i].x, wa[i].y, kp_b[2 * j], kp_b[2 * j + 1], r2f)) update(tb[j], d2_packed(B, j, A, i), i);
  for (int i = 0; i < na; ++i) { top_a[3 * i] = ta[i].d; top_a[3 * i + 1] = ta[i].j; top_a[3 * i + 2] = ta[i].s; }
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

#ifdef DESC_GUIDED_HARNESS_MAIN
int main()
{
  uint64_t s = 7;
  auto next = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
  int bad = 0;
  const int sizes[] = {1, 2, 17, 65, 130};
  const int dims[] = {1, 32, 130};
  const double radii[] = {0.5, 4.0, 1e9};
  const double H[9] = {1.01, 0.02, 3.0, -0.02, 0.99, -2.0, 1e-5, -2e-5, 1.0};
  for (int D : dims)
    for (int na : sizes)
      for (int nb : sizes)
        for (double radius : radii) {
          std::vector<uint8_t> a((size_t)na * D), b((size_t)nb * D);
          for (auto& v : a) v = (uint8_t)(D == 1 ? next() % 4 : next());
          for (auto& v : b) v = (uint8_t)(D == 1 ? next() % 4 : next());
          std::vector<float> ka(2 * na), kb(2 * nb);
          for (auto& v : ka) v = (float)(next() % 64);
          for (int j = 0; j < nb; ++j) {  // B's points near the warp of one of A's, so that a few pixels admit something
            const DescWarp w = desc_guide_warp(H, ka[2 * (j % na)], ka[2 * (j % na) + 1]);
            kb[2 * j] = w.x + (float)(next() % 5) - 2.f;
            kb[2 * j + 1] = w.y + (float)(next() % 5) - 2.f;
          }
          std::vector<int32_t> ta(3 * na), tb(3 * nb), ia(na), ib(na), dd(na);
          const int64_t n = h_desc_match_pair_guided(a.data(), na, b.data(), nb, D, ka.data(), kb.data(), H, radius, 0.0, 0, 0, 0, ta.data(),
                                                     tb.data(), ia.data(), ib.data(), dd.data());
          const float r2f = (float)(radius * radius);
          int64_t m = 0;
          for (int i = 0; i < na; ++i) {  // a plain masked scan on the raw bytes
            const DescWarp w = desc_guide_warp(H, ka[2 * i], ka[2 * i + 1]);
            int32_t bd = INT32_MAX, bj = INT32_MAX, sd = INT32_MAX;
            for (int j = 0; j < nb; ++j) {
              const float dx = w.x - kb[2 * j], dy = w.y - kb[2 * j + 1];
              if (!w.ok || !(dx * dx + dy * dy <= r2f)) continue;
              int32_t d = 0;
              for (int k = 0; k < D; ++k) { const int32_t e = (int32_t)a[(size_t)i * D + k] - (int32_t)b[(size_t)j * D + k]; d += e * e; }
              if (d < bd) { sd = bd; bd = d; bj = j; }
              else if (d < sd) sd = d;
            }
            if (ta[3 * i] != bd || ta[3 * i + 1] != bj || ta[3 * i + 2] != sd) { printf("top-2 differs at D = %d, %d x %d, radius %g\n", D, na, nb, radius); ++bad; break; }
            if (bj != INT32_MAX) {
              if (m >= n || ia[m] != i || ib[m] != bj || dd[m] != bd) { printf("match differs at D = %d, %d x %d, radius %g\n", D, na, nb, radius); ++bad; break; }
              ++m;
            }
            if (i == na - 1 && m != n) { printf("count differs at D = %d, %d x %d, radius %g\n", D, na, nb, radius); ++bad; }
          }
        }
  printf("desc_guided_harness: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
#endif
