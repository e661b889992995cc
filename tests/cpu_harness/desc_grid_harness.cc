// desc_grid_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of ptz-calib_amd/csrc/ptz_desc_grid.h in the order
// k_desc_top2_guided_grid of ptz_desc_match.hip uses it: per (pair, direction) the searched side goes through slabs of at most S
// positions (S a PARAMETER here, so that slab edges are tested at small sizes); per slab the frame of the finite positions, a
// histogram over the cells, an exclusive scan and a scatter into cell order (here in DESCENDING feature order: the update must
// not care); per query the cell range, the header's predicate on every candidate of its runs, d2 from the packed rows, and
// desc_top2_take_keyed.  Held to the numpy restatement (tests/desc_guided_util.py) without a GPU.  Never part of the product
// library.  With DESC_GRID_HARNESS_MAIN it is a stand-alone program (for a sanitizer build): generated pairs at three radii and
// three slab sizes against a plain masked scan; returns 0 if they agree.
#include <stdint.h>

#include <cstdio>
#include <vector>

#include "../../ptz-calib_amd/csrc/ptz_desc_grid.h"

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

// the index of one slab: the searched positions s0 .. s0 + cnt - 1 (x = NaN: not a position)
struct Slab {
  DescGridFrame F;
  std::vector<float> x, y;
  std::vector<int32_t> feat;
  std::vector<int32_t> end;  // end[c]: the end of cell c in the sorted arrays
};

DescGridFrame frame_of(const float* xy, int n, double reach)
{
  const float inf = __builtin_inff();
  float x0 = inf, x1 = -inf, y0 = inf, y1 = -inf;
  for (int k = 0; k < n; ++k) {
    const float x = xy[2 * k], y = xy[2 * k + 1];
    if (!desc_grid_indexed(x, y)) continue;
    x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1; y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
  }
  return desc_grid_frame(x0, x1, y0, y1, reach);
}

Slab build(const float* xy, int s0, int cnt, double reach)
{
  Slab s;
  s.F = frame_of(xy + 2 * (size_t)s0, cnt, reach);
  const int cells = kDescGridG * kDescGridG;
  std::vector<int32_t> cur(cells, 0), cell(cnt, -1);
  for (int k = 0; k < cnt; ++k) {
    const float x = xy[2 * (size_t)(s0 + k)], y = xy[2 * (size_t)(s0 + k) + 1];
    if (!desc_grid_indexed(x, y)) continue;
    cell[k] = desc_grid_cell(s.F, 1, (double)y) * kDescGridG + desc_grid_cell(s.F, 0, (double)x);
    ++cur[cell[k]];
  }
  int at = 0;
  for (int c = 0; c < cells; ++c) { const int n = cur[c]; cur[c] = at; at += n; }
  s.x.resize(at); s.y.resize(at); s.feat.resize(at);
  for (int k = cnt - 1; k >= 0; --k) {
    if (cell[k] < 0) continue;
    const int o = cur[cell[k]]++;
    s.x[o] = xy[2 * (size_t)(s0 + k)]; s.y[o] = xy[2 * (size_t)(s0 + k) + 1]; s.feat[o] = s0 + k;
  }
  s.end = cur;
  return s;
}

// one direction: queries (qx, qy, ask) of packed rows Q ask the positions sxy of packed rows Sd
void direction(const Packed& Q, const std::vector<float>& qxy, const std::vector<uint8_t>& ask, const Packed& Sd, const std::vector<float>& sxy,
               int ns, int S, float r2f, double reach, std::vector<DescTop2>& T)
{
  for (int s0 = 0; s0 < ns; s0 += S) {
    const Slab sl = build(sxy.data(), s0, ns - s0 < S ? ns - s0 : S, reach);
    if (sl.F.empty) continue;
    for (size_t q = 0; q < T.size(); ++q) {
      const float qx = qxy[2 * q], qy = qxy[2 * q + 1];
      if (!ask[q] || !desc_grid_indexed(qx, qy)) continue;
      const DescGridRange R = desc_grid_range(sl.F, qx, qy, reach);
      for (int gy = R.cy0; gy <= R.cy1; ++gy) {
        const int c0 = gy * kDescGridG + R.cx0;
        for (int k = c0 > 0 ? sl.end[c0 - 1] : 0; k < sl.end[gy * kDescGridG + R.cx1]; ++k)
          if (desc_guide_err2(qx, qy, sl.x[k], sl.y[k]) <= r2f) desc_top2_take_keyed(T[q], d2_packed(Q, (int)q, Sd, sl.feat[k]), sl.feat[k]);
      }
    }
  }
}

}  // namespace

extern "C" {
int32_t h_desc_grid_g() { return kDescGridG; }
int32_t h_desc_grid_slab() { return kDescGridSlab; }
double h_desc_grid_reach(double radius_px) { return desc_grid_reach(radius_px); }

// the frame of n positions: out = (x0, y0, 1 / cx, 1 / cy); returns 0 for an empty index
int32_t h_desc_grid_frame(int32_t n, const float* xy, double radius_px, double* out)
{
  const DescGridFrame F = frame_of(xy, n, desc_grid_reach(radius_px));
  out[0] = F.x0; out[1] = F.y0; out[2] = F.ix; out[3] = F.iy;
  return F.empty ? 0 : 1;
}

// under the frame of the n searched positions: cell [2 n] = (cx, cy) of each (-1, -1: not indexed), range [4 nq] = (cx0, cx1, cy0,
// cy1) of each query (1, 0, 1, 0: does not search)
void h_desc_grid_cells(int32_t n, const float* xy, int32_t nq, const float* qxy, double radius_px, int32_t* cell, int32_t* range)
{
  const double reach = desc_grid_reach(radius_px);
  const DescGridFrame F = frame_of(xy, n, reach);
  for (int k = 0; k < n; ++k) {
    const bool in = !F.empty && desc_grid_indexed(xy[2 * k], xy[2 * k + 1]);
    cell[2 * k] = in ? desc_grid_cell(F, 0, (double)xy[2 * k]) : -1;
    cell[2 * k + 1] = in ? desc_grid_cell(F, 1, (double)xy[2 * k + 1]) : -1;
  }
  for (int q = 0; q < nq; ++q) {
    DescGridRange R = {1, 0, 1, 0};
    if (!F.empty && desc_grid_indexed(qxy[2 * q], qxy[2 * q + 1])) R = desc_grid_range(F, qxy[2 * q], qxy[2 * q + 1], reach);
    range[4 * q] = R.cx0; range[4 * q + 1] = R.cx1; range[4 * q + 2] = R.cy0; range[4 * q + 3] = R.cy1;
  }
}

// the state (d, j, s) after the n candidates (d2[k], j[k]) in the order given
void h_desc_top2_take_keyed(int32_t n, const int32_t* d2, const int32_t* j, int32_t* out)
{
  DescTop2 T = desc_top2_empty();
  for (int k = 0; k < n; ++k) desc_top2_take_keyed(T, d2[k], j[k]);
  out[0] = T.d; out[1] = T.j; out[2] = T.s;
}

// One pair under H (b ~ H a) through slabs of S positions, in the form of h_desc_match_pair_guided (desc_guided_harness.cc).
int64_t h_desc_match_pair_grid(const uint8_t* a, int32_t na, const uint8_t* b, int32_t nb, int32_t D, const float* kp_a, const float* kp_b,
                               const double* H, double radius_px, int32_t S, double ratio, int32_t max_dist2, int32_t cross_check,
                               int32_t min_matches, int32_t* top_a, int32_t* top_b, int32_t* idx_a, int32_t* idx_b, int32_t* dist2)
{
  const float r2f = (float)(radius_px * radius_px);
  const double reach = desc_grid_reach(radius_px);
  const Packed A = pack(a, na, D), B = pack(b, nb, D);
  std::vector<DescTop2> ta(na, desc_top2_empty()), tb(nb, desc_top2_empty());
  std::vector<float> wa(2 * (size_t)na), wnan(2 * (size_t)na), kb(kp_b, kp_b + 2 * (size_t)nb);
  std::vector<uint8_t> ok(na), all(nb, 1);
  for (int i = 0; i < na; ++i) {
    const DescWarp w = desc_guide_warp(H, kp_a[2 * i], kp_a[2 * i + 1]);
    ok[i] = w.ok ? 1 : 0;
    wa[2 * i] = w.x; wa[2 * i + 1] = w.y;
    wnan[2 * i] = w.ok ? w.x : __builtin_nanf(""); wnan[2 * i + 1] = w.ok ? w.y : __builtin_nanf("");  // as the kernel stages them
  }
  if (na > 0 && nb > 0 && r2f - r2f == 0.f) {
    direction(A, wa, ok, B, kb, nb, S, r2f, reach, ta);     // direction 0: A's warped point asks B's key points
    direction(B, kb, all, A, wnan, na, S, r2f, reach, tb);  // direction 1: B's key point asks A's warped points
  }
  else {  // an r2f that is not finite: no grid, every pair is tested (the host runs the scan kernel)
    for (int i = 0; i < na; ++i)
      for (int j = 0; j < nb; ++j)
        if (ok[i] && desc_guide_admissible(wa[2 * i], wa[2 * i + 1], kp_b[2 * j], kp_b[2 * j + 1], r2f)) {
          desc_top2_take_keyed(ta[i], d2_packed(A, i, B, j), j);
          desc_top2_take_keyed(tb[j], d2_packed(B, j, A, i), i);
        }
  }
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

#ifdef DESC_GRID_HARNESS_MAIN
int main()
{
  uint64_t s = 7;
  auto next = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
  int bad = 0;
  const int sizes[] = {1, 2, 17, 65, 130};
  const int dims[] = {1, 32, 130};
  const double radii[] = {0.5, 4.0, 1e9};
  const int slabs[] = {8, 64, kDescGridSlab};
  const double H[9] = {1.01, 0.02, 3.0, -0.02, 0.99, -2.0, 1e-5, -2e-5, 1.0};
  for (int D : dims)
    for (int na : sizes)
      for (int nb : sizes)
        for (double radius : radii)
          for (int S : slabs) {
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
            h_desc_match_pair_grid(a.data(), na, b.data(), nb, D, ka.data(), kb.data(), H, radius, S, 0.0, 0, 0, 0, ta.data(), tb.data(), ia.data(),
                                   ib.data(), dd.data());
            const float r2f = (float)(radius * radius);
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
              if (ta[3 * i] != bd || ta[3 * i + 1] != bj || ta[3 * i + 2] != sd) {
                printf("top-2 differs at D = %d, %d x %d, radius %g, slab %d\n", D, na, nb, radius, S);
                ++bad;
                break;
              }
            }
          }
  printf("desc_grid_harness: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
#endif
