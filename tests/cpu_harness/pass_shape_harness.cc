// pass_shape_harness.cc -- TEST INFRASTRUCTURE.  Host entry to the pure function that chooses the grid extent of an LM pass
// (ptz-calib_amd/csrc/ptz_pass_shape.h), so that it can be checked for every count without a GPU.  Never part of the product library.
//
// Built as a shared library for tests/test_cpu_pass_shape.py; with -DPASS_SHAPE_MAIN it is a stand-alone program that sweeps the
// same cases and checks the same properties itself (the form to build with a sanitizer).
#include "../../ptz-calib_amd/csrc/ptz_pass_shape.h"

extern "C" void h_pass_extent(int count, int group_n, const int* ladder, int n_ladder, int graph, int exact_fit, int* out3)
{
  const ptz::PassExtent e = ptz::pass_extent(count, group_n, ladder, n_ladder, graph != 0, exact_fit != 0);
  out3[0] = e.shape; out3[1] = e.slots; out3[2] = e.compact ? 1 : 0;
}

#ifdef PASS_SHAPE_MAIN
#include <cstdio>
#include <vector>

// the ladder a batch of n scenes keeps: full size, then 2 (8 for a batch of up to eight), x4 while below n
static std::vector<int> ladder_of(int n)
{
  std::vector<int> l{n};
  for (int sl = n > 8 ? 2 : 8; sl < n; sl *= 4) l.push_back(sl);
  return l;
}

int main()
{
  const int batches[][2] = {{1, 1}, {16, 8}, {33, 33}, {1000, 500}, {1000, 1000}};  // (batch, group)
  int bad = 0;
  for (const auto& bg : batches) {
    const std::vector<int> lad = ladder_of(bg[0]);
    const int gn = bg[1], nl = (int)lad.size();
    for (int c = -1; c <= 1100; ++c) {
      int want = 0;  // the covering ladder shape, restated
      for (int k = 1; k < nl; ++k) if (lad[k] >= c && lad[k] < gn) { want = k; break; }
      for (int graph = 0; graph < 2; ++graph)
        for (int fit = 0; fit < 2; ++fit) {
          int o[3];
          h_pass_extent(c, gn, lad.data(), nl, graph, fit, o);
          bool ok = o[0] == want;
          if (graph || !fit || nl == 1) ok = ok && o[1] == (want ? lad[want] : gn) && o[2] == (want != 0);
          else {
            const int cl = c < 1 ? 1 : (c > gn ? gn : c);
            ok = ok && o[1] == cl && o[2] == (cl < gn);
          }
          ok = ok && o[1] >= 1 && o[1] <= gn;
          if (!ok) { ++bad; printf("FAIL batch %d group %d count %d graph %d fit %d -> shape %d slots %d compact %d\n", bg[0], gn, c, graph, fit, o[0], o[1], o[2]); }
        }
    }
  }
  printf("%s\n", bad ? "pass_shape_harness: FAILED" : "pass_shape_harness: ok");
  return bad ? 1 : 0;
}
#endif
