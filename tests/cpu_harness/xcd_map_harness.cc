// xcd_map_harness.cc -- TEST INFRASTRUCTURE.  Host entry to the index arithmetic that deals the workgroups of an (item, slot)
// launch over the XCDs by the live slot count (ptz-calib_amd/csrc/ptz_xcd_map.h), so that it can be checked for every live count
// without a GPU.  Never part of the product library.
//
// Built as a shared library for tests/test_cpu_xcd_map.py; with -DXCD_MAP_MAIN it is a stand-alone program that sweeps the same
// cases and checks the same properties itself (the form to build with a sanitizer).
#include "../../ptz-calib_amd/csrc/ptz_xcd_map.h"

// out[3 * L + {0, 1, 2}] = {work, bx, by} for every linear id L of a gx x rows launch
extern "C" void h_xcd_live_map(int gx, int rows, int live, int* out)
{
  for (unsigned L = 0; L < (unsigned)gx * (unsigned)rows; ++L) {
    const ptz::XcdItem it = ptz::xcd_live_item(L, (unsigned)gx, (unsigned)live);
    out[3 * L] = it.work ? 1 : 0; out[3 * L + 1] = (int)it.bx; out[3 * L + 2] = (int)it.by;
  }
}

// the remap the kernels used before there was a live count (every id has work), restated: out[2 * L + {0, 1}] = {bx, by}
extern "C" void h_xcd_full_map(int gx, int rows, int* out)
{
  const unsigned ugx = (unsigned)gx, total = ugx * (unsigned)rows;
  for (unsigned L = 0; L < total; ++L) {
    const unsigned q = total / 8, r = total % 8, xcd = L % 8, idx = L / 8;
    const unsigned Lp = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    out[2 * L] = (int)(Lp % ugx); out[2 * L + 1] = (int)(Lp / ugx);
  }
}

#ifdef XCD_MAP_MAIN
#include <cstdio>
#include <vector>

int main()
{
  const int gxs[] = {1, 3, 13, 200}, rowss[] = {1, 2, 7, 8, 9, 48, 512};
  int bad = 0;
  for (int gx : gxs)
    for (int rows : rowss) {
      const int total = gx * rows;
      std::vector<int> out(3 * (size_t)total), full(2 * (size_t)total);
      h_xcd_full_map(gx, rows, full.data());
      for (int live = 0; live <= rows; ++live) {
        h_xcd_live_map(gx, rows, live, out.data());
        const int items = gx * live;
        std::vector<int> hit((size_t)items, 0);
        int lo[8], hi[8], cnt[8];
        for (int x = 0; x < 8; ++x) { lo[x] = items; hi[x] = -1; cnt[x] = 0; }
        bool ok = true;
        for (int L = 0; L < total; ++L) {
          if (!out[3 * L]) continue;
          const int bx = out[3 * L + 1], by = out[3 * L + 2];
          if (bx < 0 || bx >= gx || by < 0 || by >= live) { ok = false; continue; }
          const int item = by * gx + bx, x = L % 8;
          ++hit[item]; ++cnt[x];
          if (item < lo[x]) lo[x] = item;
          if (item > hi[x]) hi[x] = item;
          // inside an XCD the items ascend with the id: idx-th id, idx-th item of the range
          if (L >= 8 && out[3 * (L - 8)] && item != (out[3 * (L - 8) + 2] * gx + out[3 * (L - 8) + 1]) + 1) ok = false;
          if (L >= 8 && !out[3 * (L - 8)]) ok = false;  // accepted ids of an XCD are its first ones
        }
        for (int i = 0; i < items; ++i) ok = ok && hit[i] == 1;                 // one-to-one onto [0, gx * live)
        int mn = items, mx = 0, next = 0;
        for (int x = 0; x < 8; ++x) {
          if (cnt[x]) { ok = ok && hi[x] - lo[x] + 1 == cnt[x] && lo[x] == next; next = hi[x] + 1; }  // contiguous, in XCD order
          if (cnt[x] < mn) mn = cnt[x];
          if (cnt[x] > mx) mx = cnt[x];
        }
        ok = ok && next == items && mx - mn <= 1;
        if (live == 0) for (int L = 0; L < total; ++L) ok = ok && !out[3 * L];
        if (live == rows)
          for (int L = 0; L < total; ++L) ok = ok && out[3 * L] && out[3 * L + 1] == full[2 * L] && out[3 * L + 2] == full[2 * L + 1];
        if (!ok) { ++bad; printf("FAIL gx %d rows %d live %d\n", gx, rows, live); }
      }
    }
  printf("%s\n", bad ? "xcd_map_harness: FAILED" : "xcd_map_harness: ok");
  return bad ? 1 : 0;
}
#endif
