// Host check of the block-layout cursor (ptz_block_layout.h) and of the layout of a relocalization batch's inputs built on it
// (ptz_krt_batch_layout.h): a stand-alone program, built with the address and undefined-behaviour sanitizers by
// tests/test_cpu_krt_batch_layout.py.  For every combination of sizes below: every slot starts on a 256-byte boundary, slots do not
// overlap, an empty array still has a slot of one element, cam_cur is the last input slot, outputs taken behind it start where the
// inputs end, and the total is the sum of the rounded sizes.  (A batch without 2D-3D points is laid out as one with zero points: the
// reservation does not look at the pointer.)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../ptz-calib_amd/csrc/ptz_krt_batch_layout.h"

using namespace ptz;

static int failures = 0;
#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    if (!(cond)) { ++failures; fprintf(stderr, "line %d: %s  (n %d, matches %lld, points %lld, mask %d, accepted %d)\n", \
                                       __LINE__, #cond, n, (long long)nm, (long long)np, (int)mask, (int)acc); }       \
  } while (0)

struct Slot { size_t at, need; };  // offset, bytes the array needs (of at least one element)

static size_t rounded(size_t x) { return (x + 255) / 256 * 256; }  // (written out again: not the header's expression)

static void check(int n, int64_t nm, int64_t np, bool mask, bool acc)
{
  const size_t nq = (size_t)n, m1 = (size_t)std::max<int64_t>(nm, 1), p1 = (size_t)std::max<int64_t>(np, 1);
  BlockLayout lay;
  const size_t lead = lay.take(40);  // something of the caller's in front
  CHECK(lead == 0 && lay.total() == 256);
  const KrtBatchSlots s = krt_batch_reserve(lay, n, nm, np, mask, acc);
  const size_t o_out = lay.take(24 * nq);
  std::vector<Slot> slots = {{s.match_ptr, 8 * (nq + 1)}, {s.uv_ref, 8 * m1}, {s.uv_cur, 8 * m1}, {s.cam_ref, 120 * nq}, {s.point_ptr, 8 * (nq + 1)},
                             {s.pt_uv, 8 * p1}, {s.pt_xyz, 24 * p1}, {s.cam_cur, 120 * nq}};
  CHECK((s.mask != kNoSlot) == mask && (s.accepted != kNoSlot) == acc);
  if (mask) slots.push_back({s.mask, m1});
  if (acc) slots.push_back({s.accepted, 4 * nq});
  std::sort(slots.begin(), slots.end(), [](const Slot& a, const Slot& b) { return a.at < b.at; });
  size_t sum = 0;
  for (size_t i = 0; i < slots.size(); ++i) {
    CHECK(slots[i].at % 256 == 0);
    CHECK(slots[i].need >= 1);
    const size_t next = i + 1 < slots.size() ? slots[i + 1].at : s.end;
    CHECK(slots[i].at + slots[i].need <= next);  // long enough, and clear of the next slot
    sum += rounded(slots[i].need);
  }
  CHECK(s.begin == 256 && slots.front().at == s.begin);
  CHECK(slots.back().at == s.cam_cur);  // the last input
  CHECK(s.end - s.begin == sum);
  CHECK(o_out == s.end && lay.total() == s.end + rounded(24 * nq));
}

int main()
{
  // the cursor by itself
  {
    const int n = 0; const int64_t nm = 0, np = 0; const bool mask = false, acc = false;
    BlockLayout lay;
    CHECK(lay.total() == 0);
    CHECK(lay.take(0) == 0 && lay.total() == 0);  // an empty slot takes nothing
    CHECK(lay.take(1) == 0 && lay.take(256) == 256 && lay.take(257) == 512 && lay.total() == 1024);
    CHECK(up256(0) == 0 && up256(255) == 256 && up256(256) == 256 && up256(((size_t)1 << 40) + 1) == ((size_t)1 << 40) + 256);
  }
  const int ns[] = {1, 3, 24, 257, 100000};
  const int64_t nms[] = {0, 1, 31, 32, 384, 3072, 12800000, ((int64_t)1 << 31) + 5};
  const int64_t nps[] = {0, 1, 5, 11, 4096};
  int count = 0;
  for (int n : ns)
    for (int64_t nm : nms)
      for (int64_t np : nps)
        for (int f = 0; f < 4; ++f, ++count) check(n, nm, np, (f & 1) != 0, (f & 2) != 0);
  printf("%d layouts, %d failures\n", count, failures);
  return failures ? 1 : 0;
}
