// ptz_krt_batch_layout.h -- where the inputs of a relocalization batch lie in a call's device block (plain C++, see ptz_block_layout.h).
#pragma once

#include <cstdint>

#include "ptz_block_layout.h"

namespace ptz {

constexpr size_t kNoSlot = ~(size_t)0;

// byte offsets of the inputs; begin .. end is their extent on the cursor, cam_cur the last slot of it: a solve's outputs follow, so
// that [cam_cur | outputs] comes back in one copy
struct KrtBatchSlots {
  size_t match_ptr, uv_ref, uv_cur, cam_ref, point_ptr, pt_uv, pt_xyz;
  size_t mask, accepted;  // kNoSlot where the call has none
  size_t cam_cur;
  size_t begin, end;
};

// n_match / n_point: the last entries of the two CSR offset arrays (an empty array still gets a slot of one element; the 2D-3D slots
// are there, empty, also for a batch without points)
inline KrtBatchSlots krt_batch_reserve(BlockLayout& lay, int n_query, int64_t n_match, int64_t n_point, bool with_mask, bool with_accepted)
{
  const size_t nq = (size_t)n_query, nm = (size_t)(n_match > 0 ? n_match : 1), np = (size_t)(n_point > 0 ? n_point : 1);
  const size_t F2 = 2 * sizeof(float), D = sizeof(double);
  KrtBatchSlots s;
  s.begin = lay.total();
  s.match_ptr = lay.take(sizeof(long long) * (nq + 1));
  s.uv_ref = lay.take(F2 * nm);
  s.uv_cur = lay.take(F2 * nm);
  s.cam_ref = lay.take(D * 15 * nq);
  s.point_ptr = lay.take(sizeof(long long) * (nq + 1));
  s.pt_uv = lay.take(F2 * np);
  s.pt_xyz = lay.take(D * 3 * np);
  s.mask = with_mask ? lay.take(nm) : kNoSlot;
  s.accepted = with_accepted ? lay.take(sizeof(int) * nq) : kNoSlot;
  s.cam_cur = lay.take(D * 15 * nq);
  s.end = lay.total();
  return s;
}

}  // namespace ptz
