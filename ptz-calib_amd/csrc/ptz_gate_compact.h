// ptz_gate_compact.h -- the integer stages of the match gate (ptz_homography.hip) for the other callers of the library: the matches
// of a CSR whose mask byte is non-zero, packed pair by pair in their order.  Three launches on one stream, device pointers throughout.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptz {

// d_cnt[p] = the non-zero mask bytes of pair p if d_found[p] == 1 and there are at least `need` of them, else 0;
// d_out_ptr [n_pair + 1] = their exclusive scan; d_out_a / d_out_b (nullable together, d_a / d_b are then not read; and d_out_index,
// nullable: the source positions) = the kept
// matches of the pairs with d_cnt[p] > 0.  d_live (nullable): a device counter of the pairs that have work; where it reads 0 the three
// launches return at once and write nothing -- for a caller that enqueues more rounds than its data may need and reads the
// outputs of a round only for pairs that had work in it.
void enqueue_compact(int n_pair, const int64_t* d_ptr, const int32_t* d_found, const uint8_t* d_mask, int32_t need, int32_t* d_cnt,
                     int64_t* d_out_ptr, const float2* d_a, const float2* d_b, float2* d_out_a, float2* d_out_b, int32_t* d_out_index,
                     hipStream_t st, const int32_t* d_live = nullptr);

}  // namespace ptz
