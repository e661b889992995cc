// ptz_desc_set.h -- what a resident descriptor set is (ptz_desc_set_create, ptz_desc_match.hip), for the files whose kernels read
// one: the matcher and the shortlist, and the check of the options every entry point over a pair of sets takes.  Rows are packed
// as ptz_desc_sweep.h describes: a byte xor 0x80 as int8, rows padded with zeros to 64 KS bytes, every image to a multiple of
// DESC_ROW_PAD rows (zero rows, norm INT32_MAX), and DESC_ROW_PAD such rows of slack behind the last image.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "ptz_common.h"
#include "ptz_host_batch.h"

namespace ptz {

constexpr int DESC_ROW_PAD = 64;  // rows of an image are padded to this

}  // namespace ptz

struct ptz_desc_set {
  int device = 0;
  int32_t n_img = 0, D = 0, KS = 0;
  int64_t n_feat = 0;
  std::vector<int64_t> feat_ptr, row_off;  // [n_img + 1]
  ptz::PoolBlock blk;
  int8_t* d_desc = nullptr;   // [rows + slack][64 KS]
  int32_t* d_norm = nullptr;  // [rows + slack]
  float2* d_kp = nullptr;     // [n_feat] or nullptr
  // the two offset tables on the device as well, [n_img + 2]: entry n_img + 1 closes the slack (feat_ptr: no features)
  const int64_t* d_feat_ptr = nullptr;
  const int64_t* d_row_off = nullptr;
};

namespace ptz {

// *o = the caller's ptz_desc_options, or the defaults on A's device; PTZ_EINVAL unless the two sets are there, share a device --
// the options' -- and a D, and every option is finite and in range
inline int32_t desc_options_check(const ptz_desc_set* A, const ptz_desc_set* B, const ptz_desc_options* opt, ptz_desc_options* o)
{
  ptz_desc_options_default(o);
  if (opt) *o = *opt;
  else if (A) o->device_id = A->device;
  if (!A || !B) return PTZ_EINVAL;
  if (A->device != B->device || o->device_id != A->device || A->D != B->D) return PTZ_EINVAL;
  if (!(std::isfinite(o->ratio) && o->ratio >= 0) || o->max_dist2 < 0 || o->min_matches < 0 || o->workspace_bytes <= 0) return PTZ_EINVAL;
  return PTZ_OK;
}

inline int32_t shortlist_options_check(const ptz_shortlist_options& s)
{
  return s.max_refs < 1 || s.n_probes < 1 || s.min_votes < 0 ? PTZ_EINVAL : PTZ_OK;
}

inline int32_t prior_options_check(const ptz_prior_options& p)
{
  return !(std::isfinite(p.radius_px) && p.radius_px > 0) || p.max_refs < 1 || p.min_overlap < 0 || p.min_overlap > 128 ? PTZ_EINVAL : PTZ_OK;
}

// every entry of every prior camera finite, the focals positive
inline int32_t prior_cams_check(int32_t n_query, const double* prior_cams)
{
  for (size_t q = 0; q < (size_t)(n_query > 0 ? n_query : 0); ++q) {
    const double* c = prior_cams + 15 * q;
    for (int k = 0; k < 15; ++k)
      if (!std::isfinite(c[k])) return PTZ_EINVAL;
    if (!(c[0] > 0) || !(c[1] > 0)) return PTZ_EINVAL;
  }
  return PTZ_OK;
}

// what ptz_relocalizer_run_tracked adds around the library's entry points (ptz_reloc_prior.hip): the H of every pair of the host's
// list from the slots (pair p of query q is slot p - query_ptr[q]), and the prior's part of the solve's initial camera
void reloc_prior_enqueue_gather(int n_pair, int n_query, int R, const int64_t* d_query_ptr, const double* d_H_slot, double* d_H, hipStream_t st);
void reloc_prior_enqueue_cams(int n_query, const double* d_prior_cams, int factor_type, double* d_cam_cur, hipStream_t st);

}  // namespace ptz
