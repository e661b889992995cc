// ptz_landmark_map.h -- what a landmark map is (ptz_landmark_map_create, ptz_landmark.hip), for the serving loop that runs against
// one (ptz_relocalizer.hip).  The rays and homes stay on the device for the assembly; every array has a host copy for
// ptz_landmark_map_download; the descriptors live in a ptz_desc_set of ONE image of n_lm features (placeholder key points, all zero:
// the matcher gathers uv_a from them and nobody reads it), so the distances stay on the matcher's kernels.
#pragma once

#include <mutex>
#include <vector>

#include "ptz_common.h"
#include "ptz_host_batch.h"

struct ptz_desc_set;

struct ptz_landmark_map {
  int device = 0;
  int32_t n_ref = 0, n_track = 0, n_lm = 0, D = 0, factor_type = 0, min_views = 1;
  ptz::PoolBlock blk;
  double* d_ray = nullptr;    // [3 n_lm]
  int32_t* d_home = nullptr;  // [n_lm]
  std::vector<int32_t> track, home, views;
  std::vector<double> ray;
  std::vector<uint8_t> desc;
  ptz_desc_set* set = nullptr;
  double build_ms = 0;
  // the HOME SET (ptz_landmark_shortlist.h): the landmarks grouped by home as a ptz_desc_set of n_ref images, built from the host
  // copies on the first request (ptz_landmark_map_home_set) and the map's until it is destroyed
  mutable std::mutex home_mutex;
  mutable ptz_desc_set* home_set = nullptr;
  mutable std::vector<int64_t> home_ptr;  // [n_ref + 1]
  mutable std::vector<int32_t> home_lm;   // [n_lm]
};

// A landmark view (ptz_landmark_visible, ptz_landmark_prior.hip): per query the landmarks its prior camera sees, and their packed
// descriptor rows gathered into a ptz_desc_set of n_query images whose key points are the predicted pixels, so that the guided
// matcher runs on it as on any set.  Everything stays on the device; only vis_ptr has a host copy (the one read that sizes the set).
struct ptz_landmark_view {
  int device = 0;
  int32_t kind = PTZ_LANDMARK_VIEW_PRIOR;  // PTZ_LANDMARK_VIEW_PRIOR, or _HOMES: no prior cameras, no H, no predicted pixels (null)
  int32_t n_query = 0, n_lm = 0;
  int64_t n_vis = 0;
  ptz::PoolBlock blk;               // [prior_cams | H | vis_ptr]
  const double* d_prior_cams = nullptr;  // [15 n_query]: the run's initial cameras take their focal, rotation and distortion
  const double* d_H = nullptr;           // [9 n_query]: identities, the guided matcher's H of pair (view image q, query q)
  const int64_t* d_vis_ptr = nullptr;    // [n_query + 1]
  const int32_t* d_vis_lm = nullptr;     // [n_vis], in the set's block
  const float* d_vis_uv = nullptr;       // [2 n_vis] = the set's key points
  std::vector<int64_t> vis_ptr;
  ptz_desc_set* set = nullptr;
  double device_ms = 0;
};
