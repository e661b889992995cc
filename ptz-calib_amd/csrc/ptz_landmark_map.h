// ptz_landmark_map.h -- what a landmark map is (ptz_landmark_map_create, ptz_landmark.hip), for the serving loop that runs against
// one (ptz_relocalizer.hip).  The rays and homes stay on the device for the assembly; every array has a host copy for
// ptz_landmark_map_download; the descriptors live in a ptz_desc_set of ONE image of n_lm features (placeholder key points, all zero:
// the matcher gathers uv_a from them and nobody reads it), so the distances stay on the matcher's kernels.
#pragma once

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
};
