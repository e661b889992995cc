// ptz_tracks_obj.h -- what a ptz_tracks is (ptz_tracks.hip), for the landmark map that is built from one (ptz_landmark.hip).  The
// arrays stay on the device, at the extents ptz_tracks_build_device asks for; the host holds the sizes and the counts only.
#pragma once

#include "ptz_common.h"
#include "ptz_host_batch.h"

struct ptz_tracks {
  int device = 0;
  int32_t n_img = 0, n_track = 0, min_len = 2;
  int64_t n_feat = 0, n_view = 0;
  int64_t counts[4] = {0, 0, 0, 0};  // matched nodes, components, dropped for a repeated image, dropped as short
  ptz::PoolBlock blk;
  int64_t* d_trk_ptr = nullptr;  // [n_track + 1]
  int32_t *d_trk_img = nullptr, *d_trk_feat = nullptr, *d_trk_node = nullptr;  // [n_view]
  float* d_trk_uv = nullptr;     // [2 n_view]
  double device_ms = 0;
};
