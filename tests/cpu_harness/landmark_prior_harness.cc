// landmark_prior_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of ptz-calib_amd/csrc/ptz_landmark_prior.h: per query the
// landmarks in ascending index, each through landmark_predict -- so that it can be held to the numpy restatement
// (tests/landmark_prior_util.py) without a GPU and the device to it.  Never part of the product library.
// Build: g++ -O2 -ffp-contract=off -shared -fPIC -o liblandmark_prior_harness.so landmark_prior_harness.cc
#include <stdint.h>

#include "../../ptz-calib_amd/csrc/ptz_landmark_prior.h"

using namespace ptz;

extern "C" {

// vis_ptr [n_query + 1] is always complete; vis_lm / vis_uv (nullable together: a counting call) take at most `capacity` entries.
// Returns n_vis.
int64_t h_landmark_visible(int32_t n_lm, const double* lm_ray, int32_t n_query, const double* prior_cams, const double* prior_R,
                           const int32_t* query_wh, int32_t factor_type, double radius_px, int64_t* vis_ptr, int32_t* vis_lm, float* vis_uv,
                           int64_t capacity)
{
  int64_t o = 0;
  vis_ptr[0] = 0;
  for (int q = 0; q < n_query; ++q) {
    double K4[4];
    const int32_t w = query_wh[2 * q], h = query_wh[2 * q + 1];
    prior_query_K(prior_cams + 15 * (int64_t)q, w, h, factor_type, K4);
    for (int32_t l = 0; l < n_lm; ++l) {
      const LandmarkSeen s = landmark_predict(K4, prior_R + 9 * (int64_t)q, w, h, radius_px, lm_ray + 3 * (int64_t)l);
      if (!s.visible) continue;
      if (vis_lm && o < capacity) {
        vis_lm[o] = l;
        vis_uv[2 * o] = s.u;
        vis_uv[2 * o + 1] = s.v;
      }
      ++o;
    }
    vis_ptr[q + 1] = o;
  }
  return o;
}
}
