// homography_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of the device math in
// ptz-calib_amd/csrc/ptz_homography.h (the batched RANSAC homography estimator) so it can be held to the host estimator
// (host/homography.cc) bit for bit without a GPU.  Never part of the product library.
#include <vector>

#include "../../ptz-calib_amd/csrc/ptz_homography.h"

using namespace ptz;

extern "C" {
// The estimator for one pair, composed as the header's sequential form: returns 1 and fills H9 (and mask[n]) or 0.
int h_find_homography(int n, const float* src, const float* dst, double thresh, double* H9, unsigned char* mask)
{
  std::vector<int32_t> bound(n > 0 ? n + 1 : 1);
  for (int c = 0; c <= n; ++c) bound[c] = ptzh_adaptive_bound(c, n);
  std::vector<int> inl(n > 0 ? n : 1);
  return ptzh_find_homography_seq(n, src, dst, thresh, bound.data(), inl.data(), H9, mask);
}

// bound[cnt] for cnt = 0 .. n
void h_adaptive_bounds(int n, int32_t* bound)
{
  for (int c = 0; c <= n; ++c) bound[c] = ptzh_adaptive_bound(c, n);
}
}
