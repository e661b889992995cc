// ptz_homography_bound.cc -- the adaptive RANSAC bound of the host estimator as a table (host code, built by the host C++
// compiler with the host library's flags: the bound is static_cast<int>(ceil(need)) of libm's log / pow, and the device's
// log / pow may differ from the host's in the last bit, so the kernel never evaluates it -- it reads this table).
#include "ptz_homography.h"

#include "../../include/ptz_calib_amd.h"

extern "C" int32_t ptz_debug_homography_bounds(int32_t n, int32_t* bound)
{
  if (n < 0 || !bound) return PTZ_EINVAL;
  for (int cnt = 0; cnt <= n; ++cnt) bound[cnt] = ptz::ptzh_adaptive_bound(cnt, n);
  return PTZ_OK;
}
