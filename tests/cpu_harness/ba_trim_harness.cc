// Host instantiation of the trimming selection rule (ptz-calib_amd/csrc/ptz_ba_trim.h, the header the kernel of ptz_ba_resid.hip
// instantiates): per-ray worst observation, the lower median, the threshold and the rejects, finished in plain loops.
// Build: g++ -O2 -ffp-contract=off -shared -fPIC -o libba_trim_harness.so ba_trim_harness.cc
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../ptz-calib_amd/csrc/ptz_ba_trim.h"

extern "C" {

// obs_ray [n_obs] non-decreasing, err [n_obs] = |e_o| in the same order.  Outputs: reject [n_obs], ray_max / ray_worst [n_ray]
// (ray_worst = -1 and ray_max = 0 for a ray without observations), threshold, median (NaN when the rule takes none).  Returns the
// number of rejects, -1 for a rule that is not valid.
int32_t ba_trim_harness_select(int64_t n_obs, int32_t n_ray, const int32_t* obs_ray, const double* err, double trim_px, double k_sigma, uint8_t* reject,
                               double* ray_max, int32_t* ray_worst, double* threshold, double* median)
{
  const ptz::TrimRule rule{trim_px, k_sigma, 2};
  if (!ptz::trim_rule_valid(rule)) return -1;
  double med = std::nan("");
  if (ptz::trim_needs_median(rule) && n_obs > 0) {
    std::vector<double> s(err, err + n_obs);
    const long long k = ptz::trim_median_index(n_obs);
    std::nth_element(s.begin(), s.begin() + k, s.end());
    med = s[k];
  }
  const double t = ptz::trim_threshold(rule, med);
  for (int64_t a = 0; a < n_obs; ++a) reject[a] = 0;
  for (int32_t r = 0; r < n_ray; ++r) { ray_max[r] = 0.0; ray_worst[r] = -1; }
  int32_t n_reject = 0;
  for (int64_t a0 = 0; a0 < n_obs;) {
    int64_t a1 = a0;
    while (a1 < n_obs && obs_ray[a1] == obs_ray[a0]) ++a1;
    const int32_t r = obs_ray[a0];
    double mx;
    int at;
    ptz::trim_ray_worst(err + a0, (int)(a1 - a0), mx, at);
    ray_max[r] = mx;
    ray_worst[r] = (int32_t)(a0 + at);
    if (ptz::trim_rejects(mx, t)) { reject[a0 + at] = 1; ++n_reject; }
    a0 = a1;
  }
  *threshold = t;
  *median = med;
  return n_reject;
}

// whether a ray with n_left observations survives re-packing
int32_t ba_trim_harness_survives(int32_t n_left)
{
  const ptz::TrimRule rule{1.0, 0.0, 2};
  return ptz::trim_ray_survives(rule, n_left) ? 1 : 0;
}

}  // extern "C"
