// ptz_ba_trim.h -- the outlier selection rule of the trimmed bundle adjustment (ptz_ba_batch_trim_select, ptz_ba_solve_trimmed*).
//
// PTZ_HD like ptz_factor.h: the kernel of ptz_ba_resid.hip and the host code (ptz_ba_trim.cc, tests/cpu_harness/ba_trim_harness.cc)
// instantiate the same functions.
//
// The rule.  Parameters: trim_px > 0, k_sigma >= 0, min_ray_obs = 2.  Given a problem's residual report (ptz_ba_batch_residuals):
//   t = max(trim_px, k_sigma * median / 1.1774)      median: the exact lower median of |e_o| over the problem's observations;
//                                                    1.1774 = sqrt(2 ln 2): the median of a Rayleigh variable with unit per-axis
//                                                    sigma, so median / 1.1774 estimates the per-axis pixel noise robustly.
//                                                    k_sigma = 0: t = trim_px, and no median is taken.
//   ray r rejects ONE observation at most: ray_worst[r] (the largest |e_o| of the track, the lowest index on a tie), if
//   ray_max[r] > t.  Nothing else is rejected: one wrong observation drags its whole ray and the cameras with it, so the other
//   observations of its track are judged again after the next solve.
//   Re-packing (ptz_ba_problem_trim) then drops a ray left with fewer than min_ray_obs observations, with what it still had.
#pragma once

#if !defined(PTZ_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PTZ_HD __host__ __device__ __forceinline__
#else
#define PTZ_HD inline
#endif
#endif

namespace ptz {

constexpr double kTrimRayleighMedian = 1.1774;

struct TrimRule {
  double trim_px;   // > 0
  double k_sigma;   // >= 0
  int min_ray_obs;  // 2
};

PTZ_HD bool trim_rule_valid(const TrimRule& r) { return r.trim_px > 0.0 && r.trim_px < 1e300 && r.k_sigma >= 0.0 && r.k_sigma < 1e300 && r.min_ray_obs == 2; }
PTZ_HD bool trim_needs_median(const TrimRule& r) { return r.k_sigma > 0.0; }
// position of the lower median in the sorted errors of a problem of n_obs observations
PTZ_HD long long trim_median_index(long long n_obs) { return (n_obs - 1) / 2; }
PTZ_HD double trim_threshold(const TrimRule& r, double median)
{
  if (!trim_needs_median(r)) return r.trim_px;
  const double s = r.k_sigma * median / kTrimRayleighMedian;
  return s > r.trim_px ? s : r.trim_px;
}
// the worst observation of a ray: err[0 .. n) its errors in stored order; at = position of the largest, the first on a tie
PTZ_HD void trim_ray_worst(const double* err, int n, double& mx, int& at)
{
  mx = err[0]; at = 0;
  for (int k = 1; k < n; ++k)
    if (err[k] > mx) { mx = err[k]; at = k; }
}
PTZ_HD bool trim_rejects(double ray_max, double t) { return ray_max > t; }
PTZ_HD bool trim_ray_survives(const TrimRule& r, int n_left) { return n_left >= r.min_ray_obs; }

}  // namespace ptz
