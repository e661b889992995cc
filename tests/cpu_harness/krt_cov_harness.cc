// krt_cov_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of the per-query covariance algebra in
// ptz-calib_amd/csrc/ptz_krt_cov.h (what k_krt_cov runs on the device) so it can be held to the oracle's functors without a
// GPU.  Never part of the product library.
#include <stdint.h>

#include "../../ptz-calib_amd/csrc/ptz_krt_cov.h"

using namespace ptz;

namespace {

// the constant part of a match as the kernels compute it (MatchEval::ray1 of ptz_krt_device.h, which is device code)
template <int KTYPE>
void ray1(const double* kref, const double* dref, float u1, float v1, double r[3], bool& skip)
{
  double u = u1, v = v1;
  skip = false;
  if (KTYPE & 1) {
    float ou, ov;
    undistort_point(kref[0], kref[1], kref[2], kref[3], dref, u1, v1, ou, ov);
    skip = (ou < 0 || ou >= kref[2] * 2 || ov < 0 || ov >= kref[3] * 2);
    u = ou; v = ov;
  }
  const double X0 = (u - kref[2]) / kref[0], X1 = (v - kref[3]) / kref[1];
  const double n = sqrt(X0 * X0 + X1 * X1 + 1.0);
  r[0] = X0 / n; r[1] = X1 / n; r[2] = 1.0 / n;
}

// one query, summed in the kernel's order: sixteen lanes stride over the matches and then the points, butterfly 8, 4, 2, 1
template <int KTYPE>
int run(int n_match, const float* uv_ref, const float* uv_cur, const unsigned char* mask, int n_pt, const float* pts2d,
        const double* pts3d, const double* ref, const double* cur, double pixel_sigma, double* cov, double* sigma0)
{
  constexpr int G = 16, COUNT = KrtCovSums<KTYPE>::COUNT;
  double x[15], Rref[9], R[9];
  krt_cov_local_frame(ref, cur, x, Rref, R);
  KrtCovSums<KTYPE> s[G];
  for (int lane = 0; lane < G; ++lane) {
    krt_cov_clear<KTYPE>(s[lane]);
    for (int m = lane; m < n_match; m += G) {
      if (mask && mask[m] == 0) continue;
      double r1[3];
      bool skip;
      ray1<KTYPE>(ref, ref + 10, uv_ref[2 * m], uv_ref[2 * m + 1], r1, skip);
      krt_cov_add_match<KTYPE>(s[lane], R, x, r1, skip, uv_cur[2 * m], uv_cur[2 * m + 1]);
    }
    for (int i = lane; i < n_pt; i += G) {
      const double* X = pts3d + 3 * i;
      double Xl[3];
      Xl[0] = Rref[0] * X[0] + Rref[1] * X[1] + Rref[2] * X[2] + ref[7];
      Xl[1] = Rref[3] * X[0] + Rref[4] * X[1] + Rref[5] * X[2] + ref[8];
      Xl[2] = Rref[6] * X[0] + Rref[7] * X[1] + Rref[8] * X[2] + ref[9];
      krt_cov_add_point<KTYPE>(s[lane], R, x, Xl, pts2d[2 * i], pts2d[2 * i + 1]);
    }
  }
  for (int off = G / 2; off >= 1; off /= 2) {
    KrtCovSums<KTYPE> t[G];
    for (int lane = 0; lane < G; ++lane)
      for (int k = 0; k < COUNT; ++k) t[lane].v[k] = s[lane].v[k] + s[lane ^ off].v[k];
    for (int lane = 0; lane < G; ++lane) s[lane] = t[lane];
  }
  return krt_cov_finish<KTYPE>(s[0], pixel_sigma, cov, sigma0);
}

}  // namespace

extern "C" {
// Status of the query (kCov*); cov [NF * NF] and sigma0 are written only with status 0.  mask / pts2d / pts3d may be null
// (n_pt = 0); pts3d are WORLD points; ref / cur are world-frame 15-vectors.  -1: unknown factor type.
int h_krt_cov(int factor_type, int n_match, const float* uv_ref, const float* uv_cur, const unsigned char* mask, int n_pt,
              const float* pts2d, const double* pts3d, const double* ref, const double* cur, double pixel_sigma, double* cov,
              double* sigma0)
{
  switch (factor_type) {
    case 0: return run<0>(n_match, uv_ref, uv_cur, mask, n_pt, pts2d, pts3d, ref, cur, pixel_sigma, cov, sigma0);
    case 1: return run<1>(n_match, uv_ref, uv_cur, mask, n_pt, pts2d, pts3d, ref, cur, pixel_sigma, cov, sigma0);
    case 2: return run<2>(n_match, uv_ref, uv_cur, mask, n_pt, pts2d, pts3d, ref, cur, pixel_sigma, cov, sigma0);
    case 3: return run<3>(n_match, uv_ref, uv_cur, mask, n_pt, pts2d, pts3d, ref, cur, pixel_sigma, cov, sigma0);
    default: return -1;
  }
}
}
