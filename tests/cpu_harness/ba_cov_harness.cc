// ba_cov_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of the bundle-adjustment covariance algebra in
// ptz-calib_amd/csrc/ptz_ba_cov.h (what the kernels of ptz_ba_cov.hip run on the device): the per-ray and per-camera functions
// come from the header, the dense assembly, the inverse and the sandwich are plain serial loops here.  Never part of the
// product library.
#include "ba_cov_common.h"

using namespace cov_harness;

namespace {

template <int TYPE>
int run(int n_cam, int n_ray, int64_t n_obs, const float* uv, const int* ocam, const int* oray, const double* rw, const double* cam,
        const double* ray, int gauge, double pixel_sigma, double* cov, double* sigma0)
{
  constexpr int NF = BaDims<TYPE>::NC, NE = NF * NF;
  const int n = NF * n_cam;
  std::vector<double> cb((size_t)n_cam * CAMBLK), S((size_t)n * n, 0.0), T((size_t)n * n, 0.0);
  for (int c = 0; c < n_cam; ++c) ba_cov_camblk(cam + 15 * (size_t)c, &cb[(size_t)c * CAMBLK]);
  int flags = 0;
  double sse = 0;
  ray_loop<TYPE>(n_obs, uv, ocam, oray, rw, cb.data(), ray, n, [](int c, int k) { return c * NF + k; }, S, T, sse, flags);
  // gauge, unit diagonal
  const int r0 = gauge * NF + NF - 3;
  std::vector<double> sc(n, 1.0);
  for (int i = 0; i < n; ++i) {
    if (i >= r0 && i < r0 + 3) continue;
    const double d = S[(size_t)i * n + i];
    if (!(d > 0.0) || !isfinite(d)) flags |= kBaCovBadDiag; else sc[i] = 1.0 / sqrt(d);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const bool g = (i >= r0 && i < r0 + 3) || (j >= r0 && j < r0 + 3);
      S[(size_t)i * n + j] = g ? (i == j ? 1.0 : 0.0) : S[(size_t)i * n + j] * sc[i] * sc[j];
      T[(size_t)i * n + j] = g ? 0.0 : T[(size_t)i * n + j] * sc[i] * sc[j];
    }
  int fail = 0;
  if (!flags && !spd_inverse(S, n)) fail = 1;
  const double dof = (double)ba_cov_dof(NF, n_cam, n_ray, n_obs);
  const double s2 = sse / dof, var = pixel_sigma > 0.0 ? pixel_sigma * pixel_sigma : s2;
  std::vector<double> out((size_t)n_cam * NE, 0.0);
  if (!flags && !fail) {
    std::vector<double> G((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < n; ++k) {
        const double s = S[(size_t)i * n + k];
        if (s == 0.0) continue;
        for (int j = 0; j < n; ++j) G[(size_t)i * n + j] += s * T[(size_t)k * n + j];
      }
    for (int c = 0; c < n_cam; ++c) {
      double Cr[NE];
      for (int k = 0; k < NF; ++k)
        for (int l = 0; l < NF; ++l) {
          double v = 0;
          for (int j = 0; j < n; ++j) v += G[(size_t)(c * NF + k) * n + j] * S[(size_t)(c * NF + l) * n + j];
          Cr[k * NF + l] = v * sc[c * NF + k] * sc[c * NF + l];
        }
      if (!ba_cov_to_left<TYPE>(Cr, &cb[(size_t)c * CAMBLK + CB_JL], var, c == gauge, &out[(size_t)c * NE])) flags |= kBaCovNonFinite;
    }
    if (!isfinite(s2)) flags |= kBaCovNonFinite;
  }
  const int st = ba_cov_status(NF, n_cam, n_ray, n_obs, fail, flags);
  if (st == kBaCovOk) {
    for (size_t k = 0; k < out.size(); ++k) cov[k] = out[k];
    *sigma0 = sqrt(s2);
  }
  return st;
}

// one ray seen by `len` cameras: V = w sum B^T B [9], E_o [len][NF][3] and the header's blocks E_o P_r E_o'^T [len NF][len NF]
template <int TYPE>
int ray_blocks(int len, const double* cams, const float* uv, const double* X, double w, double* Vout, double* Eout, double* EPE)
{
  constexpr int NF = BaDims<TYPE>::NC;
  double V[6] = {0, 0, 0, 0, 0, 0};
  std::vector<double> Y((size_t)len * 3 * NF);
  for (int o = 0; o < len; ++o) {
    double cb[CAMBLK], res[2], Jc[2][NF], Jr[2][3];
    ba_cov_camblk(cams + 15 * (size_t)o, cb);
    ba_linearize<TYPE>(cb, X, uv[2 * o], uv[2 * o + 1], res, Jc, Jr);
    ba_cov_add_V(Jr, V);
    ba_cov_E<NF>(Jc, Jr, w, Eout + (size_t)o * 3 * NF);
  }
  const double Vf[9] = {V[0], V[1], V[3], V[1], V[2], V[4], V[3], V[4], V[5]};
  for (int k = 0; k < 9; ++k) Vout[k] = w * Vf[k];
  double P[6];
  if (!ba_cov_ray_P(V, w, X, P)) return 1;
  for (int o = 0; o < len; ++o) ba_cov_Y<NF>(Eout + (size_t)o * 3 * NF, P, &Y[(size_t)o * 3 * NF]);
  const int m = len * NF;
  for (int o = 0; o < len; ++o)
    for (int p = 0; p < len; ++p)
      for (int k = 0; k < NF; ++k)
        for (int l = 0; l < NF; ++l) EPE[(size_t)(o * NF + k) * m + p * NF + l] = -ba_cov_pair_term(&Y[(size_t)o * 3 * NF], Eout + (size_t)p * 3 * NF, k, l);
  return 0;
}

}  // namespace

extern "C" {

int32_t ba_cov_harness_dim(int32_t type) { return ba_cov_dim(type); }
int32_t ba_cov_harness_status(int32_t nf, int64_t n_cam, int64_t n_ray, int64_t n_obs, int32_t chol_fail, int32_t flags)
{
  return ba_cov_status(nf, n_cam, n_ray, n_obs, chol_fail, flags);
}

// the whole computation of one problem; cov [NF NF n_cam] and sigma0 are written only with status 0
int32_t ba_cov_harness_run(int32_t type, int32_t n_cam, int32_t n_ray, int64_t n_obs, const float* uv, const int32_t* ocam, const int32_t* oray,
                           const double* rw, const double* cam, const double* ray, int32_t gauge, double pixel_sigma, double* cov, double* sigma0)
{
  switch (type) {
    case 0: return run<0>(n_cam, n_ray, n_obs, uv, ocam, oray, rw, cam, ray, gauge, pixel_sigma, cov, sigma0);
    case 1: return run<1>(n_cam, n_ray, n_obs, uv, ocam, oray, rw, cam, ray, gauge, pixel_sigma, cov, sigma0);
    case 2: return run<2>(n_cam, n_ray, n_obs, uv, ocam, oray, rw, cam, ray, gauge, pixel_sigma, cov, sigma0);
    default: return -1;
  }
}

int32_t ba_cov_harness_ray(int32_t type, int32_t len, const double* cams, const float* uv, const double* X, double w, double* V, double* E, double* EPE)
{
  switch (type) {
    case 0: return ray_blocks<0>(len, cams, uv, X, w, V, E, EPE);
    case 1: return ray_blocks<1>(len, cams, uv, X, w, V, E, EPE);
    case 2: return ray_blocks<2>(len, cams, uv, X, w, V, E, EPE);
    default: return -1;
  }
}

}  // extern "C"
