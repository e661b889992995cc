// ba_cov_georef_harness.cc -- TEST INFRASTRUCTURE.  Host instantiation of the georeferenced-covariance algebra of
// ptz-calib_amd/csrc/ptz_ba_cov_georef.h (and of the 2D-2D algebra of ptz_ba_cov.h it builds on), what the georef kernels of
// ptz_ba_cov.hip run on the device: the per-ray, per-annotation and per-camera functions come from the headers; the dense
// assembly, the inverse and the sandwich are plain serial loops here, every sum in the kernels' order (a camera's annotations and
// the (L, L) block in stored order).  Never part of the product library.
#include "../../ptz-calib_amd/csrc/ptz_ba_cov_georef.h"
#include "ba_cov_common.h"

using namespace cov_harness;

namespace {

struct Problem {
  int n_cam, n_ray;
  int64_t n_obs;
  const float* uv; const int* ocam; const int* oray; const double* rw;
  int n_o3;
  const float* o3uv; const double* o3xyz; const int* o3cam;
  const double *cam, *ray, *tlw;
};

template <int TYPE>
int run(const Problem& p, int gauge, double pixel_sigma, double annotation_sigma, double* cov, double* cov_centre, double* sigma0)
{
  constexpr int NF = BaDims<TYPE>::NC, NE = NF * NF, NC = NF + 1, NZ = NC + 6, REC = ba_geo_rec(NC);
  const int n_cam = p.n_cam, nL = NC * n_cam, n = nL + 6;
  std::vector<double> cb((size_t)n_cam * CAMBLK), S((size_t)n * n, 0.0), Tf((size_t)n * n, 0.0), Ta((size_t)n * n, 0.0);
  for (int c = 0; c < n_cam; ++c) ba_cov_camblk(p.cam + 15 * (size_t)c, &cb[(size_t)c * CAMBLK]);
  double tb[TLWBLK];
  ba_geo_tlwblk(p.tlw, tb);
  int flags = 0;
  double sse_f = 0, sse_a = 0;
  // ---- the 2D-2D part, as ba_cov_harness.cc, its columns at ba_geo_pos
  ray_loop<TYPE>(p.n_obs, p.uv, p.ocam, p.oray, p.rw, cb.data(), p.ray, n, [](int c, int k) { return c * NC + ba_geo_pos(k); }, S, Tf, sse_f, flags);
  // ---- the annotations, in stored order
  std::vector<char> live(n_cam, 0);
  for (int a = 0; a < p.n_o3; ++a) {
    const int c = p.o3cam[a];
    double rec[REC];
    if (!ba_geo_annot<TYPE>(&cb[(size_t)c * CAMBLK], tb, p.o3xyz + 3 * (size_t)a, p.o3uv[2 * a], p.o3uv[2 * a + 1], rec)) flags |= kBaCovBehind;
    live[c] = 1;
    sse_a += rec[2 * NC + 12];
    for (int k = 0; k < NC; ++k) {
      for (int l = 0; l < NC; ++l) {
        const double v = ba_geo_cc(rec, NC, k, l);
        S[(size_t)(c * NC + k) * n + c * NC + l] += v; Ta[(size_t)(c * NC + k) * n + c * NC + l] += v;
      }
      for (int m = 0; m < 6; ++m) {
        const double v = ba_geo_cl(rec, NC, k, m);
        S[(size_t)(c * NC + k) * n + nL + m] += v; S[(size_t)(nL + m) * n + c * NC + k] += v;
        Ta[(size_t)(c * NC + k) * n + nL + m] += v; Ta[(size_t)(nL + m) * n + c * NC + k] += v;
      }
    }
    for (int m = 0; m < 6; ++m)
      for (int q = 0; q < 6; ++q) {
        const double v = ba_geo_ll(rec, NC, m, q);
        S[(size_t)(nL + m) * n + nL + q] += v; Ta[(size_t)(nL + m) * n + nL + q] += v;
      }
  }
  int n_ann = 0;
  for (int c = 0; c < n_cam; ++c) n_ann += live[c];
  double est2[2], var[2];
  ba_geo_noise(NF, n_cam, p.n_ray, p.n_obs, p.n_o3, n_ann, sse_f, sse_a, pixel_sigma, annotation_sigma, est2, var);
  // ---- identity rows (the gauge, the dead fy columns), unit diagonal, M
  const int r0 = gauge * NC + NC - 3;
  std::vector<char> ident(n, 0);
  for (int i = r0; i < r0 + 3; ++i) ident[i] = 1;
  for (int c = 0; c < n_cam; ++c) if (!live[c]) ident[c * NC + 1] = 1;
  std::vector<double> sc(n, 1.0), M((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) {
    if (ident[i]) continue;
    const double d = S[(size_t)i * n + i];
    if (!(d > 0.0) || !isfinite(d)) flags |= kBaCovBadDiag; else sc[i] = 1.0 / sqrt(d);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const bool g = ident[i] || ident[j];
      const size_t e = (size_t)i * n + j;
      S[e] = g ? (i == j ? 1.0 : 0.0) : S[e] * sc[i] * sc[j];
      M[e] = g ? 0.0 : (var[0] * Tf[e] + var[1] * Ta[e]) * sc[i] * sc[j];
    }
  int fail = 0;
  if (!flags && !spd_inverse(S, n)) fail = 1;
  std::vector<double> out((size_t)n_cam * NE, 0.0);
  double cen[3], cc[9];
  if (!flags && !fail) {
    std::vector<double> G((size_t)n * n, 0.0), Cf((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < n; ++k) {
        const double s = S[(size_t)i * n + k];
        if (s == 0.0) continue;
        for (int j = 0; j < n; ++j) G[(size_t)i * n + j] += s * M[(size_t)k * n + j];
      }
    // the blocks (c, c), (c, L), (L, L) of G S^-1, unscaled (lower triangle, mirrored)
    auto Cij = [&](int i, int j) {
      double v = 0;
      for (int q = 0; q < n; ++q) v += G[(size_t)i * n + q] * S[(size_t)j * n + q];
      return v * sc[i] * sc[j];
    };
    double CLL[36];
    for (int m = 0; m < 6; ++m)
      for (int q = 0; q <= m; ++q) { CLL[6 * m + q] = Cij(nL + m, nL + q); CLL[6 * q + m] = CLL[6 * m + q]; }
    for (int c = 0; c < n_cam; ++c) {
      double Z[NZ * NZ];
      for (int k = 0; k < NC; ++k)
        for (int l = 0; l <= k; ++l) { Z[k * NZ + l] = Cij(c * NC + k, c * NC + l); Z[l * NZ + k] = Z[k * NZ + l]; }
      for (int k = 0; k < NC; ++k)
        for (int m = 0; m < 6; ++m) { Z[k * NZ + NC + m] = Cij(c * NC + k, nL + m); Z[(NC + m) * NZ + k] = Z[k * NZ + NC + m]; }
      for (int m = 0; m < 6; ++m)
        for (int q = 0; q < 6; ++q) Z[(NC + m) * NZ + NC + q] = CLL[6 * m + q];
      const double* cbc = &cb[(size_t)c * CAMBLK];
      double W[NF * NZ];
      ba_geo_world_W<TYPE>(cbc + CB_JL, cbc + CB_R, tb, W);
      for (int k = 0; k < NF; ++k)
        for (int l = 0; l <= k; ++l) {
          const double v = ba_geo_quad(W + k * NZ, W + l * NZ, Z, NZ, NZ);
          if (!isfinite(v)) flags |= kBaCovNonFinite;
          out[(size_t)c * NE + k * NF + l] = v; out[(size_t)c * NE + l * NF + k] = v;
        }
    }
    double J[18];
    ba_geo_centre_J(tb, cen, J);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j <= i; ++j) {
        const double v = ba_geo_quad(J + 6 * i, J + 6 * j, CLL, 6, 6);
        if (!isfinite(v)) flags |= kBaCovNonFinite;
        cc[3 * i + j] = v; cc[3 * j + i] = v;
      }
    if (!isfinite(est2[0]) || !isfinite(est2[1])) flags |= kBaCovNonFinite;
  }
  const int st = ba_geo_status(NF, n_cam, p.n_ray, p.n_obs, p.n_o3, n_ann, fail, flags);
  if (st == kBaCovOk) {
    for (size_t k = 0; k < out.size(); ++k) cov[k] = out[k];
    for (int k = 0; k < 9; ++k) cov_centre[k] = cc[k];
    sigma0[0] = sqrt(est2[0]); sigma0[1] = sqrt(est2[1]);
  }
  return st;
}

}  // namespace

extern "C" {

int32_t ba_geo_harness_dim(int32_t type) { return ba_geo_cov_dim(type); }
int32_t ba_geo_harness_status(int32_t nf2, int64_t n_cam, int64_t n_ray, int64_t n_obs, int64_t n_obs3d, int64_t n_ann_cam, int32_t chol_fail,
                              int32_t flags)
{
  return ba_geo_status(nf2, n_cam, n_ray, n_obs, n_obs3d, n_ann_cam, chol_fail, flags);
}

// the whole computation of one problem; cov [NF NF n_cam], cov_centre [9] and sigma0 [2] are written only with status 0
int32_t ba_geo_harness_run(int32_t type, int32_t n_cam, int32_t n_ray, int64_t n_obs, const float* uv, const int32_t* ocam, const int32_t* oray,
                           const double* rw, int32_t n_o3, const float* o3uv, const double* o3xyz, const int32_t* o3cam, const double* cam,
                           const double* ray, const double* tlw, int32_t gauge, double pixel_sigma, double annotation_sigma, double* cov,
                           double* cov_centre, double* sigma0)
{
  const Problem p{n_cam, n_ray, n_obs, uv, ocam, oray, rw, n_o3, o3uv, o3xyz, o3cam, cam, ray, tlw};
  switch (type) {
    case 0: return run<0>(p, gauge, pixel_sigma, annotation_sigma, cov, cov_centre, sigma0);
    case 1: return run<1>(p, gauge, pixel_sigma, annotation_sigma, cov, cov_centre, sigma0);
    default: return -1;
  }
}

}  // extern "C"
