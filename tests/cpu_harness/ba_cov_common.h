// ba_cov_common.h -- TEST INFRASTRUCTURE.  What ba_cov_harness.cc and ba_cov_georef_harness.cc share: the dense inverse and the
// 2D-2D part of the reduced system (the per-ray functions come from ptz-calib_amd/csrc/ptz_ba_cov.h, the assembly is plain serial
// loops).  Never part of the product library.
#pragma once

#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../ptz-calib_amd/csrc/ptz_ba_cov.h"

namespace cov_harness {

using namespace ptz;

// in-place inverse of a symmetric positive definite n x n matrix (row-major) through its Cholesky factor; false: a pivot <= 0
inline bool spd_inverse(std::vector<double>& A, int n)
{
  std::vector<double> L((size_t)n * n, 0.0), W((size_t)n * n, 0.0);
  for (int j = 0; j < n; ++j) {
    double d = A[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
    if (!(d > 0.0)) return false;
    const double l = sqrt(d);
    L[(size_t)j * n + j] = l;
    for (int i = j + 1; i < n; ++i) {
      double v = A[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) v -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
      L[(size_t)i * n + j] = v / l;
    }
  }
  for (int c = 0; c < n; ++c)  // W = L^-1
    for (int i = c; i < n; ++i) {
      double v = i == c ? 1.0 : 0.0;
      for (int k = c; k < i; ++k) v -= L[(size_t)i * n + k] * W[(size_t)k * n + c];
      W[(size_t)i * n + c] = v / L[(size_t)i * n + i];
    }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double v = 0;
      for (int k = i; k < n; ++k) v += W[(size_t)k * n + i] * W[(size_t)k * n + j];
      A[(size_t)i * n + j] = v; A[(size_t)j * n + i] = v;
    }
  return true;
}

// The 2D-2D terms of every ray (observations ray-major: uv, ocam, oray; weights rw; camera blocks cb; ray parameters ray) added into
// S and T (n x n, row-major), the squared residuals into sse, what a ray raises into flags.  row(c, k): the row of camera c's
// 2D-2D column k.
template <int TYPE, class Row>
void ray_loop(int64_t n_obs, const float* uv, const int* ocam, const int* oray, const double* rw, const double* cb, const double* ray, int n, Row row,
              std::vector<double>& S, std::vector<double>& T, double& sse, int& flags)
{
  constexpr int NF = BaDims<TYPE>::NC;
  std::vector<double> E, Y;
  for (int64_t a0 = 0; a0 < n_obs;) {
    int64_t a1 = a0;
    while (a1 < n_obs && oray[a1] == oray[a0]) ++a1;
    const int r = oray[a0];
    const double* X = ray + 3 * (size_t)r;
    const double w = rw[r];
    const int len = (int)(a1 - a0);
    double V[6] = {0, 0, 0, 0, 0, 0};
    E.assign((size_t)len * 3 * NF, 0.0); Y.assign((size_t)len * 3 * NF, 0.0);
    std::vector<double> JcAll((size_t)len * 2 * NF);
    for (int o = 0; o < len; ++o) {
      const double* c = cb + (size_t)ocam[a0 + o] * CAMBLK;
      double res[2], Jc[2][NF], Jr[2][3];
      ba_linearize<TYPE>(c, X, uv[2 * (a0 + o)], uv[2 * (a0 + o) + 1], res, Jc, Jr);
      if (TYPE == 1 && c[CB_R + 6] * X[0] + c[CB_R + 7] * X[1] + c[CB_R + 8] * X[2] < 0) flags |= kBaCovPenalty;
      ba_cov_add_V(Jr, V);
      sse += res[0] * res[0] + res[1] * res[1];
      ba_cov_E<NF>(Jc, Jr, w, &E[(size_t)o * 3 * NF]);
      for (int k = 0; k < NF; ++k) { JcAll[(size_t)o * 2 * NF + k] = Jc[0][k]; JcAll[(size_t)o * 2 * NF + NF + k] = Jc[1][k]; }
    }
    a0 = a1;
    if (len < 2) continue;  // contributes exactly zero
    double P[6];
    if (!ba_cov_ray_P(V, w, X, P)) { flags |= kBaCovBadRay; continue; }
    for (int o = 0; o < len; ++o) ba_cov_Y<NF>(&E[(size_t)o * 3 * NF], P, &Y[(size_t)o * 3 * NF]);
    for (int o = 0; o < len; ++o) {
      const int co = ocam[a1 - len + o];
      double Jc[2][NF];
      for (int k = 0; k < NF; ++k) { Jc[0][k] = JcAll[(size_t)o * 2 * NF + k]; Jc[1][k] = JcAll[(size_t)o * 2 * NF + NF + k]; }
      for (int k = 0; k < NF; ++k)
        for (int l = 0; l <= k; ++l) {
          const double v = ba_cov_diag_term<NF>(Jc, w, &Y[(size_t)o * 3 * NF], &E[(size_t)o * 3 * NF], k, l);
          const size_t i = (size_t)row(co, k), j = (size_t)row(co, l);
          S[i * n + j] += v; T[i * n + j] += w * v;
          if (l < k) { S[j * n + i] += v; T[j * n + i] += w * v; }
        }
      for (int q = 0; q < len; ++q) {
        const int cq = ocam[a1 - len + q];
        if (cq >= co) continue;  // block (co, cq), co > cq, and its mirror
        for (int k = 0; k < NF; ++k)
          for (int l = 0; l < NF; ++l) {
            const double v = ba_cov_pair_term(&Y[(size_t)o * 3 * NF], &E[(size_t)q * 3 * NF], k, l);
            const size_t i = (size_t)row(co, k), j = (size_t)row(cq, l);
            S[i * n + j] += v; S[j * n + i] += v;
            T[i * n + j] += w * v; T[j * n + i] += w * v;
          }
      }
    }
  }
}

}  // namespace cov_harness
