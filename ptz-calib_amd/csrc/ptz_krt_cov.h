// ptz_krt_cov.h -- covariance of one relocalized camera: the per-query algebra (FP64).
//
// PTZ_HD like ptz_factor.h: k_krt_cov (ptz_krt_cov.hip) instantiates these functions on the device, tests/cpu_harness
// instantiates them on the host to hold the algebra to the oracle's functors without a GPU.
//
// Definition.  The refined camera of a query is moved into the local frame of its reference camera as k_krt does
// (krt_optimizer.cc:269-284).  Free parameters p = [fx, (fy), d1, d2, d3, (k1)] (NF = KrtDims<KTYPE>::NF, the column order of
// krt_eval); d is a LEFT perturbation of the current rotation, R <- Exp(d) R, in radians about the current camera's own x, y, z
// axes -- krt_eval<KTYPE, true> with Jl = I.  R_world = R_local R_ref, so the same d perturbs the world rotation: the covariance
// does not depend on the reference view it was expressed in.  Over the residual blocks that count (matches whose mask byte is
// non-zero and that the border guard does not skip, and every 2D-3D point; B of them, m = 2 B residuals)
//   N = J^T J,  cost = 1/2 sum r^2,  sigma0^2 = 2 cost / (m - NF),
//   C = sigma0^2 N^-1 (pixel_sigma == 0, a-posteriori)  or  pixel_sigma^2 N^-1 (a-priori).
// N is scaled to unit diagonal (s_k = 1 / sqrt(N_kk)), factored by Cholesky, inverted and unscaled.
#pragma once

#include "ptz_factor.h"

namespace ptz {

// per-query status (the values of PTZ_COV_* in ptz_calib_amd.h)
constexpr int kCovOk = 0, kCovDof = 1, kCovSingular = 2, kCovSkipped = 3;
// a pivot of the unit-diagonal matrix at or below this is SINGULAR: beyond it the condition number leaves fewer than the six digits the
// covariance is held to, while round-off in forming a pivot stays near NF M 2^-53 (3e-12 at 5 000 matches)
constexpr double kCovMinPivot = 1e-10;

// sums of one query: N packed lower (row k: entries k (k + 1) / 2 .. + k), the cost, and the number of blocks that counted
template <int KTYPE> struct KrtCovSums {
  static constexpr int NF = KrtDims<KTYPE>::NF, NH = NF * (NF + 1) / 2, COUNT = NH + 2;
  double v[COUNT];  // [0, NH) N, [NH] cost, [NH + 1] blocks (an integer held as a double: exact)
};

template <int KTYPE> PTZ_HD void krt_cov_clear(KrtCovSums<KTYPE>& s)
{
#pragma unroll
  for (int k = 0; k < KrtCovSums<KTYPE>::COUNT; ++k) s.v[k] = 0;
}

// The query's cameras: x = current camera in the local frame of the reference camera, Rref / R = rotation of the reference (world) and of
// the current camera (local).  The arithmetic of k_krt's prologue.
PTZ_HD void krt_cov_local_frame(const double ref[15], const double cur[15], double x[15], double Rref[9], double R[9])
{
#pragma unroll
  for (int k = 0; k < 15; ++k) x[k] = cur[k];
  double Rcur[9], RrefT[9], Rl[9], rv[3];
  rodrigues(ref + 4, Rref);
  rodrigues(x + 4, Rcur);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) RrefT[3 * i + j] = Rref[3 * j + i];
  mat3_mul(Rcur, RrefT, Rl);
  rodrigues_inv(Rl, rv);
  const double t0 = Rl[0] * ref[7] + Rl[1] * ref[8] + Rl[2] * ref[9];
  const double t1 = Rl[3] * ref[7] + Rl[4] * ref[8] + Rl[5] * ref[9];
  const double t2 = Rl[6] * ref[7] + Rl[7] * ref[8] + Rl[8] * ref[9];
  x[4] = rv[0]; x[5] = rv[1]; x[6] = rv[2];
  x[7] = -t0 + x[7]; x[8] = -t1 + x[8]; x[9] = -t2 + x[9];
  rodrigues(x + 4, R);  // the rotation the solve's functors see: of the local rotation VECTOR
}

template <int KTYPE> PTZ_HD void krt_cov_add_block(KrtCovSums<KTYPE>& s, const double res[2], const double J[2][KrtDims<KTYPE>::NF])
{
  constexpr int NF = KrtDims<KTYPE>::NF, NH = KrtCovSums<KTYPE>::NH;
  int e = 0;
#pragma unroll
  for (int k = 0; k < NF; ++k)
#pragma unroll
    for (int l = 0; l <= k; ++l) s.v[e++] += J[0][k] * J[0][l] + J[1][k] * J[1][l];
  s.v[NH] += 0.5 * (res[0] * res[0] + res[1] * res[1]);
  s.v[NH + 1] += 1.0;
}

// one match: ray1 / skip = unit ray of the reference pixel and the border guard (MatchEval::ray1), uv2 = current pixel.  A skipped match
// is no residual block.
template <int KTYPE>
PTZ_HD void krt_cov_add_match(KrtCovSums<KTYPE>& s, const double* R, const double x[15], const double ray1[3], bool skip, float u2, float v2)
{
  if (skip) return;
  const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double res[2], J[2][KrtDims<KTYPE>::NF];
  krt_eval<KTYPE, true>(R, I3, x[0], (KTYPE & 2) ? x[1] : x[0], x[2], x[3], x + 10, ray1, false, u2, v2, res, J);
  krt_cov_add_block<KTYPE>(s, res, J);
}

// one 2D-3D point, already in the local frame (R_ref X_w + t_ref)
template <int KTYPE>
PTZ_HD void krt_cov_add_point(KrtCovSums<KTYPE>& s, const double* R, const double x[15], const double Xl[3], float u, float v)
{
  const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double res[2], J[2][KrtDims<KTYPE>::NF];
  krt_eval_2d3d<KTYPE, true>(R, I3, x[0], (KTYPE & 2) ? x[1] : x[0], x[2], x[3], x + 10, x + 7, Xl, u, v, res, J);
  krt_cov_add_block<KTYPE>(s, res, J);
}

// From the query's sums to its covariance.  Returns the status; cov [NF * NF] row-major and sigma0 are written only with kCovOk.
template <int KTYPE>
PTZ_HD int krt_cov_finish(const KrtCovSums<KTYPE>& s, double pixel_sigma, double* cov, double* sigma0)
{
  constexpr int NF = KrtDims<KTYPE>::NF, NH = KrtCovSums<KTYPE>::NH;
  const double m = 2.0 * s.v[NH + 1], cost = s.v[NH];
  if (!(m > (double)NF)) return kCovDof;
  if (!isfinite(cost)) return kCovSingular;
  // unit diagonal: A = S N S, S = diag(1 / sqrt(N_kk))
  double sc[NF], A[NF * NF];
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    const double d = s.v[k * (k + 1) / 2 + k];
    if (!(d > 0.0) || !isfinite(d)) return kCovSingular;
    sc[k] = 1.0 / sqrt(d);
  }
#pragma unroll
  for (int k = 0; k < NF; ++k)
#pragma unroll
    for (int l = 0; l <= k; ++l) A[k * NF + l] = s.v[k * (k + 1) / 2 + l] * sc[k] * sc[l];
  // Cholesky in place (lower), column by column as spd_solve does; inv[j] = 1 / L_jj
  double inv[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    double d = A[j * NF + j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= A[j * NF + k] * A[j * NF + k];
    if (!(d > kCovMinPivot)) return kCovSingular;
    const double l = sqrt(d);
    inv[j] = 1.0 / l;
    A[j * NF + j] = l;
#pragma unroll
    for (int i = j + 1; i < NF; ++i) {
      double v = A[i * NF + j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= A[i * NF + k] * A[j * NF + k];
      A[i * NF + j] = v * inv[j];
    }
  }
  // W = L^-1 (lower), column by column
  double W[NF * NF];
#pragma unroll
  for (int c = 0; c < NF; ++c) {
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      if (i < c) { W[i * NF + c] = 0; continue; }
      double v = i == c ? 1.0 : 0.0;
#pragma unroll
      for (int k = c; k < i; ++k) v -= A[i * NF + k] * W[k * NF + c];
      W[i * NF + c] = v * inv[i];
    }
  }
  const double s2 = 2.0 * cost / (m - (double)NF);
  const double var = pixel_sigma > 0.0 ? pixel_sigma * pixel_sigma : s2;
  // N^-1 = S (W^T W) S
  double out[NF * NF];
  bool finite = isfinite(s2);
#pragma unroll
  for (int i = 0; i < NF; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double v = 0;
#pragma unroll
      for (int k = i; k < NF; ++k) v += W[k * NF + i] * W[k * NF + j];
      v = var * (v * sc[i] * sc[j]);
      finite = finite && isfinite(v);
      out[i * NF + j] = v; out[j * NF + i] = v;
    }
  if (!finite) return kCovSingular;
#pragma unroll
  for (int k = 0; k < NF * NF; ++k) cov[k] = out[k];
  *sigma0 = sqrt(s2);
  return kCovOk;
}

}  // namespace ptz
