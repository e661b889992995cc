// ptz_ba_cov.h -- per-view covariance of bundle-adjusted cameras: the definition and the per-ray / per-camera algebra (FP64).
//
// PTZ_HD like ptz_factor.h and ptz_krt_cov.h: the kernels of ptz_ba_cov.hip instantiate these functions on the device,
// tests/cpu_harness/ba_cov_harness.cc (with ba_cov_common.h, which it shares with ba_cov_georef_harness.cc) instantiates them on the
// host and finishes the computation in plain loops.
//
// Definition (ptz_ba_batch_covariance).
//  Scope: a ptz_ba_batch of 2D-2D problems of type PTZRay, PTZRayDist or PTZRayFxfyDist (ptz_ba_batch_create or
//  ptz_ba_batch_create_views), evaluated at exactly the state ptz_ba_batch_get_state would return at the moment of the call:
//  after a solve the minimum-cost point, before any solve the state last set.
//  Parameters: per camera p = [fx, (fy), d1, d2, d3, (k1)], NF = 4 / 5 / 6 of them, order and meaning those of
//  ptz_krt_covariance_batch: d is a LEFT perturbation R <- Exp(d) R in radians about the camera's own x, y, z axes.  The
//  bundle-adjustment Jacobians (ba_linearize) are with respect to the additive Rodrigues vector r in the column order
//  [fx, (fy), (k1), r1, r2, r3]; R(r + dr) = Exp(Jl dr) R(r), so the camera's block is converted at the end, C_d = A C_r A^T
//  with A = diag(I, Jl) (ba_cov_to_left), and permuted into the output order.
//  Per ray r over its candidate observations o, closed-form Jacobians, no Jacobi scaling: A_o (2 x NF), B_o (2 x 3),
//    V_r = w_r sum B_o^T B_o,  E_o = w_r A_o^T B_o,  P_r = (V_r + 1/2 tr(V_r) x^ x^T)^-1,  Y_o = E_o P_r.
//  Every 2D-2D functor is invariant to the scale of the ray, so B_o x = 0: V_r has rank 2 with null vector x^ = x / |x|, and
//  because E_o x^ = 0 the product E_o P_r E_o'^T equals E_o V_r^+ E_o'^T exactly, for any positive multiple of x^ x^T.
//  Reduced matrices over the cameras:
//    S[c_o, c_o'] = sum_r ( [o = o'] w_r A_o^T A_o - E_o P_r E_o'^T ),   T = the same sum, every term times w_r once more.
//  A ray with a single candidate observation contributes exactly zero to both (it is skipped, not computed).
//  The track weights w_r (ScaledLoss, full track length) are not inverse variances: under iid pixel noise of variance s^2 the
//  estimator's covariance is the sandwich s^2 H^-1 (J^T W^2 J) H^-1, H = J^T W J, whose camera part is s^2 S^-1 T S^-1.
//  Gauge: rotation-only bundle adjustment leaves the global rotation free; the rotation of camera gauge_cam[k] of problem k
//  (NULL: camera 0) is the anchor -- its three rotation rows and columns are identity in S and zero in T, and zero in the
//  result, which describes every view's rotation relative to the anchor; the anchor's fx / fy / k1 entries are ordinary.
//  Solve: S is scaled to unit diagonal and factored by the batch Cholesky; C = s^2 S^-1 T S^-1, of which the per-camera
//  diagonal blocks are returned, NF * NF per camera, row-major, symmetric bit for bit.  s = pixel_sigma if pixel_sigma > 0,
//  else s = sigma0 with sigma0^2 = sum_o |e_o|^2 / (m - p): UNWEIGHTED residuals, m = 2 n_obs, p = NF n_cam - 3 + 2 n_ray.
//  sigma0 is an ESTIMATE of the pixel noise (exact in expectation for equal weights, within a per cent for track weights
//  2..6); it is returned either way.
//  Status per problem: PTZ_COV_DOF if m <= p; PTZ_COV_SINGULAR for the Cholesky's fail flag, a diagonal entry of S that is
//  not positive and finite, a non-finite result, or an observation in the behind-the-camera penalty branch of PTZRayDist
//  (no linearisation there); with any status but PTZ_COV_OK the problem's cov and sigma0 are left untouched.
#pragma once

#include "ptz_factor.h"

namespace ptz {

constexpr int kBaCovOk = 0, kBaCovDof = 1, kBaCovSingular = 2;  // PTZ_COV_OK / _DOF / _SINGULAR
// what a problem's kernels raise (bits): a diagonal entry of S not positive and finite, a non-finite result, an observation in
// the penalty branch, a ray whose regularised block is not positive definite
constexpr int kBaCovBadDiag = 1, kBaCovNonFinite = 2, kBaCovPenalty = 4, kBaCovBadRay = 8;

// free parameters per camera: 4, 5, 6 for PTZRay, PTZRayDist, PTZRayFxfyDist; -1 otherwise
PTZ_HD int ba_cov_dim(int factor_type) { return factor_type == 0 ? 4 : factor_type == 1 ? 5 : factor_type == 2 ? 6 : -1; }

// DOF rule: m = 2 n_obs residuals against p = NF n_cam - 3 + 2 n_ray parameters (gauge removed, two tangents per ray)
PTZ_HD long long ba_cov_dof(int nf, long long n_cam, long long n_ray, long long n_obs) { return 2 * n_obs - (nf * n_cam - 3 + 2 * n_ray); }
PTZ_HD int ba_cov_status(int nf, long long n_cam, long long n_ray, long long n_obs, int chol_fail, int flags)
{
  if (ba_cov_dof(nf, n_cam, n_ray, n_obs) <= 0) return kBaCovDof;
  if (chol_fail || flags) return kBaCovSingular;
  return kBaCovOk;
}

// output slot k of p = [fx, (fy), d1, d2, d3, (k1)] -> column of ba_linearize's order [fx, (fy), (k1), r1, r2, r3]
template <int TYPE> PTZ_HD constexpr int ba_cov_col(int k)
{
  return TYPE == 0 ? k : TYPE == 1 ? (k == 0 ? 0 : k == 4 ? 1 : k + 1) : (k < 2 ? k : k == 5 ? 2 : k + 1);
}

// the camera block ba_linearize reads (R, intrinsics, Jl; no Jacobi scales), from the 15-vector
PTZ_HD void ba_cov_camblk(const double* c15, double* cb)
{
  double R[9], Jl[9];
  rodrigues(c15 + 4, R);
  so3_left_jacobian(c15 + 4, Jl);
  for (int i = 0; i < 9; ++i) { cb[CB_R + i] = R[i]; cb[CB_JL + i] = Jl[i]; }
  cb[CB_F] = c15[0]; cb[CB_CX] = c15[2]; cb[CB_CY] = c15[3]; cb[CB_FY] = c15[1];
  for (int i = 0; i < 5; ++i) cb[CB_K + i] = c15[10 + i];
  for (int i = CB_S; i < CAMBLK; ++i) cb[i] = 1.0;
}

// V (packed lower: v00 v10 v11 v20 v21 v22) += B^T B of one observation
PTZ_HD void ba_cov_add_V(const double Jr[2][3], double V[6])
{
  V[0] += Jr[0][0] * Jr[0][0] + Jr[1][0] * Jr[1][0];
  V[1] += Jr[0][1] * Jr[0][0] + Jr[1][1] * Jr[1][0];
  V[2] += Jr[0][1] * Jr[0][1] + Jr[1][1] * Jr[1][1];
  V[3] += Jr[0][2] * Jr[0][0] + Jr[1][2] * Jr[1][0];
  V[4] += Jr[0][2] * Jr[0][1] + Jr[1][2] * Jr[1][1];
  V[5] += Jr[0][2] * Jr[0][2] + Jr[1][2] * Jr[1][2];
}

// P_r = (w V + 1/2 tr(w V) x^ x^T)^-1, packed like V; V = sum B^T B (unweighted), x = the ray parameter.  false: not positive
// definite or not finite (a ray nothing constrains).
PTZ_HD bool ba_cov_ray_P(const double V[6], double w, const double x[3], double P[6])
{
  const double n2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  const double c = 0.5 * w * (V[0] + V[2] + V[5]) / n2;
  double M[6];
  M[0] = w * V[0] + c * x[0] * x[0];
  M[1] = w * V[1] + c * x[1] * x[0];
  M[2] = w * V[2] + c * x[1] * x[1];
  M[3] = w * V[3] + c * x[2] * x[0];
  M[4] = w * V[4] + c * x[2] * x[1];
  M[5] = w * V[5] + c * x[2] * x[2];
  bool fin = true;
  for (int k = 0; k < 6; ++k) fin = fin && isfinite(M[k]);
  if (!fin) return false;
  if (!inv3_spd(M, P)) return false;
  for (int k = 0; k < 6; ++k) fin = fin && isfinite(P[k]);
  return fin;
}

// E_o = w A^T B (NF x 3, row-major)
template <int NF> PTZ_HD void ba_cov_E(const double Jc[2][NF], const double Jr[2][3], double w, double* E)
{
  for (int k = 0; k < NF; ++k)
    for (int m = 0; m < 3; ++m) E[3 * k + m] = w * (Jc[0][k] * Jr[0][m] + Jc[1][k] * Jr[1][m]);
}
// Y_o = E_o P_r
template <int NF> PTZ_HD void ba_cov_Y(const double* E, const double P[6], double* Y)
{
  for (int k = 0; k < NF; ++k) {
    const double e0 = E[3 * k], e1 = E[3 * k + 1], e2 = E[3 * k + 2];
    Y[3 * k] = e0 * P[0] + e1 * P[1] + e2 * P[3];
    Y[3 * k + 1] = e0 * P[1] + e1 * P[2] + e2 * P[4];
    Y[3 * k + 2] = e0 * P[3] + e1 * P[4] + e2 * P[5];
  }
}
// element (k, l) of the observation's term of its camera's diagonal block: w A^T A - Y_o E_o^T
template <int NF> PTZ_HD double ba_cov_diag_term(const double Jc[2][NF], double w, const double* Y, const double* E, int k, int l)
{
  return w * (Jc[0][k] * Jc[0][l] + Jc[1][k] * Jc[1][l]) - (Y[3 * k] * E[3 * l] + Y[3 * k + 1] * E[3 * l + 1] + Y[3 * k + 2] * E[3 * l + 2]);
}
// element (k, l) of the term of a pair of observations (o, o') of one ray in block (c_o, c_o'): -Y_o E_o'^T
PTZ_HD double ba_cov_pair_term(const double* Ya, const double* Eb, int k, int l)
{
  return -(Ya[3 * k] * Eb[3 * l] + Ya[3 * k + 1] * Eb[3 * l + 1] + Ya[3 * k + 2] * Eb[3 * l + 2]);
}

// One camera's block from the Rodrigues columns to the left perturbation, into the output order, times var.
// Cr: NF x NF in ba_linearize's column order (only the lower triangle k >= l is read); Jl: row-major left Jacobian at the camera's
// rotation vector; anchor: the rotation rows and columns of the result are exactly zero.  out: row-major, symmetric bit for bit.
// Returns false if an entry is not finite.
template <int TYPE> PTZ_HD bool ba_cov_to_left(const double* Cr, const double* Jl, double var, bool anchor, double* out)
{
  constexpr int NF = BaDims<TYPE>::NC, R0 = BaDims<TYPE>::ROT0;
  double C[NF * NF], H[NF * NF];
  for (int k = 0; k < NF; ++k)
    for (int l = 0; l <= k; ++l) { C[k * NF + l] = Cr[k * NF + l]; C[l * NF + k] = Cr[k * NF + l]; }
  // H = A C: the rotation rows are mixed by Jl
  for (int k = 0; k < NF; ++k)
    for (int l = 0; l < NF; ++l) {
      if (k < R0) H[k * NF + l] = C[k * NF + l];
      else H[k * NF + l] = Jl[3 * (k - R0)] * C[R0 * NF + l] + Jl[3 * (k - R0) + 1] * C[(R0 + 1) * NF + l] + Jl[3 * (k - R0) + 2] * C[(R0 + 2) * NF + l];
    }
  // D = H A^T, lower triangle, mirrored
  bool fin = true;
  for (int ko = 0; ko < NF; ++ko)
    for (int lo = 0; lo <= ko; ++lo) {
      const int k = ba_cov_col<TYPE>(ko), l = ba_cov_col<TYPE>(lo);
      double v;
      if (l < R0) v = H[k * NF + l];
      else v = H[k * NF + R0] * Jl[3 * (l - R0)] + H[k * NF + R0 + 1] * Jl[3 * (l - R0) + 1] + H[k * NF + R0 + 2] * Jl[3 * (l - R0) + 2];
      v *= var;
      if (anchor && (k >= R0 || l >= R0)) v = 0.0;
      fin = fin && isfinite(v);
      out[ko * NF + lo] = v; out[lo * NF + ko] = v;
    }
  return fin;
}

#if defined(__HIPCC__)
// ---- what ptz_ba_cov.hip is given of a batch (ptz_ba.hip fills it from the batch's resident structure) --------------------------
struct BaCovScene {  // per problem, on the device: the real extents (a view batch finds them on the device) and the state's half
  int n_cam, n_ray, n_obs, n_pair;
  int cam_off, ray_off, obs_off, pair_off;
  int idx, cur;
  int o3_off, n_o3;  // 2D-3D annotations (read by the georeferenced covariance only, ptz_ba_cov_georef.h)
};
struct BaCovIn {
  int n_scene, type, device;
  const BaCovScene* scene;  // device [n_scene]
  const float2* obs_uv;     // observations in the batch's internal order (ray-major), global index
  const int* obs_cam;       // scene-local camera
  const int* ray_ptr;       // per scene n_ray + 1 entries at ray_off + idx: global observation index
  const int* cam_ptr;       // per scene n_cam + 1 entries at cam_off + idx: positions in cam_obs
  const int* cam_obs;       // global observation index, camera-major
  const int* pair_cj;       // at pair_off: the second camera of a pair (ci > cj)
  const int* pair_ptr;      // per scene n_pair + 1 entries at pair_off + idx: global entry index
  const int* cam_pair;      // per scene n_cam + 1 entries at cam_off + idx: scene-local pair range of camera ci
  const unsigned* ent;      // low 16 bits: position of observation a in ci's list, high 16: of b in cj's
  const double* ray_w;      // [total_ray]
  const double* cam_x;      // state: camera c of the batch at cam_x + cur * cam_stride + 15 c, ray j at ray_x + cur * ray_stride + 3 j
  const double* ray_x;
  size_t cam_stride, ray_stride;
};
// Enqueues the whole computation on `st`, group by group under the workspace budget (PTZ_BA_COV_MAX_MB), and waits.  hs: host copy
// of the scenes; gauge: host [n_scene] anchors (already validated).  cov / sigma0 / status: host outputs as ptz_ba_batch_covariance.
int ba_cov_run(const BaCovIn& in, const BaCovScene* hs, const int* gauge, double pixel_sigma, hipStream_t st, double* cov, double* sigma0,
               int* status, double* device_ms);
#endif

}  // namespace ptz
