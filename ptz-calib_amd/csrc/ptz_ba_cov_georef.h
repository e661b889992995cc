// ptz_ba_cov_georef.h -- covariance of GEOREFERENCED cameras and of the rig's projection centre: the definition and the algebra
// that ptz_ba_cov.h does not have (FP64).  PTZ_HD like that header: the georef kernels of ptz_ba_cov.hip instantiate these
// functions on the device, tests/cpu_harness/ba_cov_georef_harness.cc on the host.
//
// Definition (ptz_ba_batch_covariance_georef).
//  Scope: a ptz_ba_batch of type PTZRay or PTZRayDist whose problems carry 2D-3D annotations (the two types run_ptz_ba's
//  georeferencing uses), at the state ptz_ba_batch_get_state would return, T_l_w included.  A problem takes part if n_obs3d > 0.
//  Parameters of the linearisation: per camera the NC = 5 / 6 columns [fx, fy, (k1), r1, r2, r3] of ptz_ba_batch_cam_block_dim,
//  per problem the T_l_w block L = [rho1..3, t1..3], per ray its rank-2 block, eliminated exactly as in ptz_ba_cov.h (rays do
//  not enter 2D-3D residuals).  fy is read only by the 2D-3D functor: the fy column of a camera WITHOUT annotations is
//  identically zero ("dead"); like a gauge row it is identity in S and zero in the noise-weighted matrix.
//  Reduced system of order n = NC n_cam + 6: S = the 2D-2D part of ptz_ba_cov.h (its NF2 = 4 / 5 columns at positions
//  ba_geo_pos) plus, per annotation a of camera c (weight 1, A_a 2 x NC, G_a 2 x 6 from reproj2d3d_eval):
//    A_a^T A_a into (c, c),  A_a^T G_a into the border (c, L),  G_a^T G_a into (L, L).
//  Noise: two levels.  M = s_f^2 T_f + s_a^2 T_a with T_f the T of ptz_ba_cov.h and T_a the annotation terms of S; the full
//  covariance is C = S^-1 M S^-1.  s_f = pixel_sigma and s_a = annotation_sigma where positive; a zero is estimated from the
//  UNWEIGHTED residuals, s_f^2 = SSE_2d2d / (2 n_obs - p_f), p_f = NF2 n_cam - 3 + 2 n_ray (the rule of ptz_ba_cov.h), and
//  s_a^2 = SSE_2d3d / (2 n_obs3d - p_a), p_a = 6 + (number of annotated cameras); p_f + p_a is the parameter count.  Both
//  estimates are returned either way.  They are ESTIMATES: the split of the degrees of freedom between the two residual kinds is
//  a heuristic (the annotated cameras' other columns are fitted by both kinds), and s_a comes out a few per cent low.
//  Gauge: one camera's three rotation columns are anchored as in ptz_ba_cov.h.  What is returned is a WORLD-frame quantity and
//  does not depend on the anchor (beyond round-off): the anchor's rows are NOT zero.
//  Outputs per problem: cov, NF * NF per camera with NF = 4 / 5 and order [fx, d1, d2, d3, (k1)], d a LEFT perturbation of the
//  world rotation R_w = R_i R_lw about the camera's own axes: to first order d_w = d_i + R_i d_lw with d_i = Jl(r_i) dr_i and
//  d_lw = Jl(rho) drho, so the block is W Z W^T over Z = [C_cc C_cL; C_Lc C_LL] (ba_geo_world_block); fy is marginalised.
//  cov_centre [9]: covariance of the projection centre C_w = -R_lw^T t_lw, dC_w = -R_lw^T ([t_lw]_x d_lw + tau), in world units
//  (the extrinsic translation t_i is not part of the 2D-3D model and not part of this).  Both row-major, symmetric bit for bit.
//  Status: PTZ_COV_DOF if 2 n_obs <= p_f or 2 n_obs3d <= p_a (a problem without annotations lands here); PTZ_COV_SINGULAR for
//  the Cholesky's fail flag, a bad diagonal, a non-finite result, a 2D-2D observation in the penalty branch, or a 2D-3D point
//  with camera-frame z <= 0; with any status but PTZ_COV_OK the problem's outputs are untouched.
#pragma once

#include "ptz_ba_cov.h"

namespace ptz {

constexpr int kBaCovBehind = 16;  // (a flag beside kBaCovBadDiag ...) a 2D-3D point with camera-frame z <= 0

// entries per camera of the result, [fx, d1, d2, d3, (k1)]: 4 / 5 for PTZRay / PTZRayDist; -1 otherwise
PTZ_HD int ba_geo_cov_dim(int factor_type) { return factor_type == 0 ? 4 : factor_type == 1 ? 5 : -1; }
// position of 2D-2D column k of [fx, (k1), r1, r2, r3] among the NC columns [fx, fy, (k1), r1, r2, r3]
PTZ_HD constexpr int ba_geo_pos(int k) { return k == 0 ? 0 : k + 1; }
// doubles of one annotation's record: A_a (2 x NC, row-major), G_a (2 x 6), |e_a|^2
PTZ_HD constexpr int ba_geo_rec(int nc) { return 2 * nc + 13; }

PTZ_HD long long ba_geo_dof_a(long long n_obs3d, long long n_ann_cam) { return 2 * n_obs3d - (6 + n_ann_cam); }
// nf2: the 2D-2D columns per camera (4 / 5)
PTZ_HD int ba_geo_status(int nf2, long long n_cam, long long n_ray, long long n_obs, long long n_obs3d, long long n_ann_cam, int chol_fail,
                         int flags)
{
  if (ba_cov_dof(nf2, n_cam, n_ray, n_obs) <= 0 || ba_geo_dof_a(n_obs3d, n_ann_cam) <= 0) return kBaCovDof;
  if (chol_fail || flags) return kBaCovSingular;
  return kBaCovOk;
}
// the two variances of M = s_f^2 T_f + s_a^2 T_a and their estimates
PTZ_HD void ba_geo_noise(int nf2, long long n_cam, long long n_ray, long long n_obs, long long n_obs3d, long long n_ann_cam, double sse_f,
                         double sse_a, double pixel_sigma, double annotation_sigma, double est2[2], double var[2])
{
  est2[0] = sse_f / (double)ba_cov_dof(nf2, n_cam, n_ray, n_obs);
  est2[1] = sse_a / (double)ba_geo_dof_a(n_obs3d, n_ann_cam);
  var[0] = pixel_sigma > 0.0 ? pixel_sigma * pixel_sigma : est2[0];
  var[1] = annotation_sigma > 0.0 ? annotation_sigma * annotation_sigma : est2[1];
}

// what reproj2d3d_eval reads of T_l_w = [rho, t]: {R_lw (9), Jl(rho) (9), t (3)}
PTZ_HD void ba_geo_tlwblk(const double* t6, double* tb)
{
  double R[9], Jl[9];
  const double rv[3] = {t6[0], t6[1], t6[2]};
  rodrigues(rv, R);
  so3_left_jacobian(rv, Jl);
  for (int k = 0; k < 9; ++k) { tb[k] = R[k]; tb[9 + k] = Jl[k]; }
  tb[18] = t6[3]; tb[19] = t6[4]; tb[20] = t6[5];
}

// One annotation's record (ba_geo_rec doubles).  false: the point is not in front of the camera (z <= 0 or not a number).
template <int TYPE> PTZ_HD bool ba_geo_annot(const double* cb, const double* tb, const double xyz[3], float u, float v, double* rec)
{
  constexpr int NC = BaDims<TYPE>::NC + 1;
  double res[2], Jc[2][NC], Jt[2][6];
  reproj2d3d_eval<TYPE ? 1 : 0, true>(cb, tb, xyz, u, v, res, Jc, Jt);
  for (int k = 0; k < NC; ++k) { rec[k] = Jc[0][k]; rec[NC + k] = Jc[1][k]; }
  for (int m = 0; m < 6; ++m) { rec[2 * NC + m] = Jt[0][m]; rec[2 * NC + 6 + m] = Jt[1][m]; }
  rec[2 * NC + 12] = res[0] * res[0] + res[1] * res[1];
  const double* R = cb + CB_R;
  double Xl[3];
  for (int k = 0; k < 3; ++k) Xl[k] = tb[3 * k] * xyz[0] + tb[3 * k + 1] * xyz[1] + tb[3 * k + 2] * xyz[2] + tb[18 + k];
  const double z = R[6] * Xl[0] + R[7] * Xl[1] + R[8] * Xl[2];
  return z > 0.0;
}
// elements of the annotation's terms: A^T A (k, l), A^T G (k, m), G^T G (m, q)
PTZ_HD double ba_geo_cc(const double* rec, int nc, int k, int l) { return rec[k] * rec[l] + rec[nc + k] * rec[nc + l]; }
PTZ_HD double ba_geo_cl(const double* rec, int nc, int k, int m) { return rec[k] * rec[2 * nc + m] + rec[nc + k] * rec[2 * nc + 6 + m]; }
PTZ_HD double ba_geo_ll(const double* rec, int nc, int m, int q) { return rec[2 * nc + m] * rec[2 * nc + q] + rec[2 * nc + 6 + m] * rec[2 * nc + 6 + q]; }

// The world block of one camera is W Z W^T and the centre's covariance J C_LL J^T; both are formed element by element with
// ba_geo_quad, the lower triangle mirrored (symmetric bit for bit).
// Z: (NC + 6) x (NC + 6), row-major and symmetric, the covariance of [the camera's NC additive columns; rho; t], unscaled.
// W (NF x (NC + 6), row-major) maps them to [fx, d_w (3), (k1)]: d_w = Jl dr_i + R_i Jl(rho) drho.  Jl, R: the camera's left
// Jacobian and rotation; tb: ba_geo_tlwblk.
template <int TYPE> PTZ_HD void ba_geo_world_W(const double* Jl, const double* R, const double* tb, double* W)
{
  constexpr int NF = BaDims<TYPE>::NC, NC = NF + 1, NZ = NC + 6, R0 = NC - 3;
  double RJ[9];
  for (int k = 0; k < NF * NZ; ++k) W[k] = 0.0;
  mat3_mul(R, tb + 9, RJ);
  W[0] = 1.0;
  for (int a = 0; a < 3; ++a)
    for (int j = 0; j < 3; ++j) { W[(1 + a) * NZ + R0 + j] = Jl[3 * a + j]; W[(1 + a) * NZ + NC + j] = RJ[3 * a + j]; }
  if (TYPE == 1) W[4 * NZ + 2] = 1.0;
}
// The projection centre C_w = -R_lw^T t and its Jacobian J (3 x 6, row-major) with respect to [rho; t]:
// dC_w = -R_lw^T ([t]_x d_lw + tau), d_lw = Jl(rho) drho.
PTZ_HD void ba_geo_centre_J(const double* tb, double* centre, double* J)
{
  const double* R = tb; const double* t = tb + 18;
  const double tx[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
  double TJ[9];
  mat3_mul(tx, tb + 9, TJ);
  for (int i = 0; i < 3; ++i) {
    centre[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
    for (int j = 0; j < 3; ++j) {
      J[6 * i + j] = -(R[i] * TJ[j] + R[3 + i] * TJ[3 + j] + R[6 + i] * TJ[6 + j]);
      J[6 * i + 3 + j] = -R[3 * j + i];
    }
  }
}
// a^T Z b over an nz x nz block of a row-major matrix of row stride ld, rows outermost
PTZ_HD double ba_geo_quad(const double* a, const double* b, const double* Z, int nz, int ld)
{
  double v = 0;
  for (int p = 0; p < nz; ++p) {
    double h = 0;
    for (int q = 0; q < nz; ++q) h += Z[p * ld + q] * b[q];
    v += a[p] * h;
  }
  return v;
}

#if defined(__HIPCC__)
// what the georef computation is given beyond BaCovIn (ptz_ba.hip fills it from the batch's resident structure)
struct BaGeoIn {
  const float2* o3_uv;  // [total annotations]: problem k's are BaCovScene::n_o3 entries at o3_off
  const double* o3_xyz;
  const int* o3_cam;    // scene-local camera
  const double* tlw_x;  // T_l_w of problem k at tlw_x + cur * tlw_stride + 6 idx
  size_t tlw_stride;
};
// As ba_cov_run.  cov / cov_centre / sigma0 / status: host outputs as ptz_ba_batch_covariance_georef.
int ba_geo_cov_run(const BaCovIn& in, const BaGeoIn& geo, const BaCovScene* hs, const int* gauge, double pixel_sigma,
                   double annotation_sigma, hipStream_t st, double* cov, double* cov_centre, double* sigma0, int* status, double* device_ms);
#endif

}  // namespace ptz
