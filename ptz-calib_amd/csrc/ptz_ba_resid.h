// ptz_ba_resid.h -- residual report of a bundle-adjustment batch and the trimming selection on it (ptz_ba_batch_residuals,
// ptz_ba_batch_trim_select): what ptz_ba_resid.hip is given and what it hands back.
//
// The report is taken at the state ptz_ba_batch_get_state would return; ptz_ba.hip fills the BaCovIn / BaGeoIn the covariance
// kernels are fed with (ptz_ba_cov.h) and adds the ray order.  Kernels, on the batch's stream:
//   cam      camera blocks (R, intrinsics) at the state; the T_l_w block of an annotated problem                [thread / camera]
//   order    where the observations of the CALLER's ray r begin in the caller's order: the library stores observations
//            ray-major with the rays renumbered longest first (ray_perm), the caller ray-major in its own numbering  [workgroup / problem]
//   ray      |e_o| of the ray's observations (ba_residual, the functors of ptz_factor.h), written in the library's order for
//            the passes below and through the map in the caller's; the ray's largest and where (first on a tie)    [thread / ray]
//   view     sum of squares, maximum and count over the camera's observation list in stored order: lane l takes entries
//            l, l + 64, .., the lanes meet in the butterfly                                                        [wave / camera]
//   annot    |e_a| of the 2D-3D annotations (reproj2d3d_eval)                                                      [thread / annotation]
//   problem  rms (thread t sums observations t, t + 1024, .. in the library's order, block_sum), rms3d, the exact lower median
//            by bitwise selection (a 256-bin count per byte of the bit patterns of the non-negative doubles, from the top; the
//            leading bytes all elements share are not counted), the threshold of the rule (ptz_ba_trim.h) and the rejects
//                                                                                                                  [workgroup / problem]
// No floating-point atomics; every sum has one shape that depends on the problem alone.
#pragma once

#include <stdint.h>

#include "ptz_ba_cov.h"
#include "ptz_ba_cov_georef.h"
#include "ptz_ba_trim.h"

namespace ptz {

#if defined(__HIPCC__)
// host outputs, each concatenated over the problems at their real extents; any may be NULL
struct BaResidOut {
  double* err_px = nullptr;      // [sum n_obs] caller's observation order
  double* ray_max = nullptr;     // [sum n_ray] caller's ray numbering
  int32_t* ray_worst = nullptr;  // [sum n_ray] problem-local observation index
  double* view_rms = nullptr;    // [sum n_cam]
  double* view_max = nullptr;
  int32_t* view_count = nullptr;
  double* rms = nullptr;         // [n]
  double* median = nullptr;      // [n]
  double* err3d_px = nullptr;    // [sum n_obs3d]
  double* rms3d = nullptr;       // [n]
  // the selection (select = true): rule, and reject [sum n_obs] / threshold [n] / n_reject [n]
  bool select = false;
  TrimRule rule{0, 0, 2};
  uint8_t* reject = nullptr;
  double* threshold = nullptr;
  int32_t* n_reject = nullptr;
};
// ray_perm: device, scene-local caller index of internal ray j at ray_off + j.  geo.tlw_x == nullptr: no annotations anywhere.
int ba_resid_run(const BaCovIn& in, const BaGeoIn& geo, const BaCovScene* hs, const int* ray_perm, hipStream_t st, const BaResidOut& out,
                 double* device_ms);
#endif

}  // namespace ptz
