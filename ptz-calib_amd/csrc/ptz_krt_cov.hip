// ptz_krt_cov.hip -- per-query covariance of relocalized cameras, batched over queries (gfx950).
//
// What a caller of ptz_krt_solve_batch gets back is a camera, a summary and a 0/1 `accepted`; this adds the parameter
// covariance a calibration tool reports beside it (cv::calibrateCamera's stdDeviations, ceres::Covariance): one more
// linearisation at the refined camera, an NF x NF inverse, a scale.  The algebra is ptz_krt_cov.h (shared with the host harness).
//
// k_krt_cov: SIXTEEN lanes (one DPP row) per query, four queries per wave, whatever the launch size.  The lanes stride over the
// query's 16-byte match records (a row reads 128 contiguous bytes of each pixel array per step) and then over its 2D-3D points,
// each lane summing its blocks in ascending order into NF (NF + 1) / 2 + 2 registers; the sums are reduced by the fixed butterfly
// group_sum<16> (lane l adds l ^ 8, l ^ 4, l ^ 2, l ^ 1); lane 0 of the row inverts and writes.  That is the ONE reduction order: a
// query's bits depend on its own data only -- not on its neighbours, not on the number of queries in the launch.  A single pass over
// the matches: no LDS ray cache, no trust-region state, so the kernel sits far below k_krt's 247-256 VGPRs.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ptz_common.h"
#include "ptz_pool.h"
#include "ptz_krt_device.h"
#include "ptz_krt_cov.h"

namespace ptz {
namespace {

static_assert(kCovOk == PTZ_COV_OK && kCovDof == PTZ_COV_DOF && kCovSingular == PTZ_COV_SINGULAR && kCovSkipped == PTZ_COV_SKIPPED,
              "ptz_krt_cov.h and ptz_calib_amd.h name the same codes");

constexpr int COV_G = 16, COV_QPB = 256 / COV_G;  // lanes per query, queries per workgroup

// Waves per SIMD the register budget is held to (512 VGPRs per lane of a SIMD), from the compiler's counts: F and
// Fxfy need 108 / 122 registers and run four waves; FDist (166) and F with 2D-3D points (168) run three; FxfyDist (186) and the other
// 2D-3D variants (188 - 238: undistortion, two Brown models, 23 sums) run two.  No instantiation spills.
template <int KTYPE, bool P3> struct KrtCovOcc {
  static constexpr int WAVES = (KTYPE & 1) ? ((P3 || (KTYPE & 2)) ? 2 : 3) : (P3 ? ((KTYPE & 2) ? 2 : 3) : 4);
};
template <int KTYPE, bool P3>
__global__ __launch_bounds__(256, (KrtCovOcc<KTYPE, P3>::WAVES)) void k_krt_cov(int n_query, const long long* __restrict__ match_ptr, const float2* __restrict__ uv_ref,
                                                    const float2* __restrict__ uv_cur, const long long* __restrict__ point_ptr,
                                                    const float2* __restrict__ pt_uv, const double* __restrict__ pt_xyz,
                                                    const double* __restrict__ cam_ref, const double* __restrict__ cam_cur,
                                                    const unsigned char* __restrict__ match_mask, const int* __restrict__ accepted,
                                                    double pixel_sigma, double* __restrict__ cov, double* __restrict__ sigma0,
                                                    int* __restrict__ status)
{
  constexpr int NF = KrtDims<KTYPE>::NF;
  const int q = blockIdx.x * COV_QPB + (int)threadIdx.x / COV_G;
  if (q >= n_query) return;  // (whole rows leave: the DPP moves below stay inside a row)
  const int lane = threadIdx.x % COV_G;
  if (accepted && accepted[q] == 0) {  // the solve never wrote this query's camera
    if (lane == 0) status[q] = kCovSkipped;
    return;
  }
  const long long m0 = match_ptr[q];
  const int M = (int)(match_ptr[q + 1] - m0);
  const long long p0 = P3 ? point_ptr[q] : 0;
  const int NP = P3 ? (int)(point_ptr[q + 1] - p0) : 0;
  double ref[15], cur[15], x[15], Rref[9], R[9];
#pragma unroll
  for (int k = 0; k < 15; ++k) { ref[k] = cam_ref[(size_t)q * 15 + k]; cur[k] = cam_cur[(size_t)q * 15 + k]; }
  krt_cov_local_frame(ref, cur, x, Rref, R);
  const double kref[4] = {ref[0], ref[1], ref[2], ref[3]};
  const double dref[5] = {ref[10], ref[11], ref[12], ref[13], ref[14]};
  KrtCovSums<KTYPE> s;
  krt_cov_clear<KTYPE>(s);
  for (int m = lane; m < M; m += COV_G) {
    if (match_mask && match_mask[m0 + m] == 0) continue;
    const float2 a = uv_ref[m0 + m], b = uv_cur[m0 + m];
    double r1[3];
    bool skip;
    MatchEval<KTYPE>::ray1(kref, dref, a.x, a.y, r1, skip);
    krt_cov_add_match<KTYPE>(s, R, x, r1, skip, b.x, b.y);
  }
  if (P3) {
    for (int i = lane; i < NP; i += COV_G) {
      const float2 b = pt_uv[p0 + i];
      const double* X = pt_xyz + 3 * (p0 + i);
      double Xl[3];  // R_local_world X_w + t_local_world (krt_optimizer.cc:357-362)
      Xl[0] = Rref[0] * X[0] + Rref[1] * X[1] + Rref[2] * X[2] + ref[7];
      Xl[1] = Rref[3] * X[0] + Rref[4] * X[1] + Rref[5] * X[2] + ref[8];
      Xl[2] = Rref[6] * X[0] + Rref[7] * X[1] + Rref[8] * X[2] + ref[9];
      krt_cov_add_point<KTYPE>(s, R, x, Xl, b.x, b.y);
    }
  }
#pragma unroll
  for (int k = 0; k < KrtCovSums<KTYPE>::COUNT; ++k) s.v[k] = group_sum<COV_G>(s.v[k]);
  if (lane == 0) {
    double c[NF * NF], s0;
    const int st = krt_cov_finish<KTYPE>(s, pixel_sigma, c, &s0);
    status[q] = st;
    if (st == kCovOk) {
      double* out = cov + (size_t)q * (NF * NF);
#pragma unroll
      for (int k = 0; k < NF * NF; ++k) out[k] = c[k];
      sigma0[q] = s0;
    }
  }
}

// one launch over a device-resident batch
void launch_krt_cov(const KrtBatch& in, int factor_type, const unsigned char* d_mask, const int* d_acc, double pixel_sigma, double* d_cov,
                    double* d_s0, int* d_status, hipStream_t st)
{
  const dim3 grid((in.n_query + COV_QPB - 1) / COV_QPB), block(256);
#define PTZ_COV_LAUNCH(T, P)                                                                                                          \
  hipLaunchKernelGGL((k_krt_cov<T, P>), grid, block, 0, st, in.n_query, in.match_ptr, in.uv_ref, in.uv_cur, in.point_ptr, in.pt_uv,     \
                     in.pt_xyz, in.cam_ref, in.cam_cur, d_mask, d_acc, pixel_sigma, d_cov, d_s0, d_status)
  switch (factor_type * 2 + (in.point_ptr ? 1 : 0)) {
    case 0: PTZ_COV_LAUNCH(0, false); break;
    case 1: PTZ_COV_LAUNCH(0, true); break;
    case 2: PTZ_COV_LAUNCH(1, false); break;
    case 3: PTZ_COV_LAUNCH(1, true); break;
    case 4: PTZ_COV_LAUNCH(2, false); break;
    case 5: PTZ_COV_LAUNCH(2, true); break;
    case 6: PTZ_COV_LAUNCH(3, false); break;
    default: PTZ_COV_LAUNCH(3, true); break;
  }
#undef PTZ_COV_LAUNCH
}

inline int free_dim(int factor_type)
{
  switch (factor_type) {
    case PTZ_KRT_F: return KrtDims<0>::NF;
    case PTZ_KRT_FDist: return KrtDims<1>::NF;
    case PTZ_KRT_Fxfy: return KrtDims<2>::NF;
    case PTZ_KRT_FxfyDist: return KrtDims<3>::NF;
    default: return PTZ_EUNSUPPORTED;
  }
}

}  // namespace
}  // namespace ptz

using namespace ptz;

extern "C" int32_t ptz_krt_free_dim(int32_t factor_type) { return free_dim(factor_type); }

extern "C" int32_t ptz_krt_covariance_batch_device(int32_t n_query, const int64_t* d_match_ptr, const float* d_uv_ref, const float* d_uv_cur,
                                                   const int64_t* d_point_ptr, const float* d_pts2d, const double* d_pts3d,
                                                   const double* d_cam_ref, const double* d_cam_cur, int32_t factor_type,
                                                   const uint8_t* d_match_mask, const int32_t* d_accepted, double pixel_sigma,
                                                   double* d_cov, double* d_sigma0, int32_t* d_status, void* hip_stream)
{
  if (n_query < 0 || !(pixel_sigma >= 0.0) || !std::isfinite(pixel_sigma)) return PTZ_EINVAL;
  if (d_point_ptr && (!d_pts2d || !d_pts3d)) return PTZ_EINVAL;
  if (free_dim(factor_type) < 0) return PTZ_EUNSUPPORTED;
  if (n_query == 0) return PTZ_OK;
  if (!d_match_ptr || !d_uv_ref || !d_uv_cur || !d_cam_ref || !d_cam_cur || !d_cov || !d_sigma0 || !d_status) return PTZ_EINVAL;
  clear_stale_error(__func__);
  int device = -1;
  if (const int rc = owning_device(d_cam_cur, hip_stream, &device)) return rc;
  PTZ_DEVICE_GUARD(device);
  launch_krt_cov(krt_batch_of(n_query, d_match_ptr, d_uv_ref, d_uv_cur, d_point_ptr, d_pts2d, d_pts3d, d_cam_ref, d_cam_cur), factor_type,
                 d_match_mask, d_accepted, pixel_sigma, d_cov, d_sigma0, d_status, (hipStream_t)hip_stream);
  PTZ_HIP_TRY(hipGetLastError());
  return PTZ_OK;
}

extern "C" int32_t ptz_krt_covariance_batch(int32_t n_query, const int64_t* match_ptr, const float* uv_ref, const float* uv_cur,
                                            const int64_t* point_ptr, const float* pts2d, const double* pts3d, const double* cam_ref,
                                            const double* cam_cur, int32_t factor_type, const uint8_t* match_mask, const int32_t* accepted,
                                            double pixel_sigma, int32_t device_id, double* cov, double* sigma0, int32_t* status,
                                            double* device_ms)
{
  if (n_query < 0 || !(pixel_sigma >= 0.0) || !std::isfinite(pixel_sigma)) return PTZ_EINVAL;
  if (point_ptr && (!pts2d || !pts3d)) return PTZ_EINVAL;
  const int nf = free_dim(factor_type);
  if (nf < 0) return PTZ_EUNSUPPORTED;
  if (n_query == 0) return PTZ_OK;
  if (!cov || !sigma0 || !status || device_id < 0) return PTZ_EINVAL;
  const KrtHostBatch hb = {n_query, match_ptr, uv_ref, uv_cur, point_ptr, pts2d, pts3d, cam_ref, cam_cur};
  if (const int rc = check_host_batch(hb, kKrtCheckAll)) return rc;
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);
  // one pooled device block: [inputs | cov | sigma0 | status]
  const size_t nn = (size_t)nf * nf;
  BlockLayout lay;
  const KrtBatchSlots slots = krt_batch_reserve(lay, n_query, hb.n_match(), hb.n_point(), match_mask != nullptr, accepted != nullptr);
  const size_t o_cov = lay.take(sizeof(double) * nn * n_query), o_s0 = lay.take(sizeof(double) * n_query), o_st = lay.take(sizeof(int) * n_query);
  CallHeld h;
  if (const int rc = h.acquire(device_id, lay.total())) return rc;
  KrtBatch in;
  PTZ_HIP_TRY(krt_batch_upload(hb, match_mask, accepted, slots, h, false, &in));
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  launch_krt_cov(in, factor_type, match_mask ? (const unsigned char*)(h.base + slots.mask) : nullptr,
                 accepted ? (const int*)(h.base + slots.accepted) : nullptr, pixel_sigma, (double*)(h.base + o_cov), (double*)(h.base + o_s0),
                 (int*)(h.base + o_st), h.st);
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  // cov and sigma0 of a query whose status is not PTZ_COV_OK stay as the caller had them: the device's copies come back into a
  // buffer of their own and only the rows of computed queries are copied out
  std::vector<double> hc(nn * n_query), hs(n_query);
  PTZ_HIP_TRY(hipMemcpyAsync(hc.data(), h.base + o_cov, sizeof(double) * nn * n_query, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(hs.data(), h.base + o_s0, sizeof(double) * n_query, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(status, h.base + o_st, sizeof(int) * n_query, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  PTZ_HIP_TRY(hipGetLastError());  // a refused kernel launch must not pass for a result
  for (int q = 0; q < n_query; ++q) {
    if (status[q] != PTZ_COV_OK) continue;
    memcpy(cov + nn * q, hc.data() + nn * q, sizeof(double) * nn);
    sigma0[q] = hs[q];
  }
  if (device_ms) *device_ms = h.elapsed_ms();
  return PTZ_OK;
}
