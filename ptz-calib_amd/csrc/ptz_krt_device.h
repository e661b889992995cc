// ptz_krt_device.h -- device helpers shared by the single-view kernels: k_krt (ptz_krt.hip), k_krt_cov (ptz_krt_cov.hip) and the
// residual report / trimming step (ptz_krt_resid.hip); and, host side, the one description of a relocalization batch those files
// share: its checks, its upload and the launch of k_krt.
#pragma once

#include "ptz_common.h"
#include "ptz_factor.h"
#include "ptz_host_batch.h"
#include "ptz_krt_batch_layout.h"

namespace ptz {

// 15-vector index of free parameter k: F {0,4,5,6}, FDist {0,4,5,6,10}, Fxfy {0,1,4,5,6}, FxfyDist {0,1,4,5,6,10}
template <int KTYPE> struct KFree {
  static __device__ __forceinline__ int at(int k)
  {
    constexpr int ROT0 = KrtDims<KTYPE>::ROT0;
    return k < ROT0 ? k : (k < ROT0 + 3 ? 4 + (k - ROT0) : 10);
  }
};

// in-register Cholesky solve of an NF x NF SPD system (row-major full storage); false if not SPD
template <int NF>
__device__ __forceinline__ bool spd_solve(double* A, double* b)
{
  double inv[NF];  // 1 / L_jj
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    double d = A[j * NF + j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= A[j * NF + k] * A[j * NF + k];
    if (!(d > 0.0)) return false;
    // (round 6) ONE reciprocal per column -- 1 / sqrt(d) to working precision (rsq + two Newton steps) -- instead of a square root and
    // 2 (NF - 1 - j) + 2 IEEE divisions by it: a division is ~18 instructions on this chip and the solve had twenty of them, every
    // lane of the group its own copy.  The factor and the solution differ from the divided form in the last bits (the step is held
    // to the oracle's QR step at 1e-6 either way).
    double rs = __builtin_amdgcn_rsq(d);
    rs = rs * (1.5 - 0.5 * d * rs * rs);
    rs = rs * (1.5 - 0.5 * d * rs * rs);
    inv[j] = rs;
    A[j * NF + j] = d * rs;
#pragma unroll
    for (int i = j + 1; i < NF; ++i) {
      double v = A[i * NF + j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= A[i * NF + k] * A[j * NF + k];
      A[i * NF + j] = v * rs;
    }
  }
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    double v = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= A[i * NF + k] * b[k];
    b[i] = v * inv[i];
  }
#pragma unroll
  for (int i = NF - 1; i >= 0; --i) {
    double v = b[i];
#pragma unroll
    for (int k = i + 1; k < NF; ++k) v -= A[k * NF + i] * b[k];
    b[i] = v * inv[i];
  }
  return true;
}

template <int KTYPE>
struct MatchEval {
  // constant part of a match: unit ray of the reference pixel in the local frame (krt_optimizer.cc:31-33,
  // 89-104) and the border guard of the distortion variant (:97-101)
  static __device__ __forceinline__ void ray1(const double* kref, const double* dref, float u1, float v1, double r[3], bool& skip)
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
};

// Lanes per query.  G = 64 (a wave per query) is the latency form: a registration attempt of the incremental pipeline or a
// handful of queries are as fast as they can be.  G = 16 (four queries per wave) is the throughput form for launches of
// thousands of queries of a few hundred matches each: with 128 matches a wave of 64 has two matches per lane and then spends
// as long on its 15 six-step reductions and on 64 redundant copies of one 4 x 4 solve as on the matches; 16 lanes take eight
// matches each, reduce in four steps, and a wave's redundant solves serve four queries.  The two forms sum in different
// orders: a query's bits depend on the form, never on its neighbours in the launch (ptz_krt_solve_batch picks the form from
// the launch size alone, krt_group_size()).
// (the butterfly v += v[lane ^ off], off = G / 2 .. 1, with the partners fetched by v_permlane32/16_swap and DPP instead of
//  ds_bpermute -- 21 sums of four to six steps per linearisation: the same partners, the same sums, the same bits)
template <int G> __device__ __forceinline__ double group_sum(double v)
{
  static_assert(G == 64 || G == 16, "a wave or a DPP row of lanes per query");
  if (G == 64) return wave_sum(v);
  v += lane_xor_dpp<8>(v);
  v += lane_xor_dpp<4>(v);
  v += lane_xor_dpp<2>(v);
  v += lane_xor_dpp<1>(v);
  return v;
}
template <int G> __device__ __forceinline__ double group_max(double v)  // (the same butterfly)
{
  static_assert(G == 64 || G == 16, "a wave or a DPP row of lanes per query");
  if (G == 64) return wave_max(v);
  v = fmax(v, lane_xor_dpp<8>(v));
  v = fmax(v, lane_xor_dpp<4>(v));
  v = fmax(v, lane_xor_dpp<2>(v));
  v = fmax(v, lane_xor_dpp<1>(v));
  return v;
}

// ---- one description of a relocalization batch ---------------------------------------------------------------------------------
// The device-resident batch: what the kernels and their launches take (device pointers; point_ptr = nullptr: no 2D-3D constraints).
// cam_cur is read and written by the solves; the reports and the covariance only read it.
struct KrtBatch {
  int n_query;
  const long long* match_ptr;
  const float2 *uv_ref, *uv_cur;
  const long long* point_ptr;
  const float2* pt_uv;
  const double* pt_xyz;
  const double* cam_ref;
  double* cam_cur;
};
inline KrtBatch krt_batch_of(int n_query, const int64_t* d_match_ptr, const float* d_uv_ref, const float* d_uv_cur, const int64_t* d_point_ptr,
                             const float* d_pts2d, const double* d_pts3d, const double* d_cam_ref, const double* d_cam_cur)
{
  return {n_query, (const long long*)d_match_ptr, (const float2*)d_uv_ref, (const float2*)d_uv_cur, (const long long*)d_point_ptr,
          (const float2*)d_pts2d, d_pts3d, d_cam_ref, const_cast<double*>(d_cam_cur)};
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// The same batch in the caller's host arrays, as the four host-form entry points get it.
struct KrtHostBatch {
  int n_query;
  const int64_t* match_ptr;
  const float *uv_ref, *uv_cur;
  const int64_t* point_ptr;  // nullptr: no 2D-3D constraints
  const float* pts2d;
  const double* pts3d;
  const double *cam_ref, *cam_cur;
  int64_t n_match() const { return match_ptr[n_query]; }
  int64_t n_point() const { return point_ptr ? point_ptr[n_query] : 0; }
};
// Checks of the CSR arrays before any device work, n_query > 0: PTZ_OK or PTZ_EINVAL.  kKrtCheckMatches: match_ptr, cam_ref, cam_cur
// given; match_ptr starts at 0 and does not decrease; the pixel arrays given if there is a match.  kKrtCheckPoints: the same of
// point_ptr, pts2d, pts3d where point_ptr is given.  kKrtAnyBase: the offset arrays may start anywhere.
//
// The four callers do NOT validate alike, and each keeps what it answered when it was written (tests/golden/krt_return_codes.json):
//                                n_query == 0   offsets start at 0   null pixels, no match   point_ptr order is checked   device_id < 0
//   ptz_krt_solve_batch_2d3d     PTZ_EINVAL     not required         PTZ_EINVAL              before factor_type           not checked
//   ptz_krt_covariance_batch     PTZ_OK         required             accepted                after factor_type            PTZ_EINVAL
//   ptz_krt_residuals_batch      PTZ_OK         required             accepted                after factor_type            PTZ_EINVAL
//   ptz_krt_solve_batch_trimmed  PTZ_OK         required             accepted                after factor_type            PTZ_EINVAL
// (so a decreasing point_ptr with an unknown factor_type is PTZ_EINVAL to the plain solve and PTZ_EUNSUPPORTED to the others; all four
//  ask hipGetDeviceCount only after every argument check, which on a machine without a device decides between PTZ_EINVAL and
//  PTZ_ENODEVICE)
enum : unsigned { kKrtCheckMatches = 1, kKrtCheckPoints = 2, kKrtCheckAll = 3, kKrtAnyBase = 4 };
int check_host_batch(const KrtHostBatch& hb, unsigned what);

// The inputs of `hb` into the block of `h` at the slots krt_batch_reserve() gave them (match_mask / accepted: nullable, as the slots
// were reserved), enqueued on h.st; *out: the batch as the launches take it.  staged: through the pinned block of `h` where it has
// one -- one copy of slots.begin .. slots.end instead of a pageable copy per array, the win of a registration-sized call; only
// ptz_krt_solve_batch_2d3d asks for it (probably a win for the other three as well, but not measured: a change of its own).
hipError_t krt_batch_upload(const KrtHostBatch& hb, const uint8_t* match_mask, const int32_t* accepted, const KrtBatchSlots& slots,
                            const CallHeld& h, bool staged, KrtBatch* out);

// lanes per query of a launch of n_query queries: `requested` (ptz_lm_options::krt_lanes_per_query) if 16 or 64, else PTZ_KRT_GROUP,
// else by launch size
int krt_group_size(int n_query, int requested);
// k_krt over a device-resident batch on `st`.  lanes: the group size, 16 or 64.
// d_active (nullable): queries whose entry is 0 are left alone -- camera, summary and accepted as they were.
void krt_enqueue(const KrtBatch& in, int factor_type, const ptz_lm_options& o, double max_reproj_error, int lanes,
                 ptz_lm_summary* d_summaries, int* d_accepted, const int* d_active, hipStream_t st);

}  // namespace ptz
