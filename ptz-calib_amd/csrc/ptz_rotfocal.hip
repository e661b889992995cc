// ptz_rotfocal.hip -- the rotation-and-focal match gate (ptz_rotfocal_gate): a fixed-count two-point RANSAC per assembled query, the
// contract of ptz_rotfocal.h bit for bit, one workgroup per query, one hypothesis per thread.
//
// Per query:
//  * thread t owns hypothesis number t, then t + 256, .. up to 2 iters: it draws the iteration's sample (the generator depends on the
//    iteration and the query's size only), lifts the two matches from global memory and builds (f, R) in registers;
//  * the query's matches pass through LDS in tiles of 1024, LIFTED ONCE by the thread that stages them (a_x, a_y, q_x, q_y as doubles:
//    the two divisions of the lift are paid once per match and round, not once per match and hypothesis; the lift's bits are the same
//    wherever it runs).  Every lane then walks the tile at the same address -- a broadcast read -- and counts into a private integer;
//  * no floating-point value ever crosses lanes: the best (count, lowest number) is an integer key, reduced by shuffles in the wave
//    and through LDS over the four waves; every thread rebuilds the winning hypothesis from its number, and the mask is written by
//    threads striding over the matches.
// A query may have any number of matches up to 2^31 - 1: there is no table and no per-query limit.
//
// Counting, the exclusive scan of the counts and the in-order scatter are the match gate's integer kernels (ptz_gate_compact.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "ptz_common.h"
#include "ptz_rotfocal.h"
#include "ptz_gate_compact.h"
#include "ptz_pool.h"
#include "ptz_host_batch.h"

namespace ptz {
namespace {

constexpr int RF_WG = 256;     // four waves; a round of the workgroup covers 256 hypotheses = 128 iterations
constexpr int RF_TILE = 1024;  // lifted matches per LDS tile: 32 KiB

__global__ __launch_bounds__(RF_WG) void k_rotfocal_ransac(const int64_t* __restrict__ ptr, const float* __restrict__ uv_a,
                                                          const float* __restrict__ uv_b, const double* __restrict__ cam_ref,
                                                          const double* __restrict__ cam_cur, double thr2, int iters, int64_t max_matches,
                                                          double* __restrict__ model_out, double* __restrict__ H_out,
                                                          int32_t* __restrict__ found, uint8_t* __restrict__ mask)
{
  __shared__ double s_l[4 * RF_TILE];
  __shared__ unsigned long long s_key[RF_WG / WAVE];
  const int64_t p = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t base = ptr[p], end = ptr[p + 1];
  // device-resident offsets: a range the caller's storage cannot hold is answered found = -1 and touches nothing else
  if (base < 0 || end < base || end > max_matches || end - base > INT32_MAX) {
    if (t == 0) found[p] = -1;
    return;
  }
  const int n = static_cast<int>(end - base);
  if (n < 2) {
    if (t == 0) found[p] = 0;
    return;
  }
  const float* a = uv_a + 2 * base;
  const float* b = uv_b + 2 * base;
  const double cam[4] = {cam_ref[15 * p], cam_ref[15 * p + 1], cam_ref[15 * p + 2], cam_ref[15 * p + 3]};
  const double cxq = cam_cur[15 * p + 2], cyq = cam_cur[15 * p + 3];

  int best = -1, best_h = 0;
  const int n_hyp = 2 * iters;
  for (int h0 = 0; h0 < n_hyp; h0 += RF_WG) {
    const int h = h0 + t;
    double m[10];
    const bool valid = h < n_hyp && ptzrf_hypothesis_of(h, n, a, b, cam, cxq, cyq, m);
    int c = 0;
    for (int64_t i0 = 0; i0 < n; i0 += RF_TILE) {
      const int len = static_cast<int>(std::min<int64_t>(RF_TILE, n - i0));
      __syncthreads();  // the previous tile has been read by everyone
      for (int k = t; k < len; k += RF_WG) {
        double l[4];
        ptzrf_lift(cam, cxq, cyq, a + 2 * (i0 + k), b + 2 * (i0 + k), l);
        s_l[4 * k] = l[0]; s_l[4 * k + 1] = l[1]; s_l[4 * k + 2] = l[2]; s_l[4 * k + 3] = l[3];
      }
      __syncthreads();
      if (valid) {
#pragma unroll 4
        for (int k = 0; k < len; ++k) c += ptzrf_inlier(m, s_l[4 * k], s_l[4 * k + 1], s_l[4 * k + 2], s_l[4 * k + 3], thr2) ? 1 : 0;
      }
    }
    if (valid && c > best) { best = c; best_h = h; }  // a thread's numbers ascend: its first best is its lowest
  }
  // most inliers, then the lowest number: one integer key, its maximum over the workgroup
  unsigned long long key = best < 0 ? 0ull : (static_cast<unsigned long long>(best + 1) << 32) | static_cast<unsigned int>(0x7FFFFFFF - best_h);
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(key, d);
    key = o > key ? o : key;
  }
  if (t % WAVE == 0) s_key[t / WAVE] = key;
  __syncthreads();
  key = s_key[0];
  for (int w = 1; w < RF_WG / WAVE; ++w) key = s_key[w] > key ? s_key[w] : key;
  const int cnt = static_cast<int>(key >> 32) - 1;
  if (cnt < PTZRF_MIN_COUNT) {
    if (t == 0) found[p] = 0;
    return;
  }
  const int hb = 0x7FFFFFFF - static_cast<int>(key & 0xFFFFFFFFull);
  double m[10];
  (void)ptzrf_hypothesis_of(hb, n, a, b, cam, cxq, cyq, m);
  if (t == 0) {
    for (int k = 0; k < 10; ++k) model_out[10 * p + k] = m[k];
    if (H_out) {
      double H[9];
      ptzrf_homography(m, cam, cxq, cyq, H);
      for (int k = 0; k < 9; ++k) H_out[9 * p + k] = H[k];
    }
    found[p] = 1;
  }
  for (int64_t i = t; i < n; i += RF_WG) {
    double l[4];
    ptzrf_lift(cam, cxq, cyq, a + 2 * i, b + 2 * i, l);
    mask[base + i] = ptzrf_inlier(m, l[0], l[1], l[2], l[3], thr2) ? 1 : 0;
  }
}

// offsets that start at 0 and do not decrease, arrays where there are matches
int32_t check_csr(int32_t n_pair, const int64_t* match_ptr, const float* uv_a, const float* uv_b)
{
  if (n_pair > 0 && !match_ptr) return PTZ_EINVAL;
  if (n_pair > 0 && match_ptr[0] != 0) return PTZ_EINVAL;
  for (int p = 0; p < n_pair; ++p)
    if (match_ptr[p + 1] < match_ptr[p]) return PTZ_EINVAL;
  if (n_pair > 0 && match_ptr[n_pair] > 0 && (!uv_a || !uv_b)) return PTZ_EINVAL;
  return PTZ_OK;
}

bool options_ok(double thresh, int32_t min_inliers, int32_t iters)
{
  return std::isfinite(thresh) && thresh > 0 && min_inliers >= 0 && iters >= 1 && iters <= PTZRF_MAX_ITERS;
}

}  // namespace
}  // namespace ptz

struct ptz_rotfocal_gate {
  int device = 0;
  int32_t max_pairs = 0;
  int64_t max_matches = 0;
  char* base = nullptr;        // one pooled block behind everything below
  int32_t* d_cnt = nullptr;    // [max_pairs] kept matches of a run's queries
  double* d_model = nullptr;   // [10 max_pairs] the models of callers that ask for none
  uint8_t* d_mask = nullptr;   // [max_matches] the mask of callers that ask for none
};

extern "C" int32_t ptz_rotfocal_gate_create(int32_t max_pairs, int64_t max_matches, int32_t device_id, ptz_rotfocal_gate** out)
{
  using namespace ptz;
  if (!out) return PTZ_EINVAL;
  *out = nullptr;
  if (max_pairs <= 0 || max_matches < 0 || device_id < 0) return PTZ_EINVAL;
  if (max_matches > INT32_MAX) return PTZ_ELIMIT;  // out_index is int32
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);
  const size_t nmx = (size_t)std::max<int64_t>(max_matches, 1);
  const size_t o_cnt = 0, o_model = o_cnt + up256(sizeof(int32_t) * max_pairs), o_mask = o_model + up256(sizeof(double) * 10 * max_pairs),
               total = o_mask + up256(nmx);
  std::unique_ptr<ptz_rotfocal_gate> g(new ptz_rotfocal_gate());
  g->device = device_id; g->max_pairs = max_pairs; g->max_matches = max_matches;
  void* blk = nullptr;
  if (ptzpool::dev_acquire(device_id, total, &blk) != hipSuccess) return PTZ_ENOMEM;
  g->base = static_cast<char*>(blk);
  g->d_cnt = (int32_t*)(g->base + o_cnt); g->d_model = (double*)(g->base + o_model); g->d_mask = (uint8_t*)(g->base + o_mask);
  *out = g.release();
  return PTZ_OK;
}

extern "C" void ptz_rotfocal_gate_destroy(ptz_rotfocal_gate* g)
{
  if (!g) return;
  ptz::DeviceGuard guard(g->device);
  ptzpool::dev_release(g->device, g->base);
  delete g;
}

extern "C" int32_t ptz_rotfocal_gate_run_device(ptz_rotfocal_gate* g, int32_t n_pair, const int64_t* d_match_ptr, const float* d_uv_a,
                                                const float* d_uv_b, const double* d_cam_ref, const double* d_cam_cur, double thresh,
                                                int32_t min_inliers, int32_t iters, double* d_model, double* d_H, int32_t* d_found,
                                                uint8_t* d_mask, int64_t* d_out_ptr, float* d_out_uv_a, float* d_out_uv_b,
                                                int32_t* d_out_index, void* hip_stream)
{
  using namespace ptz;
  if (!g || n_pair < 0 || !options_ok(thresh, min_inliers, iters) || !d_out_ptr) return PTZ_EINVAL;
  if (n_pair > 0 && (!d_match_ptr || !d_found || !d_cam_ref || !d_cam_cur)) return PTZ_EINVAL;
  if (n_pair > 0 && g->max_matches > 0 && (!d_uv_a || !d_uv_b || !d_out_uv_a || !d_out_uv_b)) return PTZ_EINVAL;
  if (n_pair > g->max_pairs) return PTZ_ELIMIT;
  clear_stale_error(__func__);
  if (hip_stream) {
    hipDevice_t sdev = -1;
    if (hipStreamGetDevice((hipStream_t)hip_stream, &sdev) != hipSuccess) { (void)hipGetLastError(); return PTZ_EINVAL; }
    if ((int)sdev != g->device) return PTZ_EINVAL;  // the stream must belong to the gate's device
  }
  PTZ_DEVICE_GUARD(g->device);
  hipStream_t st = (hipStream_t)hip_stream;
  uint8_t* mask = d_mask ? d_mask : g->d_mask;
  if (n_pair > 0)
    hipLaunchKernelGGL(k_rotfocal_ransac, dim3(n_pair), dim3(RF_WG), 0, st, d_match_ptr, d_uv_a, d_uv_b, d_cam_ref, d_cam_cur, thresh * thresh,
                       iters, g->max_matches, d_model ? d_model : g->d_model, d_H, d_found, mask);
  enqueue_compact(n_pair, d_match_ptr, (const int32_t*)d_found, (const uint8_t*)mask, std::max(min_inliers, 4), g->d_cnt, d_out_ptr,
                  (const float2*)d_uv_a, (const float2*)d_uv_b, (float2*)d_out_uv_a, (float2*)d_out_uv_b, d_out_index, st);
  PTZ_HIP_TRY(hipGetLastError());
  return PTZ_OK;
}

// the gate on HOST arrays: upload, ptz_rotfocal_gate_run_device, download
extern "C" int32_t ptz_rotfocal_gate_run(ptz_rotfocal_gate* g, int32_t n_pair, const int64_t* match_ptr, const float* uv_a, const float* uv_b,
                                         const double* cam_ref, const double* cam_cur, double thresh, int32_t min_inliers, int32_t iters,
                                         double* model, double* H, int32_t* found, uint8_t* mask, int64_t* out_ptr, float* out_uv_a,
                                         float* out_uv_b, int32_t* out_index, double* device_ms)
{
  using namespace ptz;
  if (!g || n_pair < 0 || !options_ok(thresh, min_inliers, iters) || !out_ptr) return PTZ_EINVAL;
  if (const int32_t rc = check_csr(n_pair, match_ptr, uv_a, uv_b)) return rc;
  if (n_pair > 0 && (!found || !cam_ref || !cam_cur)) return PTZ_EINVAL;
  const int64_t nm = n_pair > 0 ? match_ptr[n_pair] : 0;
  if (nm > 0 && (!out_uv_a || !out_uv_b)) return PTZ_EINVAL;
  if (n_pair > g->max_pairs || nm > g->max_matches) return PTZ_ELIMIT;
  if (device_ms) *device_ms = 0;
  if (n_pair == 0) { out_ptr[0] = 0; return PTZ_OK; }
  clear_stale_error(__func__);
  PTZ_DEVICE_GUARD(g->device);
  const size_t nmx = nm > 0 ? (size_t)nm : 1, np = (size_t)n_pair, np1 = np + 1;
  const size_t o_ptr = 0, o_a = o_ptr + up256(sizeof(int64_t) * np1), o_b = o_a + up256(sizeof(float) * 2 * nmx),
               o_cr = o_b + up256(sizeof(float) * 2 * nmx), o_cc = o_cr + up256(sizeof(double) * 15 * np), o_m = o_cc + up256(sizeof(double) * 15 * np),
               o_H = o_m + up256(sizeof(double) * 10 * np), o_found = o_H + up256(sizeof(double) * 9 * np), o_mask = o_found + up256(sizeof(int32_t) * np),
               o_optr = o_mask + up256(nmx), o_oa = o_optr + up256(sizeof(int64_t) * np1), o_ob = o_oa + up256(sizeof(float) * 2 * nmx),
               o_oi = o_ob + up256(sizeof(float) * 2 * nmx), total = o_oi + up256(sizeof(int32_t) * nmx);
  CallHeld h;
  if (const int32_t rc = h.acquire(g->device, total)) return rc;
  char* b = h.base;
  PTZ_HIP_TRY(hipMemcpyAsync(b + o_ptr, match_ptr, sizeof(int64_t) * np1, hipMemcpyHostToDevice, h.st));
  if (nm > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(b + o_a, uv_a, sizeof(float) * 2 * nm, hipMemcpyHostToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(b + o_b, uv_b, sizeof(float) * 2 * nm, hipMemcpyHostToDevice, h.st));
  }
  PTZ_HIP_TRY(hipMemcpyAsync(b + o_cr, cam_ref, sizeof(double) * 15 * np, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(b + o_cc, cam_cur, sizeof(double) * 15 * np, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  if (const int32_t rc = ptz_rotfocal_gate_run_device(g, n_pair, (const int64_t*)(b + o_ptr), (const float*)(b + o_a), (const float*)(b + o_b),
                                                      (const double*)(b + o_cr), (const double*)(b + o_cc), thresh, min_inliers, iters,
                                                      (double*)(b + o_m), H ? (double*)(b + o_H) : nullptr, (int32_t*)(b + o_found),
                                                      (uint8_t*)(b + o_mask), (int64_t*)(b + o_optr), (float*)(b + o_oa), (float*)(b + o_ob),
                                                      (int32_t*)(b + o_oi), h.st))
    return rc;
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  std::vector<double> md(model ? 10 * np : 0), Hd(H ? 9 * np : 0);
  std::vector<uint8_t> kd(mask ? nmx : 0);
  if (model) PTZ_HIP_TRY(hipMemcpyAsync(md.data(), b + o_m, sizeof(double) * 10 * np, hipMemcpyDeviceToHost, h.st));
  if (H) PTZ_HIP_TRY(hipMemcpyAsync(Hd.data(), b + o_H, sizeof(double) * 9 * np, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(found, b + o_found, sizeof(int32_t) * np, hipMemcpyDeviceToHost, h.st));
  if (mask && nm > 0) PTZ_HIP_TRY(hipMemcpyAsync(kd.data(), b + o_mask, nm, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(out_ptr, b + o_optr, sizeof(int64_t) * np1, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  PTZ_HIP_TRY(hipGetLastError());
  const int64_t kept = out_ptr[n_pair];
  if (kept < 0 || kept > nm) return PTZ_ENODEVICE;  // cannot happen: the scan of counts that are at most the queries' sizes
  if (kept > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(out_uv_a, b + o_oa, sizeof(float) * 2 * kept, hipMemcpyDeviceToHost, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(out_uv_b, b + o_ob, sizeof(float) * 2 * kept, hipMemcpyDeviceToHost, h.st));
    if (out_index) PTZ_HIP_TRY(hipMemcpyAsync(out_index, b + o_oi, sizeof(int32_t) * kept, hipMemcpyDeviceToHost, h.st));
    PTZ_HIP_TRY(stream_wait(h.st));
  }
  if (device_ms) *device_ms = h.elapsed_ms();
  // model, H and mask of a query without a model stay untouched, as with ptz_match_gate_run
  for (int p = 0; p < n_pair; ++p) {
    if (found[p] != 1) continue;
    if (model) memcpy(model + 10 * (size_t)p, md.data() + 10 * (size_t)p, sizeof(double) * 10);
    if (H) memcpy(H + 9 * (size_t)p, Hd.data() + 9 * (size_t)p, sizeof(double) * 9);
    if (mask) memcpy(mask + match_ptr[p], kd.data() + match_ptr[p], match_ptr[p + 1] - match_ptr[p]);
  }
  return PTZ_OK;
}
