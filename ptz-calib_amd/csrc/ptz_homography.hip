// ptz_homography.hip -- batched RANSAC homographies of a match table on the device (ptz_homography_ransac_batch): the pair
// estimator of host/homography.cc, bit for bit, one workgroup (one wave) per pair.
//
// Per pair:
//  * hypothesis batches of 64: lane 0 draws the batch's samples ahead (the random stream does not depend on the fits), every
//    lane fits one sample (normalised 4-point DLT, 9 x 9 Jacobi SVD in its LDS slot) and counts its inliers, then lane 0 applies
//    the acceptance rule in iteration order and stops at the adaptive bound; another batch runs only if the bound is not reached;
//  * the finish: the best model's inliers are compacted in index order (ballot), the DLT refit spreads the 45 distinct AtA
//    entries over lanes, Refine's outer steps the 36 + 8 distinct JtJ / Jtr entries; every entry walks the inliers in index
//    order in ONE lane, and the serial parts (Jacobi, damped solves, costs) run in lane 0;
//  * the mask of the final H, one point per lane.
// The points stay in global memory (no size limit besides int32 extents); LDS holds the 64 Jacobi slots (162 doubles per lane).
#include <algorithm>
#include <cmath>
#include <unordered_map>
#include <vector>

#include "ptz_common.h"
#include "ptz_homography.h"
#include "ptz_pool.h"

namespace ptz {
namespace {

constexpr int HB = 64;       // lanes of the workgroup = hypotheses per batch
constexpr int HSLOT = 162;   // doubles of Jacobi storage per lane: two 9 x 9 matrices

__global__ __launch_bounds__(HB) void k_homography_ransac(const int64_t* __restrict__ ptr, const int32_t* __restrict__ order,
                                                          const float* __restrict__ src_uv, const float* __restrict__ dst_uv,
                                                          double thr2, const int64_t* __restrict__ bound_off,
                                                          const int32_t* __restrict__ bound, double* __restrict__ H_out,
                                                          int32_t* __restrict__ found, uint8_t* __restrict__ mask,
                                                          int32_t* __restrict__ inl_ws)
{
  __shared__ double s_ws[HSLOT * HB];  // lane l's slot: element k at s_ws[k * HB + l]
  __shared__ double s_hyp[9 * HB];     // the batch's fitted hypotheses
  __shared__ int s_smp[4 * HB];        // the batch's samples
  __shared__ int s_cnt[HB];            // inlier counts; -1: no valid sample or a failed fit
  __shared__ double s_H[9];            // best model, then the refined one
  __shared__ double s_cs[6];           // normalisations of the refit
  __shared__ double s_jj[72];          // JtJ (64) and Jtr (8)
  __shared__ int s_ctl[3];             // best inliers, max_iters, Refine goes on
  const int p = order[blockIdx.x];
  const int lane = threadIdx.x;
  const int64_t base = ptr[p];
  const int n = static_cast<int>(ptr[p + 1] - base);
  const float* src = src_uv + 2 * base;
  const float* dst = dst_uv + 2 * base;
  double* ws = s_ws + lane;
  if (n < 4) {
    if (lane == 0) found[p] = 0;
    return;
  }
  if (n == 4) {  // a direct fit of the four
    if (lane == 0) {
      const int all[4] = {0, 1, 2, 3};
      double H[9];
      const bool ok = ptzh_fit_dlt(src, dst, all, 4, ws, HB, H);
      for (int k = 0; k < 9; ++k) s_H[k] = H[k];
      s_ctl[0] = ok ? 4 : 0;
    }
  }
  else {
    uint64_t rng = PTZH_SEED;
    const int32_t* bnd = bound + bound_off[p];
    if (lane == 0) { s_ctl[0] = 0; s_ctl[1] = PTZH_MAX_ITERS; }
    for (int it0 = 0;; it0 += HB) {
      if (lane == 0)
        for (int l = 0; l < HB; ++l) s_cnt[l] = ptzh_draw_sample(rng, n, src, dst, s_smp + 4 * l) ? 0 : -1;
      __syncthreads();
      int cnt = -1;
      if (s_cnt[lane] == 0) {
        const int s[4] = {s_smp[4 * lane], s_smp[4 * lane + 1], s_smp[4 * lane + 2], s_smp[4 * lane + 3]};
        double Hs[9];
        if (ptzh_fit_sample(src, dst, s, ws, HB, Hs)) {
          cnt = ptzh_count_inliers(Hs, src, dst, n, thr2);
          for (int k = 0; k < 9; ++k) s_hyp[k * HB + lane] = Hs[k];
        }
      }
      __syncthreads();
      s_cnt[lane] = cnt;
      __syncthreads();
      if (lane == 0) {  // the host's acceptance, in iteration order, up to the bound
        int best = s_ctl[0], max_iters = s_ctl[1];
        for (int l = 0; l < HB && it0 + l < max_iters; ++l) {
          const int c = s_cnt[l];
          if (c < 0) continue;
          if (ptzh_accept(c, it0 + l, bnd[c], best, max_iters))
            for (int k = 0; k < 9; ++k) s_H[k] = s_hyp[k * HB + l];
        }
        s_ctl[0] = best; s_ctl[1] = max_iters;
      }
      __syncthreads();
      if (it0 + HB >= s_ctl[1]) break;
    }
  }
  __syncthreads();
  if (s_ctl[0] < 4) {
    if (lane == 0) found[p] = 0;
    return;
  }
  double Hb[9];
  for (int k = 0; k < 9; ++k) Hb[k] = s_H[k];
  // the best model's inliers, in index order
  int32_t* inl = inl_ws + base;
  int m = 0;
  for (int i0 = 0; i0 < n; i0 += HB) {
    const int i = i0 + lane;
    const bool in = i < n && ptzh_err2(Hb, src + 2 * i, dst + 2 * i) <= thr2;
    const unsigned long long bal = __ballot(in);
    if (in) inl[m + __popcll(bal & ((1ull << lane) - 1ull))] = i;
    m += __popcll(bal);
  }
  if (m < 4) {
    if (lane == 0) found[p] = 0;
    return;
  }
  __syncthreads();  // the inlier list is read by every lane
  // DLT refit: normalisations (lanes 0, 1), the 45 distinct AtA entries (one lane each) into lane 0's slot, the SVD in lane 0
  if (lane < 2) ptzh_normalisation(lane == 0 ? src : dst, inl, m, s_cs + 3 * lane);
  __syncthreads();
  if (lane < 45) {
    int a = 0, e = lane;
    while (e >= 9 - a) { e -= 9 - a; ++a; }
    const int b = a + e;
    double cs[6];
    for (int k = 0; k < 6; ++k) cs[k] = s_cs[k];
    const double v = ptzh_ata_entry(a, b, src, dst, inl, m, cs);
    s_ws[(9 * a + b) * HB] = v;
    s_ws[(9 * b + a) * HB] = v;
  }
  __syncthreads();
  if (lane == 0) {
    double cs[6], H[9];
    for (int k = 0; k < 6; ++k) cs[k] = s_cs[k];
    const bool ok = ptzh_dlt_solve(s_ws, s_ws + 81 * HB, HB, cs, H);
    for (int k = 0; k < 9; ++k) s_H[k] = ok ? H[k] : Hb[k];
    s_ctl[2] = ok;
  }
  __syncthreads();
  if (s_ctl[2]) {  // Refine
    PtzhRefine r;
    double H[9];
    for (int k = 0; k < 9; ++k) H[k] = s_H[k];
    if (lane == 0) ptzh_refine_begin(r, H, src, dst, inl, m);
    for (;;) {
      if (lane < 44) {
        double v;
        if (lane < 36) {
          int a = 0, e = lane;
          while (e >= 8 - a) { e -= 8 - a; ++a; }
          const int b = a + e;
          v = ptzh_jtj_entry(a, b, H, src, dst, inl, m);
          s_jj[8 * a + b] = v;
          s_jj[8 * b + a] = v;
        }
        else
          s_jj[64 + lane - 36] = ptzh_jtr_entry(lane - 36, H, src, dst, inl, m);
      }
      __syncthreads();
      if (lane == 0) {
        s_ctl[2] = ptzh_refine_step(r, H, s_jj, s_jj + 64, src, dst, inl, m, s_ws, HB);
        for (int k = 0; k < 9; ++k) s_H[k] = H[k];
      }
      __syncthreads();
      if (!s_ctl[2]) break;
      for (int k = 0; k < 9; ++k) H[k] = s_H[k];
    }
  }
  __syncthreads();
  double H[9];
  for (int k = 0; k < 9; ++k) H[k] = s_H[k];
  const double inv = 1.0 / H[8];
  for (int k = 0; k < 9; ++k) H[k] *= inv;
  if (lane == 0) {
    for (int k = 0; k < 9; ++k) H_out[9 * (int64_t)p + k] = H[k];
    found[p] = 1;
  }
  if (mask)
    for (int i = lane; i < n; i += HB) mask[base + i] = ptzh_err2(H, src + 2 * i, dst + 2 * i) <= thr2;
}

}  // namespace
}  // namespace ptz

extern "C" int32_t ptz_homography_ransac_batch(int32_t n_pair, const int64_t* match_ptr, const float* src_uv, const float* dst_uv,
                                               double ransac_thresh, int32_t device_id, double* H, int32_t* found,
                                               uint8_t* inlier_mask, double* device_ms)
{
  using namespace ptz;
  // validation first, device second
  if (n_pair < 0 || !(std::isfinite(ransac_thresh) && ransac_thresh > 0)) return PTZ_EINVAL;
  if (n_pair > 0 && (!match_ptr || !H || !found)) return PTZ_EINVAL;
  if (match_ptr && match_ptr[0] != 0) return PTZ_EINVAL;
  int64_t longest = 0;
  for (int p = 0; p < n_pair; ++p) {
    if (match_ptr[p + 1] < match_ptr[p]) return PTZ_EINVAL;
    longest = std::max<int64_t>(longest, match_ptr[p + 1] - match_ptr[p]);
  }
  const int64_t nm = n_pair > 0 ? match_ptr[n_pair] : 0;
  if (nm > 0 && (!src_uv || !dst_uv)) return PTZ_EINVAL;
  if (device_ms) *device_ms = 0;
  if (n_pair == 0) return PTZ_OK;
  if (longest > INT32_MAX) return PTZ_ELIMIT;
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);

  // host side: the adaptive bound per distinct pair size (>= 5), and the launch order (largest pairs first)
  std::vector<int64_t> boff(n_pair, 0);
  std::vector<int32_t> tab;
  {
    std::unordered_map<int, int64_t> at;
    for (int p = 0; p < n_pair; ++p) {
      const int n = static_cast<int>(match_ptr[p + 1] - match_ptr[p]);
      if (n < 5) continue;
      auto f = at.find(n);
      if (f == at.end()) {
        f = at.emplace(n, static_cast<int64_t>(tab.size())).first;
        tab.resize(tab.size() + n + 1);
        (void)ptz_debug_homography_bounds(n, tab.data() + f->second);
      }
      boff[p] = f->second;
    }
  }
  if (tab.empty()) tab.push_back(0);
  std::vector<int32_t> order(n_pair);
  for (int p = 0; p < n_pair; ++p) order[p] = p;
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return match_ptr[a + 1] - match_ptr[a] > match_ptr[b + 1] - match_ptr[b]; });

  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t nmx = nm > 0 ? (size_t)nm : 1;
  const size_t o_ptr = 0, o_ord = o_ptr + up(sizeof(int64_t) * (n_pair + 1)), o_boff = o_ord + up(sizeof(int32_t) * n_pair),
               o_tab = o_boff + up(sizeof(int64_t) * n_pair), o_src = o_tab + up(sizeof(int32_t) * tab.size()),
               o_dst = o_src + up(sizeof(float) * 2 * nmx), o_H = o_dst + up(sizeof(float) * 2 * nmx),
               o_found = o_H + up(sizeof(double) * 9 * n_pair), o_mask = o_found + up(sizeof(int32_t) * n_pair),
               o_inl = o_mask + up(nmx), total = o_inl + up(sizeof(int32_t) * nmx);
  struct Held {
    int dev; char* base = nullptr; hipStream_t st = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Held()
    {
      if (st) (void)stream_wait(st);
      ptzpool::dev_release(dev, base);
      ptzpool::stream_release(dev, st);
      ptzpool::event_release(dev, true, e0);
      ptzpool::event_release(dev, true, e1);
    }
  } h;
  h.dev = device_id;
  if (ptzpool::dev_acquire(h.dev, total, (void**)&h.base) != hipSuccess) return PTZ_ENOMEM;
  PTZ_HIP_TRY(ptzpool::stream_acquire(h.dev, &h.st));
  PTZ_HIP_TRY(ptzpool::event_acquire(h.dev, true, &h.e0));
  PTZ_HIP_TRY(ptzpool::event_acquire(h.dev, true, &h.e1));
  char* b = h.base;
  PTZ_HIP_TRY(hipMemcpyAsync(b + o_ptr, match_ptr, sizeof(int64_t) * (n_pair + 1), hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(b + o_ord, order.data(), sizeof(int32_t) * n_pair, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(b + o_boff, boff.data(), sizeof(int64_t) * n_pair, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(b + o_tab, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, h.st));
  if (nm > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(b + o_src, src_uv, sizeof(float) * 2 * nm, hipMemcpyHostToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(b + o_dst, dst_uv, sizeof(float) * 2 * nm, hipMemcpyHostToDevice, h.st));
  }
  uint8_t* d_mask = inlier_mask ? (uint8_t*)(b + o_mask) : nullptr;
  PTZ_HIP_TRY(hipEventRecord(h.e0, h.st));
  hipLaunchKernelGGL(k_homography_ransac, dim3(n_pair), dim3(HB), 0, h.st, (const int64_t*)(b + o_ptr), (const int32_t*)(b + o_ord),
                     (const float*)(b + o_src), (const float*)(b + o_dst), ransac_thresh * ransac_thresh,
                     (const int64_t*)(b + o_boff), (const int32_t*)(b + o_tab), (double*)(b + o_H), (int32_t*)(b + o_found), d_mask,
                     (int32_t*)(b + o_inl));
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(hipEventRecord(h.e1, h.st));
  std::vector<double> Hd(9 * (size_t)n_pair);
  std::vector<uint8_t> md(inlier_mask ? nmx : 0);
  PTZ_HIP_TRY(hipMemcpyAsync(Hd.data(), b + o_H, sizeof(double) * 9 * n_pair, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(found, b + o_found, sizeof(int32_t) * n_pair, hipMemcpyDeviceToHost, h.st));
  if (inlier_mask && nm > 0) PTZ_HIP_TRY(hipMemcpyAsync(md.data(), d_mask, nm, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  PTZ_HIP_TRY(hipGetLastError());
  float ms = 0;
  (void)hipEventElapsedTime(&ms, h.e0, h.e1);
  if (device_ms) *device_ms = ms;
  // H and mask of a pair that is not found stay untouched, as with the host estimator
  for (int p = 0; p < n_pair; ++p) {
    if (!found[p]) continue;
    memcpy(H + 9 * (size_t)p, Hd.data() + 9 * (size_t)p, sizeof(double) * 9);
    if (inlier_mask) memcpy(inlier_mask + match_ptr[p], md.data() + match_ptr[p], match_ptr[p + 1] - match_ptr[p]);
  }
  return PTZ_OK;
}
