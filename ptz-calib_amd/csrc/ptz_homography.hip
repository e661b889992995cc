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
//
// The match gate (ptz_match_gate, ptz_krt_solve_batch_gated) puts the estimator's mask to use: a pair passes with a model and
// enough inliers, and a passing pair keeps its inliers in their order.  Counting, the exclusive scan of the counts and the
// in-order scatter are integer kernels behind the estimator on the same stream; nothing returns to the host in between.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <unordered_map>
#include <vector>

#include "ptz_common.h"
#include "ptz_homography.h"
#include "ptz_gate_compact.h"
#include "ptz_pool.h"
#include "ptz_host_batch.h"

namespace ptz {
namespace {

constexpr int HB = 64;       // lanes of the workgroup = hypotheses per batch
constexpr int HSLOT = 162;   // doubles of Jacobi storage per lane: two 9 x 9 matrices

__global__ __launch_bounds__(HB) void k_homography_ransac(const int64_t* __restrict__ ptr, const int32_t* __restrict__ order,
                                                          const float* __restrict__ src_uv, const float* __restrict__ dst_uv,
                                                          double thr2, const int64_t* __restrict__ bound_off,
                                                          const int32_t* __restrict__ bound, double* __restrict__ H_out,
                                                          int32_t* __restrict__ found, uint8_t* __restrict__ mask,
                                                          int32_t* __restrict__ inl_ws, int32_t max_n, int64_t max_matches)
{
  __shared__ double s_ws[HSLOT * HB];  // lane l's slot: element k at s_ws[k * HB + l]
  __shared__ double s_hyp[9 * HB];     // the batch's fitted hypotheses
  __shared__ int s_smp[4 * HB];        // the batch's samples
  __shared__ int s_cnt[HB];            // inlier counts; -1: no valid sample or a failed fit
  __shared__ double s_H[9];            // best model, then the refined one
  __shared__ double s_cs[6];           // normalisations of the refit
  __shared__ double s_jj[72];          // JtJ (64) and Jtr (8)
  __shared__ int s_ctl[3];             // best inliers, max_iters, Refine goes on
  const int p = order ? order[blockIdx.x] : static_cast<int>(blockIdx.x);  // no order: the pairs run in their own order
  const int lane = threadIdx.x;
  const int64_t base = ptr[p];
  // a pair the caller's storage cannot serve (device-resident offsets, ptz_match_gate): k_gate_prepare has set found = -1
  if (base < 0 || ptr[p + 1] < base || ptr[p + 1] > max_matches || ptr[p + 1] - base > max_n) return;
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

// ---- the match gate's integer kernels -----------------------------------------------------------------------------------
constexpr int GATE_WG = 256;   // four waves, one pair each
constexpr int SCAN_WG = 1024;  // the scan's single workgroup

// A gate holds the bound table of EVERY pair size 5 .. max_pair_matches, size after size: size n's n + 1 entries begin at
// the sum of (k + 1) over k in [5, n).
__host__ __device__ inline int64_t gate_table_offset(int64_t n) { return n < 5 ? 0 : n * (n + 1) / 2 - 15; }

// device-resident offsets: every pair's table offset; a pair the gate cannot serve (more matches than max_n, a range outside
// [0, max_matches]) gets found = -1 here and is skipped by every later kernel
__global__ void k_gate_prepare(int n_pair, const int64_t* __restrict__ ptr, int32_t max_n, int64_t max_matches,
                               int64_t* __restrict__ boff, int32_t* __restrict__ found)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pair) return;
  const int64_t a = ptr[p], b = ptr[p + 1];
  if (a < 0 || b < a || b > max_matches || b - a > max_n) {
    boff[p] = 0;
    found[p] = -1;
    return;
  }
  boff[p] = gate_table_offset(b - a);
}

// kept matches per pair: the ones of its mask if the pair has a model and at least `need` of them, else none.  found decides
// first: the mask bytes of a pair without a model are whatever an earlier run left there.
__global__ __launch_bounds__(GATE_WG) void k_gate_count(int n_pair, const int64_t* __restrict__ ptr, const int32_t* __restrict__ found,
                                                        const uint8_t* __restrict__ mask, int32_t need, int32_t* __restrict__ cnt,
                                                        const int32_t* __restrict__ live)
{
  const int p = blockIdx.x * (GATE_WG / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (p >= n_pair) return;
  if (live && *live == 0) return;  // (ptz_gate_compact.h: no pair has work, nothing is read afterwards)
  int c = 0;
  if (found[p] == 1) {
    const int64_t base = ptr[p];
    const int n = static_cast<int>(ptr[p + 1] - base);
    for (int i0 = 0; i0 < n; i0 += WAVE) {
      const int i = i0 + lane;
      c += __popcll(__ballot(i < n && mask[base + i] != 0));
    }
  }
  if (lane == 0) cnt[p] = c >= need ? c : 0;
}

// out_ptr = exclusive scan of cnt, out_ptr[n_pair] = the total.  One workgroup walks the counts 1024 at a time with a running
// carry: a shuffle scan inside each wave, the sixteen wave totals through LDS.
__global__ __launch_bounds__(SCAN_WG) void k_gate_scan(int n_pair, const int32_t* __restrict__ cnt, int64_t* __restrict__ out_ptr,
                                                       const int32_t* __restrict__ live)
{
  __shared__ long long s_wave[SCAN_WG / WAVE];
  __shared__ long long s_carry;
  if (live && *live == 0) return;  // (the whole workgroup: one value)
  const int t = threadIdx.x, lane = t % WAVE, w = t / WAVE;
  if (t == 0) s_carry = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n_pair; i0 += SCAN_WG) {
    const int i = i0 + t;
    const long long v = i < n_pair ? cnt[i] : 0;
    long long x = v;  // inclusive in the wave
    for (int d = 1; d < WAVE; d <<= 1) {
      const long long y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    if (lane == WAVE - 1) s_wave[w] = x;
    __syncthreads();
    long long below = s_carry;
    for (int k = 0; k < w; ++k) below += s_wave[k];
    if (i < n_pair) out_ptr[i] = below + x - v;
    __syncthreads();
    if (t == SCAN_WG - 1) s_carry = below + x;
    __syncthreads();
  }
  if (t == 0) out_ptr[n_pair] = s_carry;
}

// a passing pair's kept matches to out_ptr[p] .., in their order: 64 matches a step, ballot of the mask bytes, a lane's slot =
// the ones below it, the base moves on by the step's ones
__global__ __launch_bounds__(GATE_WG) void k_gate_scatter(int n_pair, const int64_t* __restrict__ ptr, const float2* __restrict__ uv_a,
                                                          const float2* __restrict__ uv_b, const uint8_t* __restrict__ mask,
                                                          const int32_t* __restrict__ cnt, const int64_t* __restrict__ out_ptr,
                                                          float2* __restrict__ out_a, float2* __restrict__ out_b,
                                                          int32_t* __restrict__ out_index, const int32_t* __restrict__ live)
{
  const int p = blockIdx.x * (GATE_WG / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (p >= n_pair || (live && *live == 0) || cnt[p] == 0) return;
  const int64_t base = ptr[p];
  const int n = static_cast<int>(ptr[p + 1] - base);
  int64_t o = out_ptr[p];
  for (int i0 = 0; i0 < n; i0 += WAVE) {
    const int i = i0 + lane;
    const bool in = i < n && mask[base + i] != 0;
    const unsigned long long bal = __ballot(in);
    if (in) {
      const int64_t at = o + __popcll(bal & ((1ull << lane) - 1ull));
      if (out_a) {  // (nullable as a pair: the descriptor matcher compacts positions only)
        out_a[at] = uv_a[base + i];
        out_b[at] = uv_b[base + i];
      }
      if (out_index) out_index[at] = static_cast<int32_t>(base + i);
    }
    o += __popcll(bal);
  }
}

}  // namespace

// ptz_gate_compact.h: kept counts, scan, scatter of a byte mask over a CSR, on one stream
void enqueue_compact(int n_pair, const int64_t* d_ptr, const int32_t* d_found, const uint8_t* d_mask, int32_t need, int32_t* d_cnt,
                     int64_t* d_out_ptr, const float2* d_a, const float2* d_b, float2* d_out_a, float2* d_out_b, int32_t* d_out_index,
                     hipStream_t st, const int32_t* d_live)
{
  const int per = GATE_WG / WAVE;
  if (n_pair > 0)
    hipLaunchKernelGGL(k_gate_count, dim3((n_pair + per - 1) / per), dim3(GATE_WG), 0, st, n_pair, d_ptr, d_found, d_mask, need, d_cnt, d_live);
  hipLaunchKernelGGL(k_gate_scan, dim3(1), dim3(SCAN_WG), 0, st, n_pair, (const int32_t*)d_cnt, d_out_ptr, d_live);
  if (n_pair > 0)
    hipLaunchKernelGGL(k_gate_scatter, dim3((n_pair + per - 1) / per), dim3(GATE_WG), 0, st, n_pair, d_ptr, d_a, d_b, d_mask, (const int32_t*)d_cnt,
                       (const int64_t*)d_out_ptr, d_out_a, d_out_b, d_out_index, d_live);
}

namespace {

// The three stages on one stream, device pointers throughout: estimator (d_order = nullptr: pair order), kept counts, scan,
// scatter.  d_found of the pairs the estimator skips (k_gate_prepare's -1) is already written.
void enqueue_gate(int n_pair, const int64_t* d_ptr, const int32_t* d_order, const int64_t* d_boff, const int32_t* d_tab, const float* d_a,
                  const float* d_b, double thr, int32_t max_n, int64_t max_matches, int32_t min_inliers, double* d_H, int32_t* d_found,
                  uint8_t* d_mask, int32_t* d_inl, int32_t* d_cnt, int64_t* d_out_ptr, float* d_out_a, float* d_out_b,
                  int32_t* d_out_index, hipStream_t st)
{
  if (n_pair > 0)
    hipLaunchKernelGGL(k_homography_ransac, dim3(n_pair), dim3(HB), 0, st, d_ptr, d_order, d_a, d_b, thr * thr, d_boff, d_tab, d_H,
                       d_found, d_mask, d_inl, max_n, max_matches);
  enqueue_compact(n_pair, d_ptr, (const int32_t*)d_found, (const uint8_t*)d_mask, std::max(min_inliers, 4), d_cnt, d_out_ptr,
                  (const float2*)d_a, (const float2*)d_b, (float2*)d_out_a, (float2*)d_out_b, d_out_index, st);
}

// host side of the entries that read the offsets: the adaptive bound per distinct pair size (>= 5) and the launch order
// (largest pairs first)
void host_bounds_and_order(int n_pair, const int64_t* match_ptr, std::vector<int64_t>& boff, std::vector<int32_t>& tab,
                           std::vector<int32_t>& order)
{
  boff.assign(n_pair, 0);
  tab.clear();
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
  if (tab.empty()) tab.push_back(0);
  order.resize(n_pair);
  for (int p = 0; p < n_pair; ++p) order[p] = p;
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return match_ptr[a + 1] - match_ptr[a] > match_ptr[b + 1] - match_ptr[b]; });
}

// the gate's table: every size 5 .. max_n at gate_table_offset
void gate_table(int32_t max_n, std::vector<int32_t>& tab)
{
  tab.assign(static_cast<size_t>(std::max<int64_t>(gate_table_offset(static_cast<int64_t>(max_n) + 1), 1)), 0);
  for (int n = 5; n <= max_n; ++n) (void)ptz_debug_homography_bounds(n, tab.data() + gate_table_offset(n));
}

// the argument list the estimator's host entries share
int32_t check_csr(int32_t n_pair, const int64_t* match_ptr, const float* src_uv, const float* dst_uv, double ransac_thresh, int64_t& longest)
{
  if (n_pair < 0 || !(std::isfinite(ransac_thresh) && ransac_thresh > 0)) return PTZ_EINVAL;
  if (n_pair > 0 && !match_ptr) return PTZ_EINVAL;
  if (match_ptr && match_ptr[0] != 0) return PTZ_EINVAL;
  longest = 0;
  for (int p = 0; p < n_pair; ++p) {
    if (match_ptr[p + 1] < match_ptr[p]) return PTZ_EINVAL;
    longest = std::max<int64_t>(longest, match_ptr[p + 1] - match_ptr[p]);
  }
  const int64_t nm = n_pair > 0 ? match_ptr[n_pair] : 0;
  if (nm > 0 && (!src_uv || !dst_uv)) return PTZ_EINVAL;
  return PTZ_OK;
}

}  // namespace
}  // namespace ptz

extern "C" int32_t ptz_homography_ransac_batch(int32_t n_pair, const int64_t* match_ptr, const float* src_uv, const float* dst_uv,
                                               double ransac_thresh, int32_t device_id, double* H, int32_t* found,
                                               uint8_t* inlier_mask, double* device_ms)
{
  using namespace ptz;
  // validation first, device second
  int64_t longest = 0;
  if (const int32_t rc = check_csr(n_pair, match_ptr, src_uv, dst_uv, ransac_thresh, longest)) return rc;
  if (n_pair > 0 && (!H || !found)) return PTZ_EINVAL;
  const int64_t nm = n_pair > 0 ? match_ptr[n_pair] : 0;
  if (device_ms) *device_ms = 0;
  if (n_pair == 0) return PTZ_OK;
  if (longest > INT32_MAX) return PTZ_ELIMIT;
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);

  std::vector<int64_t> boff;
  std::vector<int32_t> tab, order;
  host_bounds_and_order(n_pair, match_ptr, boff, tab, order);

  const size_t nmx = nm > 0 ? (size_t)nm : 1;
  const size_t o_ptr = 0, o_ord = o_ptr + up256(sizeof(int64_t) * (n_pair + 1)), o_boff = o_ord + up256(sizeof(int32_t) * n_pair),
               o_tab = o_boff + up256(sizeof(int64_t) * n_pair), o_src = o_tab + up256(sizeof(int32_t) * tab.size()),
               o_dst = o_src + up256(sizeof(float) * 2 * nmx), o_H = o_dst + up256(sizeof(float) * 2 * nmx),
               o_found = o_H + up256(sizeof(double) * 9 * n_pair), o_mask = o_found + up256(sizeof(int32_t) * n_pair),
               o_inl = o_mask + up256(nmx), total = o_inl + up256(sizeof(int32_t) * nmx);
  CallHeld h;
  if (const int32_t rc = h.acquire(device_id, total)) return rc;
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
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  hipLaunchKernelGGL(k_homography_ransac, dim3(n_pair), dim3(HB), 0, h.st, (const int64_t*)(b + o_ptr), (const int32_t*)(b + o_ord),
                     (const float*)(b + o_src), (const float*)(b + o_dst), ransac_thresh * ransac_thresh,
                     (const int64_t*)(b + o_boff), (const int32_t*)(b + o_tab), (double*)(b + o_H), (int32_t*)(b + o_found), d_mask,
                     (int32_t*)(b + o_inl), INT32_MAX, nm);
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  std::vector<double> Hd(9 * (size_t)n_pair);
  std::vector<uint8_t> md(inlier_mask ? nmx : 0);
  PTZ_HIP_TRY(hipMemcpyAsync(Hd.data(), b + o_H, sizeof(double) * 9 * n_pair, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(found, b + o_found, sizeof(int32_t) * n_pair, hipMemcpyDeviceToHost, h.st));
  if (inlier_mask && nm > 0) PTZ_HIP_TRY(hipMemcpyAsync(md.data(), d_mask, nm, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  PTZ_HIP_TRY(hipGetLastError());
  if (device_ms) *device_ms = h.elapsed_ms();
  // H and mask of a pair that is not found stay untouched, as with the host estimator
  for (int p = 0; p < n_pair; ++p) {
    if (!found[p]) continue;
    memcpy(H + 9 * (size_t)p, Hd.data() + 9 * (size_t)p, sizeof(double) * 9);
    if (inlier_mask) memcpy(inlier_mask + match_ptr[p], md.data() + match_ptr[p], match_ptr[p + 1] - match_ptr[p]);
  }
  return PTZ_OK;
}

// ---- the match gate --------------------------------------------------------------------------------------------------------
struct ptz_match_gate {
  int device = 0;
  int32_t max_pairs = 0, max_pair_matches = 0;
  int64_t max_matches = 0;
  char* base = nullptr;  // one pooled block behind everything below
  int32_t* d_tab = nullptr;   // bound tables of the sizes 5 .. max_pair_matches
  int64_t* d_boff = nullptr;  // [max_pairs] table offset of a run's pairs
  int32_t* d_cnt = nullptr;   // [max_pairs] kept matches of a run's pairs
  int32_t* d_inl = nullptr;   // [max_matches] the estimator's inlier lists
  uint8_t* d_mask = nullptr;  // [max_matches] the mask of callers that ask for none
  double* d_H = nullptr;      // [9 max_pairs] likewise
};

extern "C" int32_t ptz_debug_match_gate_table(int32_t max_pair_matches, int32_t* table, int64_t* table_len, int64_t* offsets)
{
  using namespace ptz;
  if (max_pair_matches < 0 || !table_len) return PTZ_EINVAL;
  if (max_pair_matches > 4096) return PTZ_ELIMIT;
  *table_len = gate_table_offset(static_cast<int64_t>(max_pair_matches) + 1);
  if (offsets)
    for (int n = 0; n <= max_pair_matches; ++n) offsets[n] = gate_table_offset(n);
  if (table && *table_len > 0) {
    std::vector<int32_t> tab;
    gate_table(max_pair_matches, tab);
    memcpy(table, tab.data(), sizeof(int32_t) * (size_t)*table_len);
  }
  return PTZ_OK;
}

extern "C" int32_t ptz_match_gate_create(int32_t max_pairs, int64_t max_matches, int32_t max_pair_matches, int32_t device_id,
                                         ptz_match_gate** out)
{
  using namespace ptz;
  if (!out) return PTZ_EINVAL;
  *out = nullptr;
  if (max_pairs <= 0 || max_matches < 0 || max_pair_matches < 0 || device_id < 0) return PTZ_EINVAL;
  if (max_pair_matches > 4096 || max_matches > INT32_MAX) return PTZ_ELIMIT;  // the table grows with the square; out_index is int32
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);
  std::vector<int32_t> tab;
  gate_table(max_pair_matches, tab);
  const size_t nmx = (size_t)std::max<int64_t>(max_matches, 1);
  const size_t o_tab = 0, o_boff = o_tab + up256(sizeof(int32_t) * tab.size()), o_cnt = o_boff + up256(sizeof(int64_t) * max_pairs),
               o_inl = o_cnt + up256(sizeof(int32_t) * max_pairs), o_mask = o_inl + up256(sizeof(int32_t) * nmx), o_H = o_mask + up256(nmx),
               total = o_H + up256(sizeof(double) * 9 * max_pairs);
  std::unique_ptr<ptz_match_gate> g(new ptz_match_gate());
  g->device = device_id; g->max_pairs = max_pairs; g->max_matches = max_matches; g->max_pair_matches = max_pair_matches;
  void* blk = nullptr;
  if (ptzpool::dev_acquire(device_id, total, &blk) != hipSuccess) return PTZ_ENOMEM;
  g->base = static_cast<char*>(blk);
  g->d_tab = (int32_t*)(g->base + o_tab); g->d_boff = (int64_t*)(g->base + o_boff); g->d_cnt = (int32_t*)(g->base + o_cnt);
  g->d_inl = (int32_t*)(g->base + o_inl); g->d_mask = (uint8_t*)(g->base + o_mask); g->d_H = (double*)(g->base + o_H);
  hipStream_t st = nullptr;
  hipError_t e = ptzpool::stream_acquire(device_id, &st);
  if (e == hipSuccess) e = hipMemcpyAsync(g->d_tab, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = stream_wait(st);
  if (st) ptzpool::stream_release(device_id, st);
  if (e != hipSuccess) { (void)hipGetLastError(); ptzpool::dev_release(device_id, blk); return PTZ_ENODEVICE; }
  *out = g.release();
  return PTZ_OK;
}

extern "C" void ptz_match_gate_destroy(ptz_match_gate* g)
{
  if (!g) return;
  ptz::DeviceGuard guard(g->device);
  ptzpool::dev_release(g->device, g->base);
  delete g;
}

extern "C" int32_t ptz_match_gate_run_device(ptz_match_gate* g, int32_t n_pair, const int64_t* d_match_ptr, const float* d_uv_a,
                                             const float* d_uv_b, double ransac_thresh, int32_t min_inliers, double* d_H,
                                             int32_t* d_found, uint8_t* d_mask, int64_t* d_out_ptr, float* d_out_uv_a,
                                             float* d_out_uv_b, int32_t* d_out_index, void* hip_stream)
{
  using namespace ptz;
  if (!g || n_pair < 0 || !(std::isfinite(ransac_thresh) && ransac_thresh > 0) || min_inliers < 0 || !d_out_ptr) return PTZ_EINVAL;
  if (n_pair > 0 && (!d_match_ptr || !d_found)) return PTZ_EINVAL;
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
  if (n_pair > 0) {
    hipLaunchKernelGGL(k_gate_prepare, dim3((n_pair + 255) / 256), dim3(256), 0, st, n_pair, d_match_ptr, g->max_pair_matches,
                       g->max_matches, g->d_boff, d_found);
  }
  enqueue_gate(n_pair, d_match_ptr, nullptr, g->d_boff, g->d_tab, d_uv_a, d_uv_b, ransac_thresh, g->max_pair_matches, g->max_matches,
               min_inliers, d_H ? d_H : g->d_H, d_found, d_mask ? d_mask : g->d_mask, g->d_inl, g->d_cnt, d_out_ptr, d_out_uv_a,
               d_out_uv_b, d_out_index, st);
  PTZ_HIP_TRY(hipGetLastError());
  return PTZ_OK;
}

// the gate on HOST arrays: upload, ptz_match_gate_run_device, download (callers without device buffers of their own, tests)
extern "C" int32_t ptz_match_gate_run(ptz_match_gate* g, int32_t n_pair, const int64_t* match_ptr, const float* uv_a, const float* uv_b,
                                      double ransac_thresh, int32_t min_inliers, double* H, int32_t* found, uint8_t* mask,
                                      int64_t* out_ptr, float* out_uv_a, float* out_uv_b, int32_t* out_index, double* device_ms)
{
  using namespace ptz;
  int64_t longest = 0;
  if (!g) return PTZ_EINVAL;
  if (const int32_t rc = check_csr(n_pair, match_ptr, uv_a, uv_b, ransac_thresh, longest)) return rc;
  if (min_inliers < 0 || !out_ptr || (n_pair > 0 && !found)) return PTZ_EINVAL;
  const int64_t nm = n_pair > 0 ? match_ptr[n_pair] : 0;
  if (nm > 0 && (!out_uv_a || !out_uv_b)) return PTZ_EINVAL;
  if (n_pair > g->max_pairs || nm > g->max_matches) return PTZ_ELIMIT;
  if (device_ms) *device_ms = 0;
  clear_stale_error(__func__);
  PTZ_DEVICE_GUARD(g->device);
  const size_t nmx = nm > 0 ? (size_t)nm : 1, np1 = (size_t)n_pair + 1;
  const size_t o_ptr = 0, o_a = o_ptr + up256(sizeof(int64_t) * np1), o_b = o_a + up256(sizeof(float) * 2 * nmx),
               o_H = o_b + up256(sizeof(float) * 2 * nmx), o_found = o_H + up256(sizeof(double) * 9 * np1), o_mask = o_found + up256(sizeof(int32_t) * np1),
               o_optr = o_mask + up256(nmx), o_oa = o_optr + up256(sizeof(int64_t) * np1), o_ob = o_oa + up256(sizeof(float) * 2 * nmx),
               o_oi = o_ob + up256(sizeof(float) * 2 * nmx), total = o_oi + up256(sizeof(int32_t) * nmx);
  CallHeld h;
  if (const int32_t rc = h.acquire(g->device, total)) return rc;
  char* b = h.base;
  if (n_pair > 0) PTZ_HIP_TRY(hipMemcpyAsync(b + o_ptr, match_ptr, sizeof(int64_t) * np1, hipMemcpyHostToDevice, h.st));
  if (nm > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(b + o_a, uv_a, sizeof(float) * 2 * nm, hipMemcpyHostToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(b + o_b, uv_b, sizeof(float) * 2 * nm, hipMemcpyHostToDevice, h.st));
  }
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  if (const int32_t rc = ptz_match_gate_run_device(g, n_pair, (const int64_t*)(b + o_ptr), (const float*)(b + o_a), (const float*)(b + o_b),
                                                   ransac_thresh, min_inliers, (double*)(b + o_H), (int32_t*)(b + o_found),
                                                   (uint8_t*)(b + o_mask), (int64_t*)(b + o_optr), (float*)(b + o_oa), (float*)(b + o_ob),
                                                   (int32_t*)(b + o_oi), h.st))
    return rc;
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  std::vector<double> Hd(H ? 9 * (size_t)n_pair : 0);
  std::vector<uint8_t> md(mask ? nmx : 0);
  if (H && n_pair > 0) PTZ_HIP_TRY(hipMemcpyAsync(Hd.data(), b + o_H, sizeof(double) * 9 * n_pair, hipMemcpyDeviceToHost, h.st));
  if (n_pair > 0) PTZ_HIP_TRY(hipMemcpyAsync(found, b + o_found, sizeof(int32_t) * n_pair, hipMemcpyDeviceToHost, h.st));
  if (mask && nm > 0) PTZ_HIP_TRY(hipMemcpyAsync(md.data(), b + o_mask, nm, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(out_ptr, b + o_optr, sizeof(int64_t) * np1, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  PTZ_HIP_TRY(hipGetLastError());
  const int64_t kept = out_ptr[n_pair];
  if (kept < 0 || kept > nm) return PTZ_ENODEVICE;  // cannot happen: the scan of counts that are at most the pairs' sizes
  if (kept > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(out_uv_a, b + o_oa, sizeof(float) * 2 * kept, hipMemcpyDeviceToHost, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(out_uv_b, b + o_ob, sizeof(float) * 2 * kept, hipMemcpyDeviceToHost, h.st));
    if (out_index) PTZ_HIP_TRY(hipMemcpyAsync(out_index, b + o_oi, sizeof(int32_t) * kept, hipMemcpyDeviceToHost, h.st));
    PTZ_HIP_TRY(stream_wait(h.st));
  }
  if (device_ms) *device_ms = h.elapsed_ms();
  // H and mask of a pair without a model stay untouched, as with ptz_homography_ransac_batch
  for (int p = 0; p < n_pair; ++p) {
    if (found[p] != 1) continue;
    if (H) memcpy(H + 9 * (size_t)p, Hd.data() + 9 * (size_t)p, sizeof(double) * 9);
    if (mask) memcpy(mask + match_ptr[p], md.data() + match_ptr[p], match_ptr[p + 1] - match_ptr[p]);
  }
  return PTZ_OK;
}

extern "C" int32_t ptz_krt_solve_batch_gated(int32_t n_query, const int64_t* match_ptr, const float* uv_ref, const float* uv_cur,
                                             const double* cam_ref, double* cam_cur, int32_t factor_type, double max_reproj_error,
                                             double ransac_thresh, int32_t min_inliers, const ptz_lm_options* opt,
                                             ptz_lm_summary* summaries, int32_t* accepted, int32_t* n_inliers, uint8_t* inlier_mask,
                                             double* H, double* device_ms)
{
  using namespace ptz;
  int64_t longest = 0;
  if (const int32_t rc = check_csr(n_query, match_ptr, uv_ref, uv_cur, ransac_thresh, longest)) return rc;
  if (min_inliers < 0) return PTZ_EINVAL;
  if (n_query > 0 && (!cam_ref || !cam_cur || !summaries || !accepted || !n_inliers)) return PTZ_EINVAL;
  if (factor_type < PTZ_KRT_F || factor_type > PTZ_KRT_FxfyDist) return PTZ_EUNSUPPORTED;
  if (device_ms) device_ms[0] = device_ms[1] = 0;
  if (n_query == 0) return PTZ_OK;
  if (longest > INT32_MAX) return PTZ_ELIMIT;
  ptz_lm_options o;
  if (opt) o = *opt; else ptz_lm_options_default(&o);
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || o.device_id < 0 || ndev <= o.device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(o.device_id);
  const int64_t nm = match_ptr[n_query];
  std::vector<int64_t> boff;
  std::vector<int32_t> tab, order;
  host_bounds_and_order(n_query, match_ptr, boff, tab, order);

  // one pooled block: [offsets | order | table offsets | tables | pixels | H | found | mask | inlier lists | kept counts |
  //                    compacted CSR | cameras | summaries | accepted]
  const size_t nmx = nm > 0 ? (size_t)nm : 1, nq = (size_t)n_query;
  const size_t o_ptr = 0, o_ord = o_ptr + up256(sizeof(int64_t) * (nq + 1)), o_boff = o_ord + up256(sizeof(int32_t) * nq),
               o_tab = o_boff + up256(sizeof(int64_t) * nq), o_ref = o_tab + up256(sizeof(int32_t) * tab.size()),
               o_cur = o_ref + up256(sizeof(float) * 2 * nmx), o_H = o_cur + up256(sizeof(float) * 2 * nmx),
               o_found = o_H + up256(sizeof(double) * 9 * nq), o_mask = o_found + up256(sizeof(int32_t) * nq), o_inl = o_mask + up256(nmx),
               o_cnt = o_inl + up256(sizeof(int32_t) * nmx), o_optr = o_cnt + up256(sizeof(int32_t) * nq),
               o_oref = o_optr + up256(sizeof(int64_t) * (nq + 1)), o_ocur = o_oref + up256(sizeof(float) * 2 * nmx),
               o_cref = o_ocur + up256(sizeof(float) * 2 * nmx), o_ccur = o_cref + up256(sizeof(double) * 15 * nq),
               o_sum = o_ccur + up256(sizeof(double) * 15 * nq), o_acc = o_sum + up256(sizeof(ptz_lm_summary) * nq),
               total = o_acc + up256(sizeof(int32_t) * nq);
  CallHeld h;
  if (const int32_t rc = h.acquire(o.device_id, total)) return rc;
  PTZ_HIP_TRY(h.third_event());
  char* b = h.base;
  PTZ_HIP_TRY(hipMemcpyAsync(b + o_ptr, match_ptr, sizeof(int64_t) * (nq + 1), hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(b + o_ord, order.data(), sizeof(int32_t) * nq, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(b + o_boff, boff.data(), sizeof(int64_t) * nq, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(b + o_tab, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, h.st));
  if (nm > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(b + o_ref, uv_ref, sizeof(float) * 2 * nm, hipMemcpyHostToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(b + o_cur, uv_cur, sizeof(float) * 2 * nm, hipMemcpyHostToDevice, h.st));
  }
  PTZ_HIP_TRY(hipMemcpyAsync(b + o_cref, cam_ref, sizeof(double) * 15 * nq, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(b + o_ccur, cam_cur, sizeof(double) * 15 * nq, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  enqueue_gate(n_query, (const int64_t*)(b + o_ptr), (const int32_t*)(b + o_ord), (const int64_t*)(b + o_boff), (const int32_t*)(b + o_tab),
               (const float*)(b + o_ref), (const float*)(b + o_cur), ransac_thresh, INT32_MAX, nm, min_inliers, (double*)(b + o_H),
               (int32_t*)(b + o_found), (uint8_t*)(b + o_mask), (int32_t*)(b + o_inl), (int32_t*)(b + o_cnt), (int64_t*)(b + o_optr),
               (float*)(b + o_oref), (float*)(b + o_ocur), nullptr, h.st);
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  // the LM of ptz_krt_solve_batch on the compacted CSR: same launch path, same stream
  if (const int32_t rc = ptz_krt_solve_batch_device(n_query, (const int64_t*)(b + o_optr), (const float*)(b + o_oref), (const float*)(b + o_ocur),
                                                    nullptr, nullptr, nullptr, (const double*)(b + o_cref), (double*)(b + o_ccur), factor_type,
                                                    max_reproj_error, &o, (ptz_lm_summary*)(b + o_sum), (int32_t*)(b + o_acc), h.st))
    return rc;
  PTZ_HIP_TRY(hipEventRecord(h.ev[2], h.st));
  std::vector<double> Hd(H ? 9 * nq : 0);
  std::vector<int32_t> fd(nq);
  std::vector<uint8_t> md(inlier_mask ? nmx : 0);
  if (H) PTZ_HIP_TRY(hipMemcpyAsync(Hd.data(), b + o_H, sizeof(double) * 9 * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(fd.data(), b + o_found, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, h.st));
  if (inlier_mask && nm > 0) PTZ_HIP_TRY(hipMemcpyAsync(md.data(), b + o_mask, nm, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(n_inliers, b + o_cnt, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(cam_cur, b + o_ccur, sizeof(double) * 15 * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(summaries, b + o_sum, sizeof(ptz_lm_summary) * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(accepted, b + o_acc, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  PTZ_HIP_TRY(hipGetLastError());  // a refused kernel launch must not pass for a solve
  if (device_ms) { device_ms[0] = h.elapsed_ms(0); device_ms[1] = h.elapsed_ms(1); }
  // H of a query without a model stays untouched, as with ptz_homography_ransac_batch; inlier_mask is the KEPT set: the
  // estimator's mask of a query that passes, zeros for every other query
  for (int q = 0; q < n_query; ++q) {
    if (H && fd[q] == 1) memcpy(H + 9 * (size_t)q, Hd.data() + 9 * (size_t)q, sizeof(double) * 9);
    if (!inlier_mask) continue;
    const int64_t a = match_ptr[q], n = match_ptr[q + 1] - a;
    if (n_inliers[q] > 0) memcpy(inlier_mask + a, md.data() + a, n);
    else memset(inlier_mask + a, 0, n);
  }
  return PTZ_OK;
}
