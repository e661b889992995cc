// ptz_ba_resid.hip -- residual report of a bundle-adjustment batch and the trimming selection on MI355X (gfx950).  The kernels and
// their reduction shapes: ptz_ba_resid.h; the rule: ptz_ba_trim.h.  A streaming pass: every observation is evaluated once (thread
// per ray, like k_ba_cov_ray), its error kept in the library's order for the per-view and per-problem passes, which read it back
// from L2.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "ptz_common.h"
#include "ptz_pool.h"
#include "ptz_host_batch.h"
#include "ptz_ba_resid.h"

namespace ptz {

namespace {

struct ResidWork {
  // scratch
  double* camblk;   // [cameras][CAMBLK]
  double* tlwblk;   // [problems][TLWBLK]
  double* err_int;  // [observations] |e_o| in the library's order (global index)
  int* cstart;      // [rays] at ray_off + r: problem-local index of the first observation of the caller's ray r, caller's order
  // results, at the batch's offsets
  double *err, *rmax, *vrms, *vmax, *rms, *med, *rms3, *thr, *e3;
  int *rworst, *vcnt, *nrej;
  unsigned char* rej;
  const int* ray_perm;
  int want_median, select, has_o3;
  TrimRule rule;
};

__global__ void k_resid_cam(BaCovIn in, BaGeoIn geo, ResidWork w)
{
  const int g = blockIdx.y;
  const BaCovScene s = in.scene[g];
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && w.has_o3) ba_geo_tlwblk(geo.tlw_x + (size_t)s.cur * geo.tlw_stride + (size_t)s.idx * 6, w.tlwblk + (size_t)g * TLWBLK);
  if (c >= s.n_cam) return;
  const double* c15 = in.cam_x + (size_t)s.cur * in.cam_stride + (size_t)(s.cam_off + c) * 15;
  ba_cov_camblk(c15, w.camblk + (size_t)(s.cam_off + c) * CAMBLK);
}

// lengths of the caller's rays, then their exclusive prefix sum: thread t owns a contiguous chunk, the 256 chunk sums are scanned by
// one thread
__global__ __launch_bounds__(256) void k_resid_order(BaCovIn in, ResidWork w)
{
  const BaCovScene s = in.scene[blockIdx.x];
  const int* rp = in.ray_ptr + s.ray_off + s.idx;
  const int* perm = w.ray_perm + s.ray_off;
  int* cs = w.cstart + s.ray_off;
  const int tid = threadIdx.x;
  for (int j = tid; j < s.n_ray; j += 256) {
    const int r = perm[j];
    if (r >= 0 && r < s.n_ray) cs[r] = rp[j + 1] - rp[j];
  }
  __threadfence_block();
  __syncthreads();  // (the lengths this workgroup wrote are read back by it below)
  const int chunk = (s.n_ray + 255) / 256;
  const int lo = min(tid * chunk, s.n_ray), hi = min(lo + chunk, s.n_ray);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += cs[i];
  __shared__ int part[256];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < 256; ++t) { const int x = part[t]; part[t] = run; run += x; }
  }
  __syncthreads();
  int run = part[tid];
  for (int i = lo; i < hi; ++i) { const int x = cs[i]; cs[i] = run; run += x; }
}

template <int TYPE>
__global__ __launch_bounds__(256) void k_resid_ray(BaCovIn in, ResidWork w)
{
  const int g = blockIdx.y;
  const BaCovScene s = in.scene[g];
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= s.n_ray) return;  // (rays are sorted by length: the lanes of a wave that stays run about equally long)
  const int* rp = in.ray_ptr + s.ray_off + s.idx;
  const int a0 = rp[j], a1 = rp[j + 1];
  const int jc = w.ray_perm[s.ray_off + j];
  if (jc < 0 || jc >= s.n_ray) return;
  const int c0 = w.cstart[s.ray_off + jc];
  const double* xp = in.ray_x + (size_t)s.cur * in.ray_stride + (size_t)(s.ray_off + j) * 3;
  const double X[3] = {xp[0], xp[1], xp[2]};
  const double* cbs = w.camblk + (size_t)s.cam_off * CAMBLK;
  double mx = 0.0;
  int at = -1;
  for (int a = a0; a < a1; ++a) {
    const int k = c0 + (a - a0);  // the observation's index in the caller's order
    if (a < s.obs_off || a >= s.obs_off + s.n_obs || k < 0 || k >= s.n_obs) continue;
    const float2 uv = in.obs_uv[a];
    double res[2];
    ba_residual<TYPE>(cbs + (size_t)in.obs_cam[a] * CAMBLK, X, uv.x, uv.y, res);
    const double e = sqrt(res[0] * res[0] + res[1] * res[1]);
    w.err_int[a] = e;
    w.err[(size_t)s.obs_off + k] = e;
    if (at < 0 || e > mx) { mx = e; at = k; }  // (the first on a tie)
  }
  w.rmax[s.ray_off + jc] = mx;
  w.rworst[s.ray_off + jc] = at;
}

__global__ __launch_bounds__(64) void k_resid_view(BaCovIn in, ResidWork w)
{
  const int g = blockIdx.y, c = blockIdx.x;
  const BaCovScene s = in.scene[g];
  if (c >= s.n_cam) return;
  const int* cp = in.cam_ptr + s.cam_off + s.idx;
  const int o0 = cp[c], no = cp[c + 1] - o0;
  double ss = 0, mx = 0;
  for (int q = threadIdx.x; q < no; q += 64) {
    const double e = w.err_int[in.cam_obs[o0 + q]];
    ss += e * e;
    mx = fmax(mx, e);
  }
  ss = wave_sum(ss);
  mx = wave_max(mx);
  if (threadIdx.x != 0) return;
  w.vrms[s.cam_off + c] = no > 0 ? sqrt(ss / (double)no) : 0.0;
  w.vmax[s.cam_off + c] = mx;
  w.vcnt[s.cam_off + c] = no;
}

template <int TYPE>
__global__ __launch_bounds__(256) void k_resid_annot(BaCovIn in, BaGeoIn geo, ResidWork w)
{
  const int g = blockIdx.y;
  const BaCovScene s = in.scene[g];
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= s.n_o3) return;
  const size_t ga = (size_t)s.o3_off + a;
  const int c = geo.o3_cam[ga];
  if (c < 0 || c >= s.n_cam) return;
  const float2 uv = geo.o3_uv[ga];
  const double xyz[3] = {geo.o3_xyz[3 * ga], geo.o3_xyz[3 * ga + 1], geo.o3_xyz[3 * ga + 2]};
  constexpr int F3 = TYPE ? 1 : 0;
  double res[2], Jc[2][5 + F3], Jt[2][6];
  reproj2d3d_eval<F3, false>(w.camblk + (size_t)(s.cam_off + c) * CAMBLK, w.tlwblk + (size_t)g * TLWBLK, xyz, uv.x, uv.y, res, Jc, Jt);
  w.e3[ga] = sqrt(res[0] * res[0] + res[1] * res[1]);
}

constexpr int PROBLEM_BLOCK = 1024;  // threads of k_resid_problem: its sums take observations t, t + 1024, ..

__global__ __launch_bounds__(PROBLEM_BLOCK) void k_resid_problem(BaCovIn in, ResidWork w)
{
  constexpr int NT = PROBLEM_BLOCK;
  const int g = blockIdx.x, tid = threadIdx.x;
  const BaCovScene s = in.scene[g];
  __shared__ double scratch[16];
  __shared__ unsigned hist[256];
  __shared__ unsigned s_k;
  __shared__ int s_bin, s_cnt;
  __shared__ unsigned long long s_kmin, s_kmax;
  const double* e = w.err_int + s.obs_off;
  const int n = s.n_obs;
  double ss = 0;
  for (int i = tid; i < n; i += NT) ss += e[i] * e[i];
  ss = block_sum(ss, scratch);
  if (tid == 0) w.rms[g] = n > 0 ? sqrt(ss / (double)n) : nan("");
  double s3 = 0;
  if (w.has_o3)
    for (int i = tid; i < s.n_o3; i += NT) { const double v = w.e3[(size_t)s.o3_off + i]; s3 += v * v; }
  s3 = block_sum(s3, scratch);
  if (tid == 0) w.rms3[g] = (w.has_o3 && s.n_o3 > 0) ? sqrt(s3 / (double)s.n_o3) : nan("");
  // the exact lower median: the errors are non-negative doubles, whose bit patterns order like the values; the pattern of element
  // (n - 1) / 2 of the sorted list is fixed byte by byte from the top, each pass counting the candidates that share the prefix.
  // The leading bytes that the smallest and the largest pattern share are every element's: those passes are not counted.
  double med = nan("");
  if (w.want_median && n > 0) {
    const unsigned long long kabs = 0x7fffffffffffffffull;
    if (tid == 0) { s_kmin = ~0ull; s_kmax = 0ull; }
    __syncthreads();
    unsigned long long lo = ~0ull, hi = 0ull;
    for (int i = tid; i < n; i += NT) {
      const unsigned long long key = (unsigned long long)__double_as_longlong(e[i]) & kabs;
      lo = key < lo ? key : lo;
      hi = key > hi ? key : hi;
    }
    if (tid < n) { atomicMin(&s_kmin, lo); atomicMax(&s_kmax, hi); }
    __syncthreads();
    const unsigned long long kmin = s_kmin, kdiff = s_kmin ^ s_kmax;
    unsigned long long prefix = 0;
    unsigned k = (unsigned)trim_median_index(n);
    bool all_share = true;  // every element still carries the prefix
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (all_share && (kdiff >> shift) == 0) {
        prefix |= kmin & (0xffull << shift);
        continue;
      }
      all_share = false;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      const unsigned long long himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
      for (int i = tid; i < n; i += NT) {
        const unsigned long long key = (unsigned long long)__double_as_longlong(e[i]) & kabs;
        if ((key & himask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        unsigned cum = 0;
        int bn = 0;
        for (; bn < 255; ++bn) {
          if (cum + hist[bn] > k) break;
          cum += hist[bn];
        }
        s_k = k - cum; s_bin = bn;
      }
      __syncthreads();
      k = s_k;
      prefix |= (unsigned long long)s_bin << shift;
      __syncthreads();
    }
    med = __longlong_as_double((long long)prefix);
  }
  if (tid == 0) w.med[g] = med;
  if (!w.select) return;
  const double t = trim_threshold(w.rule, med);
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (int r = tid; r < s.n_ray; r += NT) {
    const int at = w.rworst[s.ray_off + r];
    if (at >= 0 && at < n && trim_rejects(w.rmax[s.ray_off + r], t)) {
      w.rej[(size_t)s.obs_off + at] = 1;
      atomicAdd(&s_cnt, 1);
    }
  }
  __syncthreads();
  if (tid == 0) { w.thr[g] = t; w.nrej[g] = s_cnt; }
}

}  // namespace

int ba_resid_run(const BaCovIn& in, const BaGeoIn& geo, const BaCovScene* hs, const int* ray_perm, hipStream_t st, const BaResidOut& out,
                 double* device_ms)
{
  if (ba_cov_dim(in.type) < 0) return PTZ_EUNSUPPORTED;
  const int n = in.n_scene;
  // the batch's extents (a view batch keeps its arrays at upper bounds: offsets are the batch's, counts the real ones)
  size_t TC = 0, TR = 0, TO = 0, T3 = 0;
  int max_cam = 0, max_ray = 0, max_o3 = 0;
  for (int i = 0; i < n; ++i) {
    TC = std::max(TC, (size_t)hs[i].cam_off + hs[i].n_cam); TR = std::max(TR, (size_t)hs[i].ray_off + hs[i].n_ray);
    TO = std::max(TO, (size_t)hs[i].obs_off + hs[i].n_obs);
    max_cam = std::max(max_cam, hs[i].n_cam); max_ray = std::max(max_ray, hs[i].n_ray);
    if (geo.tlw_x) { T3 = std::max(T3, (size_t)hs[i].o3_off + hs[i].n_o3); max_o3 = std::max(max_o3, hs[i].n_o3); }
  }
  // one block: results first (they come back in one copy), scratch behind
  size_t o = 0;
  auto take = [&o](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
  const size_t D = sizeof(double), I = sizeof(int);
  const size_t o_err = take(D * TO), o_rmax = take(D * TR), o_vrms = take(D * TC), o_vmax = take(D * TC), o_rms = take(D * n), o_med = take(D * n),
               o_rms3 = take(D * n), o_thr = take(D * n), o_e3 = take(D * T3), o_rworst = take(I * TR), o_vcnt = take(I * TC), o_nrej = take(I * n),
               o_rej = take(TO);
  const size_t result_bytes = o;
  const size_t o_camblk = take(D * TC * CAMBLK), o_tlw = take(D * (size_t)n * TLWBLK), o_eint = take(D * TO), o_cstart = take(I * TR);
  CallHeld h(st);
  if (const int rc = h.acquire(in.device, std::max<size_t>(o, 256))) {
    if (rc == PTZ_ENOMEM) (void)hipGetLastError();
    return rc;
  }
  char* base = h.base;
  ResidWork w;
  auto dp = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
  auto ip = [&](size_t off) { return reinterpret_cast<int*>(base + off); };
  w.err = dp(o_err); w.rmax = dp(o_rmax); w.vrms = dp(o_vrms); w.vmax = dp(o_vmax); w.rms = dp(o_rms); w.med = dp(o_med); w.rms3 = dp(o_rms3);
  w.thr = dp(o_thr); w.e3 = dp(o_e3); w.rworst = ip(o_rworst); w.vcnt = ip(o_vcnt); w.nrej = ip(o_nrej);
  w.rej = reinterpret_cast<unsigned char*>(base + o_rej);
  w.camblk = dp(o_camblk); w.tlwblk = dp(o_tlw); w.err_int = dp(o_eint); w.cstart = ip(o_cstart);
  w.ray_perm = ray_perm;
  w.select = out.select ? 1 : 0;
  w.rule = out.rule;
  w.want_median = (out.median || (out.select && trim_needs_median(out.rule))) ? 1 : 0;
  w.has_o3 = (geo.tlw_x && T3 > 0) ? 1 : 0;
  PTZ_HIP_TRY(hipMemsetAsync(base, 0, o, st));
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], st));
  if (n > 0 && TO > 0) {
    hipLaunchKernelGGL(k_resid_cam, dim3((max_cam + 63) / 64, n), dim3(64), 0, st, in, geo, w);
    hipLaunchKernelGGL(k_resid_order, dim3(n), dim3(256), 0, st, in, w);
    const dim3 gr((max_ray + 255) / 256, n);
    if (in.type == 0) hipLaunchKernelGGL(k_resid_ray<0>, gr, dim3(256), 0, st, in, w);
    else if (in.type == 1) hipLaunchKernelGGL(k_resid_ray<1>, gr, dim3(256), 0, st, in, w);
    else hipLaunchKernelGGL(k_resid_ray<2>, gr, dim3(256), 0, st, in, w);
    hipLaunchKernelGGL(k_resid_view, dim3(max_cam, n), dim3(64), 0, st, in, w);
    if (w.has_o3 && max_o3 > 0) {
      const dim3 ga((max_o3 + 255) / 256, n);
      if (in.type == 0) hipLaunchKernelGGL(k_resid_annot<0>, ga, dim3(256), 0, st, in, geo, w);
      else if (in.type == 1) hipLaunchKernelGGL(k_resid_annot<1>, ga, dim3(256), 0, st, in, geo, w);
      else hipLaunchKernelGGL(k_resid_annot<2>, ga, dim3(256), 0, st, in, geo, w);
    }
    hipLaunchKernelGGL(k_resid_problem, dim3(n), dim3(PROBLEM_BLOCK), 0, st, in, w);
  }
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], st));
  std::vector<char> hb(result_bytes);
  PTZ_HIP_TRY(hipMemcpyAsync(hb.data(), base, result_bytes, hipMemcpyDeviceToHost, st));
  PTZ_HIP_TRY(stream_wait(st));
  PTZ_HIP_TRY(hipGetLastError());  // a refused kernel launch must not pass for a result
  if (device_ms) *device_ms = h.elapsed_ms();
  // to the caller's arrays: concatenated at the real extents
  auto hd = [&](size_t off) { return reinterpret_cast<const double*>(hb.data() + off); };
  auto hi = [&](size_t off) { return reinterpret_cast<const int*>(hb.data() + off); };
  size_t co = 0, cr = 0, cc = 0, c3 = 0;
  for (int i = 0; i < n; ++i) {
    const BaCovScene& s = hs[i];
    if (out.err_px) memcpy(out.err_px + co, hd(o_err) + s.obs_off, D * s.n_obs);
    if (out.reject) memcpy(out.reject + co, hb.data() + o_rej + s.obs_off, (size_t)s.n_obs);
    if (out.ray_max) memcpy(out.ray_max + cr, hd(o_rmax) + s.ray_off, D * s.n_ray);
    if (out.ray_worst) memcpy(out.ray_worst + cr, hi(o_rworst) + s.ray_off, I * s.n_ray);
    if (out.view_rms) memcpy(out.view_rms + cc, hd(o_vrms) + s.cam_off, D * s.n_cam);
    if (out.view_max) memcpy(out.view_max + cc, hd(o_vmax) + s.cam_off, D * s.n_cam);
    if (out.view_count) memcpy(out.view_count + cc, hi(o_vcnt) + s.cam_off, I * s.n_cam);
    if (out.rms) out.rms[i] = hd(o_rms)[i];
    if (out.median) out.median[i] = hd(o_med)[i];
    if (out.rms3d) out.rms3d[i] = w.has_o3 ? hd(o_rms3)[i] : std::numeric_limits<double>::quiet_NaN();
    if (out.threshold) out.threshold[i] = hd(o_thr)[i];
    if (out.n_reject) out.n_reject[i] = hi(o_nrej)[i];
    if (out.err3d_px && w.has_o3 && s.n_o3 > 0) memcpy(out.err3d_px + c3, hd(o_e3) + s.o3_off, D * s.n_o3);
    co += s.n_obs; cr += s.n_ray; cc += s.n_cam;
    if (w.has_o3) c3 += s.n_o3;
  }
  return PTZ_OK;
}

}  // namespace ptz
