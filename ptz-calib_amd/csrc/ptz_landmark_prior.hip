// ptz_landmark_prior.hip -- the landmark view on the device (gfx950): which landmarks of a map each query sees under its prior
// camera, and their packed descriptor rows gathered into a transient ptz_desc_set the guided matcher runs on as on any set.  The
// contract is ptz_landmark_prior.h (first include: its fp contract(off) must precede ptz_factor.h); this file adds the launch
// shapes and the C-ABI, nothing the result depends on.
//
//   k_landmark_visible<false>  a workgroup is one (query, tile of 1024 landmarks): four waves, each four steps of 64 consecutive
//                              landmarks, the rays read as one stream (the map's 24 bytes a landmark stay in L2 across queries).
//                              A wave counts its ballots; the workgroup writes one count per (query, tile).
//   k_landmark_view_scan, k_landmark_view_ptr   the scans of the counts to vis_ptr (ptz_landmark_view_kernels.h, shared with the
//                              view from homes of ptz_landmark_shortlist.hip)
//   k_landmark_visible<true>   recomputes the predicate and scatters vis_lm / vis_uv at vis_ptr[q] + tile offset + the counts of
//                              the waves and steps before + the ballot's prefix: ascending landmark index with no atomics, and the
//                              bits do not depend on the launch shape
//   k_landmark_view_rows       (the same header) gathers the packed rows and norms of the visible landmarks into the view's set
//
// No atomics, no scratch.  A query's outputs depend on its own prior and the map only.
#include "ptz_landmark_prior.h"

#include <memory>

#include "ptz_common.h"
#include "ptz_desc_set.h"
#include "ptz_host_batch.h"
#include "ptz_landmark_map.h"
#include "ptz_landmark_view_kernels.h"

namespace ptz {
namespace {

struct LvIn {
  int n_lm, n_query, n_tile, factor_type;
  double radius;
  const double *ray, *cams, *R;
  const int32_t* wh;
};

// blockIdx.x = q * n_tile + tile.  SCATTER = false: cnt[blockIdx.x] = the visible landmarks of the tile.  SCATTER = true: cnt holds
// the tile's offset inside its query, vis_ptr the query's; entries at or beyond `capacity` are not written.
template <bool SCATTER>
__global__ __launch_bounds__(LV_WG) void k_landmark_visible(LvIn a, int32_t* __restrict__ cnt, const int64_t* __restrict__ vis_ptr,
                                                            int32_t* __restrict__ vis_lm, float2* __restrict__ vis_uv, int64_t capacity)
{
  __shared__ int32_t s_cnt[LV_WAVES];
  const int q = blockIdx.x / a.n_tile, tile = blockIdx.x % a.n_tile;
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int32_t w = a.wh[2 * q], h = a.wh[2 * q + 1];
  double K4[4], R[9];
  prior_query_K(a.cams + 15 * (int64_t)q, w, h, a.factor_type, K4);
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = a.R[9 * (int64_t)q + k];
  const int base = tile * LV_TILE + wave * (LV_STEPS * WAVE);
  unsigned long long m[LV_STEPS];
  float2 uv[LV_STEPS];
  int n = 0;
#pragma unroll
  for (int s = 0; s < LV_STEPS; ++s) {
    const int l = base + s * WAVE + lane;
    bool vis = false;
    uv[s] = make_float2(0.f, 0.f);
    if (l < a.n_lm) {
      const double L[3] = {a.ray[3 * (int64_t)l], a.ray[3 * (int64_t)l + 1], a.ray[3 * (int64_t)l + 2]};
      const LandmarkSeen p = landmark_predict(K4, R, w, h, a.radius, L);
      vis = p.visible;
      uv[s] = make_float2(p.u, p.v);
    }
    m[s] = __ballot(vis);
    n += __popcll(m[s]);
  }
  if (lane == 0) s_cnt[wave] = n;
  __syncthreads();
  if (!SCATTER) {
    if (threadIdx.x == 0) {
      int32_t t = 0;
#pragma unroll
      for (int k = 0; k < LV_WAVES; ++k) t += s_cnt[k];
      cnt[blockIdx.x] = t;
    }
    return;
  }
  int64_t o = vis_ptr[q] + cnt[blockIdx.x];
  for (int k = 0; k < wave; ++k) o += s_cnt[k];
  const unsigned long long below = lane ? (~0ull >> (WAVE - lane)) : 0ull;
#pragma unroll
  for (int s = 0; s < LV_STEPS; ++s) {
    if ((m[s] >> lane) & 1ull) {
      const int64_t at = o + __popcll(m[s] & below);
      if (at >= 0 && at < capacity) {
        vis_lm[at] = base + s * WAVE + lane;
        vis_uv[at] = uv[s];
      }
    }
    o += __popcll(m[s]);
  }
}

bool lv_known_factor(int32_t t) { return t >= PTZ_KRT_F && t <= PTZ_KRT_FxfyDist; }

LvIn lv_in(int n_lm, const double* d_ray, int n_query, const double* d_cams, const double* d_R, const int32_t* d_wh, int factor_type, double radius)
{
  return LvIn{n_lm, n_query, lv_tiles(n_lm), factor_type, radius, d_ray, d_cams, d_R, d_wh};
}

// pass 1 and the two scans: d_vis_ptr complete
void enqueue_lv_count(const LvIn& a, int64_t* d_vis_ptr, char* ws, hipStream_t st)
{
  const LvWork w(a.n_lm, a.n_query);
  int32_t* cnt = (int32_t*)(ws + w.cnt);
  if (a.n_query > 0 && a.n_tile > 0)
    hipLaunchKernelGGL(k_landmark_visible<false>, dim3((unsigned)(a.n_query * a.n_tile)), dim3(LV_WG), 0, st, a, cnt, (const int64_t*)nullptr,
                       (int32_t*)nullptr, (float2*)nullptr, (int64_t)0);
  lv_enqueue_scans(a.n_lm, a.n_query, d_vis_ptr, ws, st);
}

// pass 2, after enqueue_lv_count on the same workspace
void enqueue_lv_scatter(const LvIn& a, const int64_t* d_vis_ptr, int32_t* d_vis_lm, float* d_vis_uv, int64_t capacity, char* ws, hipStream_t st)
{
  const LvWork w(a.n_lm, a.n_query);
  if (a.n_query > 0 && a.n_tile > 0 && capacity > 0)
    hipLaunchKernelGGL(k_landmark_visible<true>, dim3((unsigned)(a.n_query * a.n_tile)), dim3(LV_WG), 0, st, a, (int32_t*)(ws + w.cnt), d_vis_ptr,
                       d_vis_lm, (float2*)d_vis_uv, capacity);
}

}  // namespace
}  // namespace ptz

extern "C" void ptz_landmark_prior_options_default(ptz_landmark_prior_options* o)
{
  if (!o) return;
  o->radius_px = 40.0;
  o->max_view_bytes = (int64_t)2 << 30;
}

extern "C" void ptz_landmark_view_destroy(ptz_landmark_view* v)
{
  if (!v) return;
  ptz::DeviceGuard g(v->device);
  ptz_desc_set_destroy(v->set);
  delete v;
}

extern "C" int64_t ptz_landmark_view_n_visible(const ptz_landmark_view* v) { return v ? v->n_vis : 0; }

extern "C" const ptz_desc_set* ptz_landmark_view_desc_set(const ptz_landmark_view* v) { return v ? v->set : nullptr; }

extern "C" double ptz_landmark_view_device_ms(const ptz_landmark_view* v) { return v ? v->device_ms : 0.0; }

extern "C" int32_t ptz_landmark_view_device_ptrs(const ptz_landmark_view* v, const int64_t** d_vis_ptr, const int32_t** d_vis_lm,
                                                 const float** d_vis_uv)
{
  if (!v) return PTZ_EINVAL;
  if (d_vis_ptr) *d_vis_ptr = v->d_vis_ptr;
  if (d_vis_lm) *d_vis_lm = v->d_vis_lm;
  if (d_vis_uv) *d_vis_uv = v->d_vis_uv;
  return PTZ_OK;
}

extern "C" int32_t ptz_landmark_view_download(const ptz_landmark_view* v, int64_t* vis_ptr, int32_t* vis_lm, float* vis_uv)
{
  using namespace ptz;
  if (!v) return PTZ_EINVAL;
  if (vis_ptr) memcpy(vis_ptr, v->vis_ptr.data(), sizeof(int64_t) * v->vis_ptr.size());
  if (v->n_vis == 0 || (!vis_lm && !vis_uv)) return PTZ_OK;
  PTZ_DEVICE_GUARD(v->device);
  CallHeld h;
  if (const int32_t rc = h.open(v->device)) return rc;
  if (vis_lm) PTZ_HIP_TRY(hipMemcpyAsync(vis_lm, v->d_vis_lm, sizeof(int32_t) * (size_t)v->n_vis, hipMemcpyDeviceToHost, h.st));
  if (vis_uv) PTZ_HIP_TRY(hipMemcpyAsync(vis_uv, v->d_vis_uv, sizeof(float) * 2 * (size_t)v->n_vis, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  return PTZ_OK;
}

extern "C" int64_t ptz_landmark_visible_workspace_bytes(int32_t n_lm, int32_t n_query)
{
  if (n_lm < 0 || n_query < 0 || !ptz::lv_fits(n_lm, n_query)) return 0;
  return (int64_t)ptz::LvWork(n_lm, n_query).total;
}

extern "C" int32_t ptz_landmark_visible_device(int32_t n_lm, const double* d_ray, int32_t n_query, const double* d_prior_cams,
                                               const double* d_prior_R, const int32_t* d_query_wh, int32_t factor_type, double radius_px,
                                               int64_t* d_vis_ptr, int32_t* d_vis_lm, float* d_vis_uv, int64_t capacity, void* d_workspace,
                                               int64_t workspace_bytes, void* hip_stream)
{
  using namespace ptz;
  if (n_lm < 0 || n_query < 0 || capacity < 0 || !d_vis_ptr || !d_workspace) return PTZ_EINVAL;
  if (!(std::isfinite(radius_px) && radius_px > 0)) return PTZ_EINVAL;
  if (n_lm > 0 && !d_ray) return PTZ_EINVAL;
  if (n_query > 0 && (!d_prior_cams || !d_prior_R || !d_query_wh)) return PTZ_EINVAL;
  if (capacity > 0 && (!d_vis_lm || !d_vis_uv)) return PTZ_EINVAL;
  if (!lv_known_factor(factor_type)) return PTZ_EUNSUPPORTED;
  if (!lv_fits(n_lm, n_query)) return PTZ_ELIMIT;
  if (((uintptr_t)d_workspace & 255) != 0 || workspace_bytes < ptz_landmark_visible_workspace_bytes(n_lm, n_query)) return PTZ_EINVAL;
  clear_stale_error(__func__);
  int device = -1;
  if (const int rc = owning_device(d_vis_ptr, hip_stream, &device)) return rc;
  PTZ_DEVICE_GUARD(device);
  const LvIn a = lv_in(n_lm, d_ray, n_query, d_prior_cams, d_prior_R, d_query_wh, factor_type, radius_px);
  enqueue_lv_count(a, d_vis_ptr, (char*)d_workspace, (hipStream_t)hip_stream);
  enqueue_lv_scatter(a, d_vis_ptr, d_vis_lm, d_vis_uv, capacity, (char*)d_workspace, (hipStream_t)hip_stream);
  PTZ_HIP_TRY(hipGetLastError());
  return PTZ_OK;
}

extern "C" int32_t ptz_landmark_visible(const ptz_landmark_map* map, int32_t n_query, const double* prior_cams, const double* prior_R,
                                        const int32_t* query_wh, int32_t factor_type, const ptz_landmark_prior_options* opt,
                                        ptz_landmark_view** out)
{
  using namespace ptz;
  if (!out) return PTZ_EINVAL;
  *out = nullptr;
  // validation first, device second
  ptz_landmark_prior_options o;
  ptz_landmark_prior_options_default(&o);
  if (opt) o = *opt;
  if (!map || !map->set || n_query < 0 || (n_query > 0 && (!prior_cams || !prior_R || !query_wh))) return PTZ_EINVAL;
  for (int q = 0; q < n_query; ++q)
    if (query_wh[2 * q] <= 0 || query_wh[2 * q + 1] <= 0) return PTZ_EINVAL;
  if (prior_cams_check(n_query, prior_cams)) return PTZ_EINVAL;
  for (size_t k = 0; k < 9 * (size_t)n_query; ++k)
    if (!std::isfinite(prior_R[k])) return PTZ_EINVAL;
  if (!(std::isfinite(o.radius_px) && o.radius_px > 0) || o.max_view_bytes < 1) return PTZ_EINVAL;
  if (!lv_known_factor(factor_type)) return PTZ_EUNSUPPORTED;
  if (!lv_fits(map->n_lm, n_query)) return PTZ_ELIMIT;
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= map->device) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(map->device);

  struct Free { void operator()(ptz_landmark_view* v) const { ptz_landmark_view_destroy(v); } };
  std::unique_ptr<ptz_landmark_view, Free> view(new ptz_landmark_view());
  view->device = map->device; view->n_query = n_query; view->n_lm = map->n_lm;
  view->vis_ptr.assign((size_t)n_query + 1, 0);
  view->set = new ptz_desc_set();
  ptz_desc_set* s = view->set;
  s->device = map->device; s->n_img = n_query; s->D = map->D; s->KS = map->set->KS;
  const size_t nq = (size_t)n_query, nq1 = nq ? nq : 1;
  BlockLayout vb;
  const size_t o_pc = vb.take(sizeof(double) * 15 * nq1), o_H = vb.take(sizeof(double) * 9 * nq1), o_vp = vb.take(sizeof(int64_t) * (nq + 1));
  if (view->blk.get(map->device, vb.total()) != hipSuccess) { (void)hipGetLastError(); return PTZ_ENOMEM; }
  view->d_prior_cams = (const double*)(view->blk.p + o_pc);
  view->d_H = (const double*)(view->blk.p + o_H);
  view->d_vis_ptr = (const int64_t*)(view->blk.p + o_vp);

  // pass 1: the counts, the scans, and the one read that sizes the set
  BlockLayout tb;
  const size_t o_R = tb.take(sizeof(double) * 9 * nq1), o_wh = tb.take(sizeof(int32_t) * 2 * nq1),
               o_ws = tb.take(LvWork(map->n_lm, n_query).total);
  LvTables tables;  // (uploaded from: outlives the wait of h)
  CallHeld h;  // (declared after the view: the stream is waited for before a view that is not returned gives its blocks back)
  if (const int32_t rc = h.acquire(map->device, tb.total())) { (void)hipGetLastError(); return rc; }
  char* d = h.base;
  std::vector<double> H(9 * nq1, 0.0);
  for (size_t q = 0; q < nq; ++q) H[9 * q] = H[9 * q + 4] = H[9 * q + 8] = 1.0;
  if (n_query > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(view->blk.p + o_pc, prior_cams, sizeof(double) * 15 * nq, hipMemcpyHostToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(view->blk.p + o_H, H.data(), sizeof(double) * 9 * nq, hipMemcpyHostToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_R, prior_R, sizeof(double) * 9 * nq, hipMemcpyHostToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_wh, query_wh, sizeof(int32_t) * 2 * nq, hipMemcpyHostToDevice, h.st));
  }
  const LvIn a = lv_in(map->n_lm, map->d_ray, n_query, view->d_prior_cams, (const double*)(d + o_R), (const int32_t*)(d + o_wh), factor_type,
                       o.radius_px);
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  enqueue_lv_count(a, (int64_t*)(view->blk.p + o_vp), d + o_ws, h.st);
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(view->vis_ptr.data(), view->d_vis_ptr, sizeof(int64_t) * (nq + 1), hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  view->device_ms = h.elapsed_ms();
  // the set's host tables, its size against the caller's bound, its block
  if (const int32_t rc = lv_size_set(view.get(), map, o.max_view_bytes, &tables, h.st)) return rc;
  const int64_t n_vis = view->n_vis;
  view->d_vis_uv = (const float*)s->d_kp;

  // pass 2: the scatter, then the rows
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  enqueue_lv_scatter(a, view->d_vis_ptr, (int32_t*)view->d_vis_lm, (float*)s->d_kp, n_vis, d + o_ws, h.st);
  lv_enqueue_rows(view.get(), map, h.st);
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  view->device_ms += h.elapsed_ms();
  *out = view.release();
  return PTZ_OK;
}
