// ptz_landmark_shortlist.hip -- the landmark shortlist on the device (gfx950): the map's landmarks grouped by home as a descriptor
// set of n_ref images, the vote pass over it, and the view of the landmarks whose home is on a query's list, gathered into a
// transient ptz_desc_set the dense matcher runs on as on any set.  The contract is ptz_landmark_shortlist.h, all integer; this
// file adds the launch shapes and the C-ABI, nothing the result depends on.
//
//   home set                    built on the host from the map's own copies (a counting sort by home and ptz_desc_set_create: the
//                               packing stays where it is), on the first request, under the map's mutex
//   votes                       ptz_desc_shortlist[_device] with the home set as the reference set: k_desc_votes and
//                               k_desc_shortlist as they are
//   k_landmark_home_view<false> a workgroup is one (query, tile of 1024 landmarks), the shape of k_landmark_visible.  Thread w first
//                               builds word w of the query's bitmap over homes from its list (at most 8192 homes: 256 words, 1 KiB
//                               of LDS; the list entries are read at one address by all lanes); then four waves take four steps of
//                               64 consecutive landmarks each: d_home as one coalesced int32 stream (4 bytes a landmark, L2-resident
//                               across queries), one LDS word per lane -- neighbouring landmarks mostly share a home, so the reads
//                               of a wave fall on few words -- a ballot, a popcount.  One count per (query, tile).
//   k_landmark_view_scan / _ptr / _rows   ptz_landmark_view_kernels.h, shared with the prior's view
//   k_landmark_home_view<true>  rebuilds the bitmap, recomputes the predicate and scatters vis_lm at vis_ptr[q] + tile offset + the
//                               counts of the waves and steps before + the ballot's prefix: ascending landmark index
//
// No atomics, no scratch.  A query's outputs depend on its own list and the map only, not on the launch shape or its neighbours.
#include "ptz_landmark_shortlist.h"

#include <memory>
#include <mutex>
#include <optional>

#include "ptz_common.h"
#include "ptz_desc_set.h"
#include "ptz_host_batch.h"
#include "ptz_landmark.h"
#include "ptz_landmark_map.h"
#include "ptz_landmark_view_kernels.h"

namespace ptz {
namespace {

static_assert(kLmHomeWords == LV_WG, "one bitmap word a thread");
static_assert(kLandmarkMaxRefs == 32 * kLmHomeWords, "the bitmap covers every home a map can have");

struct LhIn {
  int n_lm, n_ref, n_query, n_tile, R;
  const int32_t* home;  // [n_lm]
  const int32_t* list;  // [R n_query]
};

// blockIdx.x = q * n_tile + tile.  SCATTER = false: cnt[blockIdx.x] = the listed landmarks of the tile.  SCATTER = true: cnt holds
// the tile's offset inside its query, vis_ptr the query's; entries at or beyond `capacity` are not written.
template <bool SCATTER>
__global__ __launch_bounds__(LV_WG) void k_landmark_home_view(LhIn a, int32_t* __restrict__ cnt, const int64_t* __restrict__ vis_ptr,
                                                              int32_t* __restrict__ vis_lm, int64_t capacity)
{
  __shared__ uint32_t s_bits[kLmHomeWords];
  __shared__ int32_t s_cnt[LV_WAVES];
  const int q = blockIdx.x / a.n_tile, tile = blockIdx.x % a.n_tile;
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  s_bits[threadIdx.x] = 32 * (int)threadIdx.x < a.n_ref ? lm_home_word(a.list + (int64_t)q * a.R, a.R, a.n_ref, (int32_t)threadIdx.x) : 0u;
  __syncthreads();
  const int base = tile * LV_TILE + wave * (LV_STEPS * WAVE);
  unsigned long long m[LV_STEPS];
  int n = 0;
#pragma unroll
  for (int s = 0; s < LV_STEPS; ++s) {
    const int l = base + s * WAVE + lane;
    const bool in = l < a.n_lm && lm_home_listed(s_bits, a.n_ref, a.home[l]);
    m[s] = __ballot(in);
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
      if (at >= 0 && at < capacity) vis_lm[at] = base + s * WAVE + lane;
    }
    o += __popcll(m[s]);
  }
}

// the home set of a map, built once; PTZ_OK or what ptz_desc_set_create answers
int32_t lh_home_set(const ptz_landmark_map* m)
{
  std::lock_guard<std::mutex> lock(m->home_mutex);
  if (m->home_set) return PTZ_OK;
  const size_t nl = (size_t)m->n_lm, D = (size_t)m->D;
  std::vector<int64_t> ptr((size_t)m->n_ref + 1, 0);
  std::vector<int32_t> lm(nl);
  if (!lm_home_groups(m->home.data(), m->n_lm, m->n_ref, ptr.data(), lm.data())) return PTZ_EINVAL;  // (cannot happen: the build's homes)
  std::vector<uint8_t> desc(nl * D);
  for (size_t i = 0; i < nl; ++i) memcpy(desc.data() + i * D, m->desc.data() + (size_t)lm[i] * D, D);
  const std::vector<float> kp(2 * (nl ? nl : 1), 0.f);
  ptz_desc_set* s = nullptr;
  if (const int32_t rc = ptz_desc_set_create(m->n_ref, ptr.data(), nl ? desc.data() : nullptr, m->D, kp.data(), m->device, &s)) return rc;
  m->home_ptr.swap(ptr);
  m->home_lm.swap(lm);
  m->home_set = s;
  return PTZ_OK;
}

bool lh_fits(const ptz_landmark_map* map, int n_query, int R)
{
  return map->n_ref <= kLandmarkMaxRefs && lv_fits(map->n_lm, n_query) && (int64_t)n_query * R <= INT32_MAX;
}

// The view of the lists: list (host, uploaded on the call's stream) or d_list (device).  st_callers: the stream d_list was written on.
int32_t lh_view(const ptz_landmark_map* map, int32_t n_query, int32_t R, const int32_t* list, const int32_t* d_list, int64_t max_view_bytes,
                bool callers_stream, hipStream_t st_callers, ptz_landmark_view** out)
{
  PTZ_DEVICE_GUARD(map->device);
  struct Free { void operator()(ptz_landmark_view* v) const { ptz_landmark_view_destroy(v); } };
  std::unique_ptr<ptz_landmark_view, Free> view(new ptz_landmark_view());
  view->device = map->device; view->kind = PTZ_LANDMARK_VIEW_HOMES; view->n_query = n_query; view->n_lm = map->n_lm;
  view->vis_ptr.assign((size_t)n_query + 1, 0);
  view->set = new ptz_desc_set();
  ptz_desc_set* s = view->set;
  s->device = map->device; s->n_img = n_query; s->D = map->D; s->KS = map->set->KS;
  const size_t nq = (size_t)n_query, slots = (size_t)R * nq;
  BlockLayout vb;
  const size_t o_vp = vb.take(sizeof(int64_t) * (nq + 1));
  if (view->blk.get(map->device, vb.total()) != hipSuccess) { (void)hipGetLastError(); return PTZ_ENOMEM; }
  view->d_vis_ptr = (const int64_t*)(view->blk.p + o_vp);

  // pass 1: the counts, the scans, and the one read that sizes the set
  BlockLayout tb;
  const size_t o_list = tb.take(sizeof(int32_t) * (slots ? slots : 1)), o_ws = tb.take(LvWork(map->n_lm, n_query).total);
  LvTables tables;  // (uploaded from: outlives the wait of h)
  std::optional<CallHeld> held;  // (after the view: the stream is waited for before a view that is not returned gives its blocks back)
  if (callers_stream) held.emplace(st_callers); else held.emplace();
  CallHeld& h = *held;
  if (const int32_t rc = h.acquire(map->device, tb.total())) { (void)hipGetLastError(); return rc; }
  char* d = h.base;
  if (list && slots > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_list, list, sizeof(int32_t) * slots, hipMemcpyHostToDevice, h.st));
    d_list = (const int32_t*)(d + o_list);
  }
  const LhIn a = {map->n_lm, map->n_ref, n_query, lv_tiles(map->n_lm), R, map->d_home, d_list};
  const bool work = n_query > 0 && a.n_tile > 0;
  int32_t* cnt = (int32_t*)(d + o_ws + LvWork(map->n_lm, n_query).cnt);
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  if (work)
    hipLaunchKernelGGL(k_landmark_home_view<false>, dim3((unsigned)(n_query * a.n_tile)), dim3(LV_WG), 0, h.st, a, cnt, (const int64_t*)nullptr,
                       (int32_t*)nullptr, (int64_t)0);
  lv_enqueue_scans(map->n_lm, n_query, (int64_t*)(view->blk.p + o_vp), d + o_ws, h.st);
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(view->vis_ptr.data(), view->d_vis_ptr, sizeof(int64_t) * (nq + 1), hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  view->device_ms = h.elapsed_ms();
  if (const int32_t rc = lv_size_set(view.get(), map, max_view_bytes, &tables, h.st)) return rc;
  const int64_t n_vis = view->n_vis;
  view->d_vis_uv = (const float*)s->d_kp;  // zeros: a home view predicts no pixel

  // pass 2: the scatter, then the rows
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  PTZ_HIP_TRY(hipMemsetAsync(s->d_kp, 0, sizeof(float2) * (size_t)(n_vis > 0 ? n_vis : 1), h.st));
  if (work && n_vis > 0)
    hipLaunchKernelGGL(k_landmark_home_view<true>, dim3((unsigned)(n_query * a.n_tile)), dim3(LV_WG), 0, h.st, a, cnt, view->d_vis_ptr,
                       (int32_t*)view->d_vis_lm, n_vis);
  lv_enqueue_rows(view.get(), map, h.st);
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  view->device_ms += h.elapsed_ms();
  *out = view.release();
  return PTZ_OK;
}

// the checks both forms of the view share, before any device work
int32_t lh_view_check(const ptz_landmark_map* map, int32_t n_query, int32_t R, const void* list, int64_t max_view_bytes, ptz_landmark_view** out)
{
  if (!out) return PTZ_EINVAL;
  *out = nullptr;
  if (!map || !map->set || n_query < 0 || R < 1 || max_view_bytes < 1 || (n_query > 0 && !list)) return PTZ_EINVAL;
  if (!lh_fits(map, n_query, R)) return PTZ_ELIMIT;
  return PTZ_OK;
}

}  // namespace
}  // namespace ptz

extern "C" const ptz_desc_set* ptz_landmark_map_home_set(const ptz_landmark_map* map)
{
  if (!map) return nullptr;
  if (ptz::lh_home_set(map) != PTZ_OK) return nullptr;
  return map->home_set;
}

extern "C" int32_t ptz_landmark_map_home_groups(const ptz_landmark_map* map, int64_t* home_ptr, int32_t* home_lm)
{
  if (!map) return PTZ_EINVAL;
  if (const int32_t rc = ptz::lh_home_set(map)) return rc;
  if (home_ptr) memcpy(home_ptr, map->home_ptr.data(), sizeof(int64_t) * map->home_ptr.size());
  if (home_lm && !map->home_lm.empty()) memcpy(home_lm, map->home_lm.data(), sizeof(int32_t) * map->home_lm.size());
  return PTZ_OK;
}

extern "C" int32_t ptz_landmark_shortlist(const ptz_landmark_map* map, const ptz_desc_set* query_set, int32_t n_query, const int32_t* query_img,
                                          const ptz_desc_options* desc_opt, const ptz_shortlist_options* sl_opt, int32_t* shortlist,
                                          int32_t* n_short, int32_t* votes, double* device_ms)
{
  if (!map) return PTZ_EINVAL;
  if (const int32_t rc = ptz::lh_home_set(map)) return rc;
  return ptz_desc_shortlist(map->home_set, query_set, n_query, query_img, desc_opt, sl_opt, shortlist, n_short, votes, device_ms);
}

extern "C" int64_t ptz_landmark_shortlist_workspace_bytes(const ptz_landmark_map* map, const ptz_desc_set* query_set, int32_t n_query,
                                                          const ptz_shortlist_options* sl_opt)
{
  if (!map || ptz::lh_home_set(map) != PTZ_OK) return 0;
  return ptz_desc_shortlist_workspace_bytes(map->home_set, query_set, n_query, sl_opt);
}

extern "C" int32_t ptz_landmark_shortlist_device(const ptz_landmark_map* map, const ptz_desc_set* query_set, int32_t n_query,
                                                 const int32_t* d_query_img, const ptz_desc_options* desc_opt,
                                                 const ptz_shortlist_options* sl_opt, int32_t* d_shortlist, int32_t* d_n_short, int32_t* d_votes,
                                                 void* d_workspace, int64_t workspace_bytes, void* hip_stream)
{
  if (!map) return PTZ_EINVAL;
  if (const int32_t rc = ptz::lh_home_set(map)) return rc;
  return ptz_desc_shortlist_device(map->home_set, query_set, n_query, d_query_img, desc_opt, sl_opt, d_shortlist, d_n_short, d_votes, d_workspace,
                                   workspace_bytes, hip_stream);
}

extern "C" int32_t ptz_landmark_view_kind(const ptz_landmark_view* v) { return v ? v->kind : PTZ_EINVAL; }

extern "C" int32_t ptz_landmark_view_from_homes(const ptz_landmark_map* map, int32_t n_query, int32_t max_refs, const int32_t* shortlist,
                                                int64_t max_view_bytes, ptz_landmark_view** out)
{
  using namespace ptz;
  // validation first, device second
  if (const int32_t rc = lh_view_check(map, n_query, max_refs, shortlist, max_view_bytes, out)) return rc;
  for (size_t k = 0; k < (size_t)max_refs * (size_t)n_query; ++k)
    if (!lm_home_entry_ok(shortlist[k], map->n_ref)) return PTZ_EINVAL;
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= map->device) return PTZ_ENODEVICE;
  return lh_view(map, n_query, max_refs, shortlist, nullptr, max_view_bytes, false, nullptr, out);
}

extern "C" int32_t ptz_landmark_view_from_homes_device(const ptz_landmark_map* map, int32_t n_query, int32_t max_refs, const int32_t* d_shortlist,
                                                       int64_t max_view_bytes, void* hip_stream, ptz_landmark_view** out)
{
  using namespace ptz;
  if (const int32_t rc = lh_view_check(map, n_query, max_refs, d_shortlist, max_view_bytes, out)) return rc;
  clear_stale_error(__func__);
  if (n_query > 0) {
    int device = -1;
    if (const int rc = owning_device(d_shortlist, hip_stream, &device)) return rc;
    if (device != map->device) return PTZ_EINVAL;
  }
  else {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= map->device) return PTZ_ENODEVICE;
  }
  return lh_view(map, n_query, max_refs, nullptr, d_shortlist, max_view_bytes, true, (hipStream_t)hip_stream, out);
}
