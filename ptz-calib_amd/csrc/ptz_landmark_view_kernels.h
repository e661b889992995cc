// ptz_landmark_view_kernels.h -- what the two landmark views share (ptz_landmark_prior.hip: the landmarks a prior camera sees;
// ptz_landmark_shortlist.hip: the landmarks of the homes on a query's list): a count pass and a scatter pass of their own stand
// around the scans and the row gather of this header, and the set of n_query images is sized and filled the same way.
//
//   tiles                      a workgroup of either predicate kernel is one (query, tile of 1024 landmarks): four waves, each four
//                              steps of 64 consecutive landmarks; its count goes to cnt[q * n_tile + tile]
//   k_landmark_view_scan       one wave per query: the exclusive scan of its tile counts, in place, and the query's total
//   k_landmark_view_ptr        one wave: the exclusive scan of the totals, vis_ptr [n_query + 1]
//   k_landmark_view_rows       blockIdx.x = image of the target set (the last is the slack behind it), threads stride over the
//                              16-byte pieces of its rows: a row of a listed landmark is copied from the map's set with its norm,
//                              a padding or slack row is zero with norm INT32_MAX -- every byte the matcher may read is written
// Everything here sits in an unnamed namespace: each of the two files gets kernels and helpers of its own.
#pragma once

#include <algorithm>
#include <vector>

#include "ptz_common.h"
#include "ptz_desc_set.h"
#include "ptz_host_batch.h"
#include "ptz_landmark_map.h"

namespace ptz {
namespace {

constexpr int LV_WG = 256;                     // four waves
constexpr int LV_STEPS = 4;                    // steps of 64 landmarks a wave
constexpr int LV_TILE = LV_WG * LV_STEPS;      // landmarks of a workgroup
constexpr int LV_WAVES = LV_WG / WAVE;

inline int lv_tiles(int n_lm) { return n_lm / LV_TILE + (n_lm % LV_TILE != 0); }  // (no overflow near 2^31)

template <typename T> __device__ __forceinline__ T lv_wave_inclusive(T v, int lane)
{
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const T o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// one wave per query: cnt[q][*] -> its exclusive scan, total[q] = the query's visible landmarks
__global__ __launch_bounds__(LV_WG) void k_landmark_view_scan(int n_query, int n_tile, int32_t* __restrict__ cnt, int32_t* __restrict__ total)
{
  const int q = blockIdx.x * LV_WAVES + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  if (q >= n_query) return;  // (one value in the wave)
  int32_t* c = cnt + (int64_t)q * n_tile;
  int32_t run = 0;
  for (int t0 = 0; t0 < n_tile; t0 += WAVE) {
    const int t = t0 + lane;
    const int32_t v = t < n_tile ? c[t] : 0;
    const int32_t inc = lv_wave_inclusive(v, lane);
    if (t < n_tile) c[t] = run + inc - v;
    run += __shfl(inc, WAVE - 1);
  }
  if (lane == 0) total[q] = run;
}

// one wave: vis_ptr = the exclusive scan of total, closed by the sum
__global__ __launch_bounds__(WAVE) void k_landmark_view_ptr(int n_query, const int32_t* __restrict__ total, int64_t* __restrict__ vis_ptr)
{
  const int lane = threadIdx.x;
  long long run = 0;
  for (int q0 = 0; q0 < n_query; q0 += WAVE) {
    const int q = q0 + lane;
    const long long v = q < n_query ? (long long)total[q] : 0;
    const long long inc = lv_wave_inclusive(v, lane);
    if (q < n_query) vis_ptr[q] = run + inc - v;
    run += __shfl(inc, WAVE - 1);
  }
  if (lane == 0) vis_ptr[n_query] = run;
}

// blockIdx.x = image m of the target set, image n_img its slack; blockIdx.y strides over the 16-byte pieces of the image's rows.
// feat_ptr / row_off: the target's tables [n_img + 2]; cpr = 4 KS pieces a row; src_row0: the map's first packed row.
__global__ __launch_bounds__(256) void k_landmark_view_rows(const int64_t* __restrict__ feat_ptr, const int64_t* __restrict__ row_off,
                                                            const int32_t* __restrict__ vis_lm, int32_t n_lm, int cpr, int64_t src_row0,
                                                            const uint4* __restrict__ src_desc, const int32_t* __restrict__ src_norm,
                                                            uint4* __restrict__ desc, int32_t* __restrict__ norm)
{
  const int m = blockIdx.x;
  const int64_t f0 = feat_ptr[m], n = feat_ptr[m + 1] - f0, r0 = row_off[m], np = row_off[m + 1] - r0;
  const int64_t pieces = np * cpr;
  for (int64_t c = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; c < pieces; c += (int64_t)gridDim.y * blockDim.x) {
    const int64_t r = c / cpr;
    const int part = (int)(c - r * cpr);
    int32_t l = -1;
    if (r < n) {
      l = vis_lm[f0 + r];
      if (l < 0 || l >= n_lm) l = -1;  // (cannot happen: the index came from the scatter)
    }
    uint4 x = make_uint4(0u, 0u, 0u, 0u);
    if (l >= 0) x = src_desc[(src_row0 + l) * cpr + part];
    desc[(r0 + r) * cpr + part] = x;
    if (part == 0) norm[r0 + r] = l >= 0 ? src_norm[src_row0 + l] : INT32_MAX;
  }
}

struct LvWork {
  size_t cnt, total_q, total;
  int n_tile;
  LvWork(int n_lm, int n_query)
  {
    n_tile = lv_tiles(n_lm);
    const size_t nq = (size_t)(n_query > 0 ? n_query : 1), nt = (size_t)(n_tile > 0 ? n_tile : 1);
    BlockLayout b;
    cnt = b.take(sizeof(int32_t) * nq * nt);
    total_q = b.take(sizeof(int32_t) * nq);
    total = b.total();
  }
};

inline bool lv_fits(int n_lm, int n_query) { return (int64_t)n_query * (lv_tiles(n_lm)) <= INT32_MAX; }

// after a count pass has written cnt of the workspace: the two scans, d_vis_ptr complete
inline void lv_enqueue_scans(int n_lm, int n_query, int64_t* d_vis_ptr, char* ws, hipStream_t st)
{
  const LvWork w(n_lm, n_query);
  int32_t *cnt = (int32_t*)(ws + w.cnt), *total = (int32_t*)(ws + w.total_q);
  if (n_query > 0)
    hipLaunchKernelGGL(k_landmark_view_scan, dim3((n_query + LV_WAVES - 1) / LV_WAVES), dim3(LV_WG), 0, st, n_query, w.n_tile, cnt, total);
  hipLaunchKernelGGL(k_landmark_view_ptr, dim3(1), dim3(WAVE), 0, st, n_query, (const int32_t*)total, d_vis_ptr);
}

// the tables of the view's set as they are uploaded: the caller keeps them until it has waited for the stream
struct LvTables {
  std::vector<int64_t> fp, ro;
};

// view->vis_ptr is on the host: the checks of a scan that ran, n_vis, the set's host tables, its size against the caller's bound
// and its block; the two tables are enqueued on st.  The set's key points (= d_vis_uv) and d_vis_lm are left to the scatter.
inline int32_t lv_size_set(ptz_landmark_view* view, const ptz_landmark_map* map, int64_t max_view_bytes, LvTables* t, hipStream_t st)
{
  ptz_desc_set* s = view->set;
  const size_t nq = (size_t)view->n_query;
  if (view->vis_ptr[0] != 0) return PTZ_ENODEVICE;  // (a scan that did not run)
  for (size_t q = 0; q < nq; ++q)
    if (view->vis_ptr[q + 1] < view->vis_ptr[q] || view->vis_ptr[q + 1] - view->vis_ptr[q] > map->n_lm) return PTZ_ENODEVICE;
  const int64_t n_vis = view->vis_ptr[nq];
  view->n_vis = n_vis;
  s->n_feat = n_vis;
  s->feat_ptr = view->vis_ptr;
  s->row_off.assign(nq + 1, 0);
  for (size_t q = 0; q < nq; ++q)
    s->row_off[q + 1] = s->row_off[q] + (s->feat_ptr[q + 1] - s->feat_ptr[q] + DESC_ROW_PAD - 1) / DESC_ROW_PAD * DESC_ROW_PAD;
  const int DP = 64 * s->KS;
  const int64_t rows64 = s->row_off[nq] + DESC_ROW_PAD;
  if (rows64 > INT32_MAX || n_vis > INT32_MAX) return PTZ_ELIMIT;
  const size_t rows = (size_t)rows64, nv1 = (size_t)(n_vis > 0 ? n_vis : 1);
  BlockLayout b;
  const size_t o_desc = b.take(rows * DP), o_norm = b.take(rows * sizeof(int32_t)), o_kp = b.take(nv1 * sizeof(float2)),
               o_lm = b.take(nv1 * sizeof(int32_t)), o_fp = b.take(sizeof(int64_t) * (nq + 2)), o_ro = b.take(sizeof(int64_t) * (nq + 2));
  if ((int64_t)b.total() > max_view_bytes) return PTZ_ELIMIT;
  if (s->blk.get(map->device, b.total()) != hipSuccess) { (void)hipGetLastError(); return PTZ_ENOMEM; }
  s->d_desc = (int8_t*)(s->blk.p + o_desc);
  s->d_norm = (int32_t*)(s->blk.p + o_norm);
  s->d_kp = (float2*)(s->blk.p + o_kp);
  s->d_feat_ptr = (const int64_t*)(s->blk.p + o_fp);
  s->d_row_off = (const int64_t*)(s->blk.p + o_ro);
  view->d_vis_lm = (const int32_t*)(s->blk.p + o_lm);
  t->fp = s->feat_ptr;
  t->ro = s->row_off;
  t->fp.push_back(n_vis);
  t->ro.push_back((int64_t)rows);
  PTZ_HIP_TRY(hipMemcpyAsync(s->blk.p + o_fp, t->fp.data(), sizeof(int64_t) * t->fp.size(), hipMemcpyHostToDevice, st));
  PTZ_HIP_TRY(hipMemcpyAsync(s->blk.p + o_ro, t->ro.data(), sizeof(int64_t) * t->ro.size(), hipMemcpyHostToDevice, st));
  return PTZ_OK;
}

// after the scatter has written d_vis_lm: the packed rows and norms of the view's set
inline void lv_enqueue_rows(const ptz_landmark_view* view, const ptz_landmark_map* map, hipStream_t st)
{
  const ptz_desc_set* s = view->set;
  int64_t most = DESC_ROW_PAD;
  for (size_t q = 0; q < (size_t)view->n_query; ++q) most = std::max(most, s->row_off[q + 1] - s->row_off[q]);
  const int cpr = 4 * s->KS;
  const int64_t gy = std::min<int64_t>((most * cpr + 255) / 256, 1024);
  hipLaunchKernelGGL(k_landmark_view_rows, dim3((unsigned)view->n_query + 1, (unsigned)gy), dim3(256), 0, st, s->d_feat_ptr, s->d_row_off,
                     view->d_vis_lm, map->n_lm, cpr, map->set->row_off[0], (const uint4*)map->set->d_desc, (const int32_t*)map->set->d_norm,
                     (uint4*)s->d_desc, s->d_norm);
}

}  // namespace
}  // namespace ptz
