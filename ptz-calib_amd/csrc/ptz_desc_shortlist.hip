// ptz_desc_shortlist.hip -- the reference shortlist in front of the matcher (ptz_desc_shortlist): a few probe features of every
// query vote for the references in which their nearest neighbour passes the ratio test, and the references with the most votes are
// the only ones the matcher then sees.  The contract is ptz_desc_shortlist.h; everything here is integer arithmetic on the packed
// rows of ptz_desc_set.h, so a query's votes are the bits of the brute-force restatement whatever the batch or the launch.
//
//   votes      k_desc_votes is the matcher's sweep (ptz_desc_sweep.h) with another outer shape: a workgroup owns 128 probe slots of
//              ONE query -- four waves of two 16-probe tiles, gathered once by the index rule -- and walks a strided group of
//              references, one sweep per reference.  On a reference's finished top-2 the g == 0 lanes apply the vote rule, and a
//              ballot's popcount is the wave's count: 12 bytes of top-2 state per feature and side become one int32.  No state,
//              keep byte, scan or gather.
//   partials   a wave writes its count to a cell of its own, [query][slot of 32 probes][reference]: no atomics; k_desc_shortlist
//              sums a query's slots in ascending order.  Every cell that is read has been written by exactly one wave of the same
//              call, so the workspace needs no clearing.
//   placement  the grid is one-dimensional over (query, probe tile) x reference group and dealt by ptz_xcd_map.h: the workgroups
//              that share an XCD's L2 walk the same reference group.  The references are split into enough groups for a full
//              machine's worth of workgroups when there is one query only.
//   shortlist  one wave per query: sum, rank by counting (the header's sl_takes, O(n_ref^2) per query), write in ascending index.
#include "ptz_common.h"
#include "ptz_desc_set.h"
#include "ptz_desc_shortlist.h"
#include "ptz_desc_sweep.h"
#include "ptz_host_batch.h"
#include "ptz_xcd_map.h"

namespace ptz {
namespace {

constexpr int SL_WG = 256;                       // four waves
constexpr int SL_QT = 2;                         // probe tiles of 16 per wave
constexpr int SL_WAVE_P = SL_QT * 16;            // 32 probe slots per wave: one partial cell
constexpr int SL_WG_P = (SL_WG / WAVE) * SL_WAVE_P;  // 128 probe slots per workgroup
constexpr int SL_TARGET_WGS = 1024;              // the reference split aims at this many workgroups at least

struct SlSide {  // one resident set, as a kernel reads it
  const int8_t* desc;
  const int32_t* norm;
  const int64_t* feat_ptr;  // [n_img + 2]
  const int64_t* row_off;   // [n_img + 2]; row_off[n_img] is the first row of the slack
  int32_t n_img;
};

struct SlQuery {  // a query's image, or no features for an index out of range
  int64_t row0;
  int32_t n;
};

__device__ __forceinline__ SlQuery sl_query(const SlSide& Q, const int32_t* __restrict__ query_img, int q)
{
  const int img = query_img ? query_img[q] : q;
  if (img < 0 || img >= Q.n_img) return SlQuery{0, 0};
  return SlQuery{Q.row_off[img], (int32_t)(Q.feat_ptr[img + 1] - Q.feat_ptr[img])};
}

// blockIdx.x dealt over gx = n_query * tiles items (query, tile of 128 probe slots) and gy reference groups (r = group, group + gy, ..)
template <int KS>
__global__ __launch_bounds__(SL_WG) void k_desc_votes(SlSide R, SlSide Q, const int32_t* __restrict__ query_img, int n_ref, int M, int tiles,
                                                      int n_slot, unsigned gx, unsigned gy, double r2, int32_t max_dist2,
                                                      int32_t* __restrict__ partial)
{
  constexpr int DP = KS * 64;
  const XcdItem it = xcd_live_item(blockIdx.x, gx, gy);
  if (!it.work) return;
  const int q = (int)(it.bx / (unsigned)tiles), tile = (int)(it.bx % (unsigned)tiles);
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE, c = lane & 15, g = lane >> 4;
  const SlQuery qi = sl_query(Q, query_img, q);
  const int m = sl_probe_count(qi.n, M);
  const int p0 = tile * SL_WG_P + wave * SL_WAVE_P;
  if (p0 >= m) return;  // (one value per wave, no barrier in this kernel; the next kernel reads no cell of this slot)

  // the probe rows, once: a slot past m reads a zero row of the slack behind the set and never votes
  const int64_t slack = Q.row_off[Q.n_img];
  v4i qf[SL_QT][KS];
  int32_t qn2[SL_QT];
  bool live[SL_QT];
#pragma unroll
  for (int t = 0; t < SL_QT; ++t) {
    const int slot = p0 + 16 * t + c;
    live[t] = slot < m;
    const int64_t row = live[t] ? qi.row0 + sl_probe_feature(slot, qi.n, M) : slack;
    qn2[t] = live[t] ? Q.norm[row] : 0;
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[t][s] = desc_frag<KS>(Q.desc, row, s, g);
  }

  for (int r = (int)it.by; r < n_ref; r += (int)gy) {
    const int64_t rr = R.row_off[r];
    DescRun run[SL_QT];
    desc_sweep<KS, SL_QT>(qf, R.desc + rr * DP, R.norm + rr, (int)(R.feat_ptr[r + 1] - R.feat_ptr[r]), c, g,
                          [&](int t, int32_t key, int32_t jj) { run[t].take(key, jj); });
    int32_t count = 0;
#pragma unroll
    for (int t = 0; t < SL_QT; ++t) {
      const DescTop2 T = desc_run_finish(run[t], qn2[t]);
      const bool vote = g == 0 && live[t] && sl_votes_for(r2, max_dist2, T);
      count += __popcll(__ballot(vote));
    }
    if (lane == 0) partial[((int64_t)q * n_slot + (p0 / SL_WAVE_P)) * n_ref + r] = count;
  }
}

// one wave per query: the votes (the query's slots in ascending order), the ranks, the list in ascending reference index
__global__ __launch_bounds__(SL_WG) void k_desc_shortlist(SlSide Q, const int32_t* __restrict__ query_img, int n_query, int n_ref, int M,
                                                          int n_slot, int R, int min_votes, const int32_t* __restrict__ partial,
                                                          int32_t* __restrict__ votes, int32_t* __restrict__ shortlist,
                                                          int32_t* __restrict__ n_short)
{
  const int lane = threadIdx.x % WAVE, q = blockIdx.x * (SL_WG / WAVE) + threadIdx.x / WAVE;
  const bool has = q < n_query;  // (every wave reaches the barrier)
  int32_t* v = votes + (int64_t)(has ? q : 0) * n_ref;
  if (has) {
    const int m = sl_probe_count(sl_query(Q, query_img, q).n, M);
    const int used = (m + SL_WAVE_P - 1) / SL_WAVE_P;
    for (int r = lane; r < n_ref; r += WAVE) {
      int32_t sum = 0;
      for (int s = 0; s < used; ++s) sum += partial[((int64_t)q * n_slot + s) * n_ref + r];
      v[r] = sum;
    }
  }
  __syncthreads();  // the wave ranks on what its other lanes wrote
  if (!has) return;
  const int taken = sl_wave_list(v, n_ref, R, min_votes, lane, shortlist + (int64_t)q * R, [](int, int) {});
  if (lane == 0) n_short[q] = taken;
}

// the extents of one call: the probe slots any query of the set can use, the workspace
struct SlWork {
  int cap, tiles, n_slot;
  size_t partial, votes, total;
  SlWork(const ptz_desc_set* Q, int n_query, int n_ref, int M)
  {
    int64_t most = 0;
    for (int i = 0; i < Q->n_img; ++i) most = std::max(most, Q->feat_ptr[i + 1] - Q->feat_ptr[i]);
    cap = (int)std::max<int64_t>(std::min<int64_t>(most, M), 1);
    tiles = (cap + SL_WG_P - 1) / SL_WG_P;
    n_slot = (cap + SL_WAVE_P - 1) / SL_WAVE_P;
    const size_t nq = (size_t)std::max(n_query, 1), nr = (size_t)std::max(n_ref, 1);
    BlockLayout b;
    partial = b.take(sizeof(int32_t) * nq * n_slot * nr);
    votes = b.take(sizeof(int32_t) * nq * nr);
    total = b.total();
  }
};

SlSide sl_side(const ptz_desc_set* s) { return SlSide{s->d_desc, s->d_norm, s->d_feat_ptr, s->d_row_off, s->n_img}; }

// the checks both forms share; *d and *s are the options with the defaults filled in
int32_t sl_check(const ptz_desc_set* refs, const ptz_desc_set* queries, int32_t n_query, const ptz_desc_options* desc_opt,
                 const ptz_shortlist_options* sl_opt, ptz_desc_options* d, ptz_shortlist_options* s)
{
  ptz_shortlist_options_default(s);
  if (sl_opt) *s = *sl_opt;
  if (const int32_t rc = desc_options_check(refs, queries, desc_opt, d)) return rc;
  if (n_query < 0) return PTZ_EINVAL;
  return shortlist_options_check(*s);
}

int32_t sl_limits(const ptz_desc_set* refs, const ptz_desc_set* queries, int32_t n_query, const ptz_shortlist_options& s)
{
  const SlWork w(queries, n_query, refs->n_img, s.n_probes);
  if ((int64_t)s.max_refs * n_query > INT32_MAX || (int64_t)n_query * w.n_slot * std::max(refs->n_img, 1) > INT32_MAX) return PTZ_ELIMIT;
  return PTZ_OK;
}

void sl_enqueue(const ptz_desc_set* refs, const ptz_desc_set* queries, int n_query, const int32_t* d_query_img, const ptz_desc_options& d,
                const ptz_shortlist_options& s, int32_t* d_shortlist, int32_t* d_n_short, int32_t* d_votes, char* ws, hipStream_t st)
{
  const int n_ref = refs->n_img, M = s.n_probes;
  const SlWork w(queries, n_query, n_ref, M);
  int32_t* partial = (int32_t*)(ws + w.partial);
  int32_t* votes = d_votes ? d_votes : (int32_t*)(ws + w.votes);
  const SlSide R = sl_side(refs), Q = sl_side(queries);
  if (n_ref > 0) {
    // (gx * gy <= n_query * tiles * n_ref <= the vote cells: below 2^31)
    const unsigned gx = (unsigned)n_query * (unsigned)w.tiles;
    const unsigned gy = std::min<unsigned>((unsigned)n_ref, std::max<unsigned>((SL_TARGET_WGS + gx - 1) / gx, 1u));
    const double r2 = d.ratio * d.ratio;
    PTZ_DESC_FOR_KS(refs->KS, hipLaunchKernelGGL((k_desc_votes<K>), dim3(gx * gy), dim3(SL_WG), 0, st, R, Q, d_query_img, n_ref, M, w.tiles,
                                                 w.n_slot, gx, gy, r2, d.max_dist2, partial));
  }
  const int per = SL_WG / WAVE;
  hipLaunchKernelGGL(k_desc_shortlist, dim3((n_query + per - 1) / per), dim3(SL_WG), 0, st, Q, d_query_img, n_query, n_ref, M, w.n_slot, s.max_refs,
                     s.min_votes, (const int32_t*)partial, votes, d_shortlist, d_n_short);
}

}  // namespace
}  // namespace ptz

extern "C" void ptz_shortlist_options_default(ptz_shortlist_options* o)
{
  if (!o) return;
  o->max_refs = 8;
  o->n_probes = 256;
  o->min_votes = 1;
  o->reserved_ = 0;
}

extern "C" int64_t ptz_desc_shortlist_workspace_bytes(const ptz_desc_set* ref_set, const ptz_desc_set* query_set, int32_t n_query,
                                                      const ptz_shortlist_options* sl_opt)
{
  ptz_shortlist_options s;
  ptz_shortlist_options_default(&s);
  if (sl_opt) s = *sl_opt;
  if (!ref_set || !query_set || n_query < 0 || s.n_probes < 1) return 0;
  return (int64_t)ptz::SlWork(query_set, n_query, ref_set->n_img, s.n_probes).total;
}

extern "C" int32_t ptz_desc_shortlist_device(const ptz_desc_set* ref_set, const ptz_desc_set* query_set, int32_t n_query,
                                             const int32_t* d_query_img, const ptz_desc_options* desc_opt,
                                             const ptz_shortlist_options* sl_opt, int32_t* d_shortlist, int32_t* d_n_short, int32_t* d_votes,
                                             void* d_workspace, int64_t workspace_bytes, void* hip_stream)
{
  using namespace ptz;
  ptz_desc_options d;
  ptz_shortlist_options s;
  if (const int32_t rc = sl_check(ref_set, query_set, n_query, desc_opt, sl_opt, &d, &s)) return rc;
  if (n_query == 0) return PTZ_OK;
  if (!d_query_img && n_query > query_set->n_img) return PTZ_EINVAL;
  if (!d_shortlist || !d_n_short || !d_workspace) return PTZ_EINVAL;
  if (const int32_t rc = sl_limits(ref_set, query_set, n_query, s)) return rc;
  if (((uintptr_t)d_workspace & 255) != 0 || workspace_bytes < ptz_desc_shortlist_workspace_bytes(ref_set, query_set, n_query, &s)) return PTZ_EINVAL;
  clear_stale_error(__func__);
  int device = -1;
  if (const int rc = owning_device(d_shortlist, hip_stream, &device)) return rc;
  if (device != ref_set->device) return PTZ_EINVAL;
  PTZ_DEVICE_GUARD(device);
  sl_enqueue(ref_set, query_set, n_query, d_query_img, d, s, d_shortlist, d_n_short, d_votes, (char*)d_workspace, (hipStream_t)hip_stream);
  PTZ_HIP_TRY(hipGetLastError());
  return PTZ_OK;
}

extern "C" int32_t ptz_desc_shortlist(const ptz_desc_set* ref_set, const ptz_desc_set* query_set, int32_t n_query, const int32_t* query_img,
                                      const ptz_desc_options* desc_opt, const ptz_shortlist_options* sl_opt, int32_t* shortlist,
                                      int32_t* n_short, int32_t* votes, double* device_ms)
{
  using namespace ptz;
  ptz_desc_options d;
  ptz_shortlist_options s;
  if (const int32_t rc = sl_check(ref_set, query_set, n_query, desc_opt, sl_opt, &d, &s)) return rc;
  if (n_query > 0 && (!query_img || !shortlist || !n_short)) return PTZ_EINVAL;
  for (int q = 0; q < n_query; ++q)
    if (query_img[q] < 0 || query_img[q] >= query_set->n_img) return PTZ_EINVAL;
  if (device_ms) *device_ms = 0;
  if (n_query == 0) return PTZ_OK;
  if (const int32_t rc = sl_limits(ref_set, query_set, n_query, s)) return rc;
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= ref_set->device) return PTZ_ENODEVICE;
  const int dev = ref_set->device;
  PTZ_DEVICE_GUARD(dev);

  const size_t nq = (size_t)n_query, nr = (size_t)std::max(ref_set->n_img, 1), R = (size_t)s.max_refs;
  BlockLayout b;
  const size_t o_img = b.take(sizeof(int32_t) * nq), o_sl = b.take(sizeof(int32_t) * R * nq), o_ns = b.take(sizeof(int32_t) * nq),
               o_votes = b.take(sizeof(int32_t) * nq * nr), o_ws = b.take(SlWork(query_set, n_query, ref_set->n_img, s.n_probes).total);
  CallHeld h;
  if (const int32_t rc = h.acquire(dev, b.total())) return rc;
  char* p = h.base;
  PTZ_HIP_TRY(hipMemcpyAsync(p + o_img, query_img, sizeof(int32_t) * nq, hipMemcpyHostToDevice, h.st));
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  sl_enqueue(ref_set, query_set, n_query, (const int32_t*)(p + o_img), d, s, (int32_t*)(p + o_sl), (int32_t*)(p + o_ns), (int32_t*)(p + o_votes),
             p + o_ws, h.st);
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(shortlist, p + o_sl, sizeof(int32_t) * R * nq, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(hipMemcpyAsync(n_short, p + o_ns, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, h.st));
  if (votes && ref_set->n_img > 0) PTZ_HIP_TRY(hipMemcpyAsync(votes, p + o_votes, sizeof(int32_t) * nq * ref_set->n_img, hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  PTZ_HIP_TRY(hipGetLastError());
  if (device_ms) *device_ms = h.elapsed_ms();
  return PTZ_OK;
}
