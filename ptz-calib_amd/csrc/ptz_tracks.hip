// ptz_tracks.hip -- feature tracks on the device (gfx950): the connected components of the resident match table by hooking, in one
// pass over the edges, and the components that are tracks laid out in ascending (label, node).  The contract is ptz_tracks.h; this
// file adds the launch shapes and the C-ABI, nothing the result depends on.
//
//   k_trk_init      parent[k] = k, counters and flags cleared (the workspace is never read before it is written)
//   k_trk_hook      one edge a lane: the pair of the match by bisection of match_ptr, trk_edge_nodes, trk_hook.  Inside THIS launch
//                   every read of parent is a relaxed agent-scope atomic load and every write an agent-scope atomic (TrkAgentMem):
//                   workgroups on different XCDs hook into the same array, and neither a CU's L1 nor another XCD's L2 may serve a
//                   stale parent.  The matched flags are plain stores of one value, read by later launches only.
//   k_trk_label     one node a lane, plain loads: label = root, integer add into the root's count
//   k_trk_classify  one node a lane: roots by trk_class; the scan's input (1 << 32 | count) for the roots that become segments
//   (scan)          k_scan_sums / k_scan_blocks / k_scan_apply: an exclusive scan of uint64 over 1024 elements a workgroup, the block
//                   sums by ONE workgroup in a loop -- three launches, no workgroup waits for another
//   k_trk_scatter   one node a lane: its slot through its root's cursor; a root writes its segment's offset
//   k_trk_sort      one wave a segment: trk_rank by counting (a segment has at most n_img entries)
//   k_trk_verdict   one wave a segment: neighbours that share an image, trk_verdict, the second scan's input (1 << 32 | len)
//   (scan again)    track index and view offset of every kept segment
//   k_trk_gather    one wave a segment: the kept ones to trk_ptr / trk_img / trk_feat / trk_node / trk_uv, and the sizes
//
// Every loop is bounded by a count known at its entry; a walk or a retry loop that reaches the cap of n_feat steps sets the error
// word and leaves.  Integer atomics only; the counts are sums of integers, so nothing depends on the order of anything.
#include "ptz_tracks.h"

#include <memory>
#include <vector>

#include "ptz_common.h"
#include "ptz_desc_set.h"
#include "ptz_host_batch.h"
#include "ptz_tracks_obj.h"

namespace ptz {
namespace {

constexpr int TRK_WG = 256;
constexpr int SCAN_ITEMS = 4;                      // elements a lane
constexpr int SCAN_BLOCK = TRK_WG * SCAN_ITEMS;    // elements a workgroup
enum { SZ_TRACK = 0, SZ_VIEW, SZ_MATCHED, SZ_COMP, SZ_REPEAT, SZ_SHORT, SZ_ERR, SZ_N };
typedef unsigned long long u64;

struct TrkAgentMem {
  __device__ __forceinline__ int32_t load(const int32_t* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void store(int32_t* p, int32_t v) const { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ bool cas(int32_t* p, int32_t expect, int32_t v, int32_t* seen) const
  {
    const bool won = __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *seen = expect;
    return won;
  }
};

struct TrkIn {
  int32_t n_img, n_pair, min_len;
  int64_t n_feat, n_match, n_seg_max;
  const int64_t *feat_ptr, *match_ptr;
  const int32_t *img_a, *img_b, *idx_a, *idx_b;
  const float2* kp;
};

struct TrkWork {
  int32_t *parent, *label, *cnt, *cursor, *tmp, *sorted;
  uint8_t* matched;
  u64 *val, *out, *bsum;
  int64_t* seg_ptr;
};

__device__ __forceinline__ void count_add(int64_t* sizes, int slot, bool mine)
{
  const u64 b = __ballot(mine);
  if (b != 0 && (threadIdx.x & (WAVE - 1)) == (unsigned)(__ffsll((long long)b) - 1)) atomicAdd((u64*)(sizes + slot), (u64)__popcll(b));
}

__global__ __launch_bounds__(TRK_WG) void k_trk_init(int64_t n, int64_t n_seg_max, TrkWork w, int64_t* __restrict__ sizes, int64_t* __restrict__ trk_ptr)
{
  const int64_t k = (int64_t)blockIdx.x * TRK_WG + threadIdx.x;
  if (k < n) { w.parent[k] = (int32_t)k; w.cnt[k] = 0; w.cursor[k] = 0; w.matched[k] = 0; }
  if (k <= n_seg_max) w.seg_ptr[k] = 0;
  if (k < SZ_N + 1) sizes[k] = 0;
  if (k == 0) trk_ptr[0] = 0;
}

__global__ __launch_bounds__(TRK_WG) void k_trk_hook(TrkIn a, TrkWork w, int64_t* __restrict__ sizes)
{
  const int64_t m = (int64_t)blockIdx.x * TRK_WG + threadIdx.x;
  if (m >= a.n_match) return;
  if (m < a.match_ptr[0] || m >= a.match_ptr[a.n_pair]) return;  // (a table that does not cover its matches: no pair, no edge)
  const int32_t p = trk_owner(a.match_ptr, a.n_pair, m);
  int32_t u, v;
  if (!trk_edge_nodes(a.n_img, a.feat_ptr, a.img_a[p], a.img_b[p], a.idx_a[m], a.idx_b[m], &u, &v)) return;
  if (u < 0 || v < 0 || u >= a.n_feat || v >= a.n_feat) return;  // (a feat_ptr that runs past the n_feat the workspace was sized for)
  w.matched[u] = 1;
  w.matched[v] = 1;
  if (u == v) return;
  if (!trk_hook(TrkAgentMem(), w.parent, u, v, a.n_feat)) sizes[SZ_ERR] = 1;
}

__global__ __launch_bounds__(TRK_WG) void k_trk_label(int64_t n, TrkWork w, int64_t* __restrict__ sizes)
{
  const int64_t k = (int64_t)blockIdx.x * TRK_WG + threadIdx.x;
  if (k >= n) return;
  int32_t r = -1;
  if (w.matched[k]) {
    r = trk_root(w.parent, (int32_t)k, n);
    if (r < 0) sizes[SZ_ERR] = 1;
    else atomicAdd(&w.cnt[r], 1);
  }
  w.label[k] = r;
}

__global__ __launch_bounds__(TRK_WG) void k_trk_classify(int64_t n, int32_t n_img, TrkWork w, int64_t* __restrict__ sizes)
{
  const int64_t k = (int64_t)blockIdx.x * TRK_WG + threadIdx.x;
  const bool in = k < n;
  const bool matched = in && w.label[in ? k : 0] >= 0;
  const bool root = matched && w.label[k] == (int32_t)k;
  const int32_t c = root ? w.cnt[k] : 0;
  const int32_t cls = trk_class(c, n_img);
  if (in) w.val[k] = cls == TRK_SEGMENT ? ((u64)1 << 32 | (u64)c) : 0;
  count_add(sizes, SZ_MATCHED, matched);
  count_add(sizes, SZ_COMP, root);
  count_add(sizes, SZ_REPEAT, cls == TRK_PIGEON);
  count_add(sizes, SZ_SHORT, cls == TRK_SINGLE);
}

// ---- exclusive scan of u64: out [n + 1], out[n] the total --------------------------------------------------------------------------
// the sum of a workgroup's values in every lane of it, and before[0] the sum over the lanes below this one
__device__ __forceinline__ u64 block_exclusive(u64 v, u64* lds, u64* total)
{
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  u64 inc = v;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const u64 t = __shfl_up(inc, d, WAVE);
    if (lane >= d) inc += t;
  }
  __syncthreads();
  if (lane == WAVE - 1) lds[wv] = inc;
  __syncthreads();
  u64 base = 0, all = 0;
#pragma unroll
  for (int i = 0; i < TRK_WG / WAVE; ++i) {
    if (i < wv) base += lds[i];
    all += lds[i];
  }
  *total = all;
  return base + inc - v;
}

__global__ __launch_bounds__(TRK_WG) void k_scan_sums(int64_t n, const u64* __restrict__ in, u64* __restrict__ bsum)
{
  __shared__ u64 lds[TRK_WG / WAVE];
  const int64_t i0 = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)threadIdx.x * SCAN_ITEMS;
  u64 s = 0;
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j)
    if (i0 + j < n) s += in[i0 + j];
  u64 total;
  (void)block_exclusive(s, lds, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// ONE workgroup: bsum [nb] -> its exclusive scan in place, bsum[nb] the total
__global__ __launch_bounds__(TRK_WG) void k_scan_blocks(int64_t nb, u64* __restrict__ bsum)
{
  __shared__ u64 lds[TRK_WG / WAVE];
  u64 carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += TRK_WG) {
    const int64_t b = b0 + threadIdx.x;
    const u64 v = b < nb ? bsum[b] : 0;
    u64 total;
    const u64 before = block_exclusive(v, lds, &total);
    if (b < nb) bsum[b] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) bsum[nb] = carry;
}

__global__ __launch_bounds__(TRK_WG) void k_scan_apply(int64_t n, int64_t nb, const u64* __restrict__ in, const u64* __restrict__ bsum, u64* __restrict__ out)
{
  __shared__ u64 lds[TRK_WG / WAVE];
  const int64_t i0 = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)threadIdx.x * SCAN_ITEMS;
  u64 v[SCAN_ITEMS], s = 0;
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    v[j] = i0 + j < n ? in[i0 + j] : 0;
    s += v[j];
  }
  u64 total;
  u64 run = bsum[blockIdx.x] + block_exclusive(s, lds, &total);
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    if (i0 + j < n) out[i0 + j] = run;
    run += v[j];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = bsum[nb];
}

void enqueue_scan(int64_t n, const u64* in, u64* bsum, u64* out, hipStream_t st)
{
  const int64_t nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
  hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)nb), dim3(TRK_WG), 0, st, n, in, bsum);
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(TRK_WG), 0, st, nb, bsum);
  hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(TRK_WG), 0, st, n, nb, in, (const u64*)bsum, out);
}

__device__ __forceinline__ int32_t hi32(u64 x) { return (int32_t)(x >> 32); }
__device__ __forceinline__ int32_t lo32(u64 x) { return (int32_t)(x & 0xffffffffu); }

__global__ __launch_bounds__(TRK_WG) void k_trk_scatter(int64_t n, int32_t n_img, TrkWork w)
{
  const int64_t k = (int64_t)blockIdx.x * TRK_WG + threadIdx.x;
  if (k == 0) w.seg_ptr[hi32(w.out[n])] = lo32(w.out[n]);  // (the end of the last segment; without segments entry 0)
  if (k >= n) return;
  const int32_t r = w.label[k];
  if (r < 0) return;
  const int32_t c = w.cnt[r];
  if (trk_class(c, n_img) != TRK_SEGMENT) return;
  const int32_t start = lo32(w.out[r]);
  const int32_t at = atomicAdd(&w.cursor[r], 1);
  if (at < c) w.tmp[start + at] = (int32_t)k;  // (at < c always: the count was taken over the same nodes)
  if (r == (int32_t)k) w.seg_ptr[hi32(w.out[r])] = start;
}

__global__ __launch_bounds__(TRK_WG) void k_trk_sort(int64_t n, TrkWork w)
{
  const int64_t s = (int64_t)blockIdx.x * (TRK_WG / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (s >= hi32(w.out[n])) return;
  const int64_t start = w.seg_ptr[s];
  const int32_t len = (int32_t)(w.seg_ptr[s + 1] - start);
  for (int32_t i = lane; i < len; i += WAVE) w.sorted[start + trk_rank(w.tmp + start, len, i)] = w.tmp[start + i];
}

__global__ __launch_bounds__(TRK_WG) void k_trk_verdict(TrkIn a, TrkWork w, int64_t* __restrict__ sizes)
{
  const int64_t s = (int64_t)blockIdx.x * (TRK_WG / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (s >= a.n_seg_max) return;
  if (s >= hi32(w.out[a.n_feat])) {
    if (lane == 0) w.val[s] = 0;
    return;
  }
  const int64_t start = w.seg_ptr[s];
  const int32_t len = (int32_t)(w.seg_ptr[s + 1] - start);
  bool rep = false;
  for (int32_t i = lane; i + 1 < len; i += WAVE)
    rep = rep || trk_owner(a.feat_ptr, a.n_img, w.sorted[start + i]) == trk_owner(a.feat_ptr, a.n_img, w.sorted[start + i + 1]);
  const int32_t verdict = trk_verdict(__any(rep), len, a.min_len);
  if (lane != 0) return;
  w.val[s] = verdict == TRK_KEEP ? ((u64)1 << 32 | (u64)len) : 0;
  if (verdict == TRK_REPEAT) atomicAdd((u64*)(sizes + SZ_REPEAT), (u64)1);
  if (verdict == TRK_SHORT) atomicAdd((u64*)(sizes + SZ_SHORT), (u64)1);
}

// (w.val / w.out hold the SECOND scan here: over segments)
__global__ __launch_bounds__(TRK_WG) void k_trk_gather(TrkIn a, TrkWork w, int64_t n_seg, int64_t* __restrict__ trk_ptr, int32_t* __restrict__ trk_img,
                                                       int32_t* __restrict__ trk_feat, int32_t* __restrict__ trk_node, float2* __restrict__ trk_uv,
                                                       int64_t* __restrict__ sizes)
{
  const int64_t s = (int64_t)blockIdx.x * (TRK_WG / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const u64 all = w.out[a.n_seg_max];
    sizes[SZ_TRACK] = hi32(all);
    sizes[SZ_VIEW] = lo32(all);
    trk_ptr[hi32(all)] = lo32(all);
  }
  if (s >= n_seg || w.val[s] == 0) return;
  const int32_t t = hi32(w.out[s]), o = lo32(w.out[s]), len = lo32(w.val[s]);
  const int64_t start = w.seg_ptr[s];
  if (lane == 0) trk_ptr[t] = o;
  for (int32_t i = lane; i < len; i += WAVE) {
    const int32_t node = w.sorted[start + i];
    const int32_t img = trk_owner(a.feat_ptr, a.n_img, node);
    trk_node[o + i] = node;
    trk_img[o + i] = img;
    trk_feat[o + i] = (int32_t)(node - a.feat_ptr[img]);
    if (trk_uv) trk_uv[o + i] = a.kp ? a.kp[node] : make_float2(0.f, 0.f);
  }
}

int64_t seg_max_of(int64_t n_feat) { return n_feat / 2 + 1; }

struct TrkLayout {
  size_t parent, label, cnt, cursor, tmp, sorted, matched, val, out, bsum, seg_ptr, total;
  explicit TrkLayout(int64_t n_feat)
  {
    const size_t n = (size_t)(n_feat > 0 ? n_feat : 1), s = (size_t)seg_max_of(n_feat);
    const size_t nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    BlockLayout b;
    parent = b.take(sizeof(int32_t) * n); label = b.take(sizeof(int32_t) * n); cnt = b.take(sizeof(int32_t) * n);
    cursor = b.take(sizeof(int32_t) * n); tmp = b.take(sizeof(int32_t) * n); sorted = b.take(sizeof(int32_t) * n);
    matched = b.take(n); val = b.take(sizeof(u64) * n); out = b.take(sizeof(u64) * (n + 1)); bsum = b.take(sizeof(u64) * (nb + 1));
    seg_ptr = b.take(sizeof(int64_t) * (s + 1));
    total = b.total();
  }
};

// the launches of one build on `st`; nothing is waited for
void enqueue_tracks(const TrkIn& a, char* ws, int64_t* d_trk_ptr, int32_t* d_trk_img, int32_t* d_trk_feat, int32_t* d_trk_node, float* d_trk_uv,
                    int64_t* d_sizes, hipStream_t st)
{
  const TrkLayout l(a.n_feat);
  const TrkWork w = {(int32_t*)(ws + l.parent), (int32_t*)(ws + l.label), (int32_t*)(ws + l.cnt), (int32_t*)(ws + l.cursor), (int32_t*)(ws + l.tmp),
                     (int32_t*)(ws + l.sorted), (uint8_t*)(ws + l.matched), (u64*)(ws + l.val), (u64*)(ws + l.out), (u64*)(ws + l.bsum),
                     (int64_t*)(ws + l.seg_ptr)};
  const int64_t n = a.n_feat, smax = a.n_seg_max;
  auto blocks = [](int64_t items, int per) { return dim3((unsigned)((items + per - 1) / per)); };
  const int64_t n_init = std::max<int64_t>(std::max<int64_t>(n, smax + 1), SZ_N + 1);
  hipLaunchKernelGGL(k_trk_init, blocks(n_init, TRK_WG), dim3(TRK_WG), 0, st, n, smax, w, d_sizes, d_trk_ptr);
  if (n <= 0 || a.n_match <= 0 || a.n_pair <= 0) return;
  hipLaunchKernelGGL(k_trk_hook, blocks(a.n_match, TRK_WG), dim3(TRK_WG), 0, st, a, w, d_sizes);
  hipLaunchKernelGGL(k_trk_label, blocks(n, TRK_WG), dim3(TRK_WG), 0, st, n, w, d_sizes);
  hipLaunchKernelGGL(k_trk_classify, blocks(n, TRK_WG), dim3(TRK_WG), 0, st, n, a.n_img, w, d_sizes);
  enqueue_scan(n, w.val, w.bsum, w.out, st);
  hipLaunchKernelGGL(k_trk_scatter, blocks(n, TRK_WG), dim3(TRK_WG), 0, st, n, a.n_img, w);
  const int per = TRK_WG / WAVE;
  hipLaunchKernelGGL(k_trk_sort, blocks(smax, per), dim3(TRK_WG), 0, st, n, w);
  hipLaunchKernelGGL(k_trk_verdict, blocks(smax, per), dim3(TRK_WG), 0, st, a, w, d_sizes);
  enqueue_scan(smax, w.val, w.bsum, w.out, st);
  hipLaunchKernelGGL(k_trk_gather, blocks(smax, per), dim3(TRK_WG), 0, st, a, w, smax, d_trk_ptr, d_trk_img, d_trk_feat, d_trk_node,
                     (float2*)d_trk_uv, d_sizes);
}

struct TracksFree { void operator()(ptz_tracks* t) const { ptz_tracks_destroy(t); } };

// the outputs of a ptz_tracks at the extents of ptz_tracks_build_device, the sizes behind them
int32_t tracks_alloc(ptz_tracks* t, int64_t** d_sizes)
{
  const size_t n = (size_t)(t->n_feat > 0 ? t->n_feat : 1);
  BlockLayout b;
  const size_t o_ptr = b.take(sizeof(int64_t) * ((size_t)seg_max_of(t->n_feat) + 1)), o_img = b.take(sizeof(int32_t) * n), o_feat = b.take(sizeof(int32_t) * n),
               o_node = b.take(sizeof(int32_t) * n), o_uv = b.take(sizeof(float) * 2 * n), o_sizes = b.take(sizeof(int64_t) * (SZ_N + 1));
  if (t->blk.get(t->device, b.total()) != hipSuccess) { (void)hipGetLastError(); return PTZ_ENOMEM; }
  char* d = t->blk.p;
  t->d_trk_ptr = (int64_t*)(d + o_ptr); t->d_trk_img = (int32_t*)(d + o_img); t->d_trk_feat = (int32_t*)(d + o_feat);
  t->d_trk_node = (int32_t*)(d + o_node); t->d_trk_uv = (float*)(d + o_uv);
  *d_sizes = (int64_t*)(d + o_sizes);
  return PTZ_OK;
}

// after the launches: the sizes, the counts and the error word -- the only download of a build
int32_t tracks_finish(ptz_tracks* t, CallHeld& h, const int64_t* d_sizes)
{
  PTZ_HIP_TRY(hipGetLastError());
  PTZ_HIP_TRY(hipEventRecord(h.ev[1], h.st));
  int64_t sizes[SZ_N + 1] = {0};
  PTZ_HIP_TRY(hipMemcpyAsync(sizes, d_sizes, sizeof(sizes), hipMemcpyDeviceToHost, h.st));
  PTZ_HIP_TRY(stream_wait(h.st));
  if (sizes[SZ_ERR] != 0) {
    fprintf(stderr, "[ptzcalib] ptz_tracks: a bounded loop reached its cap of %lld steps\n", (long long)t->n_feat);
    return PTZ_EINTERNAL;
  }
  if (sizes[SZ_TRACK] < 0 || sizes[SZ_TRACK] > seg_max_of(t->n_feat) || sizes[SZ_VIEW] < 0 || sizes[SZ_VIEW] > t->n_feat) return PTZ_EINTERNAL;
  t->n_track = (int32_t)sizes[SZ_TRACK];
  t->n_view = sizes[SZ_VIEW];
  for (int k = 0; k < 4; ++k) t->counts[k] = sizes[SZ_MATCHED + k];
  t->device_ms = h.elapsed_ms();
  return PTZ_OK;
}

bool offsets_ok(const int64_t* ptr, int64_t n)
{
  if (!ptr || ptr[0] != 0) return false;
  for (int64_t k = 0; k < n; ++k)
    if (ptr[k + 1] < ptr[k]) return false;
  return true;
}

}  // namespace
}  // namespace ptz

extern "C" void ptz_tracks_destroy(ptz_tracks* t)
{
  if (!t) return;
  ptz::DeviceGuard g(t->device);
  delete t;
}

extern "C" int64_t ptz_tracks_workspace_bytes(int64_t n_feat) { return n_feat < 0 ? 0 : (int64_t)ptz::TrkLayout(n_feat).total; }

extern "C" int32_t ptz_tracks_build_device(int32_t n_img, const int64_t* d_feat_ptr, int64_t n_feat, const float* d_kp, int32_t n_pair,
                                           const int32_t* d_img_a, const int32_t* d_img_b, const int64_t* d_match_ptr, int64_t n_match,
                                           const int32_t* d_idx_a, const int32_t* d_idx_b, int32_t min_len, int64_t* d_trk_ptr,
                                           int32_t* d_trk_img, int32_t* d_trk_feat, int32_t* d_trk_node, float* d_trk_uv, int64_t* d_sizes,
                                           void* d_workspace, int64_t workspace_bytes, void* hip_stream)
{
  using namespace ptz;
  if (n_img < 0 || n_feat < 0 || n_pair < 0 || n_match < 0 || min_len < 2 || !d_feat_ptr || !d_trk_ptr || !d_sizes || !d_workspace) return PTZ_EINVAL;
  if (n_feat > 0 && (!d_trk_img || !d_trk_feat || !d_trk_node)) return PTZ_EINVAL;
  if (n_pair > 0 && (!d_img_a || !d_img_b || !d_match_ptr)) return PTZ_EINVAL;
  if (n_match > 0 && (!d_idx_a || !d_idx_b || n_pair == 0)) return PTZ_EINVAL;
  if (n_feat >= ((int64_t)1 << 31) || n_match >= ((int64_t)1 << 31)) return PTZ_ELIMIT;
  if (((uintptr_t)d_workspace & 255) != 0 || workspace_bytes < ptz_tracks_workspace_bytes(n_feat)) return PTZ_EINVAL;
  int device = 0;
  if (const int32_t rc = owning_device(d_trk_ptr, hip_stream, &device)) return rc;
  clear_stale_error(__func__);
  PTZ_DEVICE_GUARD(device);
  const TrkIn a = {n_img, n_pair, min_len, n_feat, n_match, seg_max_of(n_feat), d_feat_ptr, d_match_ptr, d_img_a, d_img_b, d_idx_a, d_idx_b, (const float2*)d_kp};
  enqueue_tracks(a, (char*)d_workspace, d_trk_ptr, d_trk_img, d_trk_feat, d_trk_node, d_trk_uv, d_sizes, (hipStream_t)hip_stream);
  PTZ_HIP_TRY(hipGetLastError());
  return PTZ_OK;
}

extern "C" int32_t ptz_tracks_build(int32_t n_img, const int64_t* feat_ptr, int32_t n_pair, const int32_t* img_a, const int32_t* img_b,
                                    const int64_t* match_ptr, const int32_t* idx_a, const int32_t* idx_b, int32_t min_len, int32_t device_id,
                                    ptz_tracks** out)
{
  using namespace ptz;
  if (!out) return PTZ_EINVAL;
  *out = nullptr;
  // validation first, device second
  if (n_img < 0 || n_pair < 0 || min_len < 2 || device_id < 0 || !offsets_ok(feat_ptr, n_img)) return PTZ_EINVAL;
  if (n_pair > 0 && (!img_a || !img_b || !offsets_ok(match_ptr, n_pair))) return PTZ_EINVAL;
  const int64_t n_feat = feat_ptr[n_img], n_match = n_pair > 0 ? match_ptr[n_pair] : 0;
  if (n_match > 0 && (!idx_a || !idx_b)) return PTZ_EINVAL;
  if (n_feat >= ((int64_t)1 << 31) || n_match >= ((int64_t)1 << 31)) return PTZ_ELIMIT;
  for (int32_t p = 0; p < n_pair; ++p) {
    if (img_a[p] < 0 || img_a[p] >= n_img || img_b[p] < 0 || img_b[p] >= n_img) return PTZ_EINVAL;
    for (int64_t m = match_ptr[p]; m < match_ptr[p + 1]; ++m) {
      int32_t u, v;
      if (!trk_edge_nodes(n_img, feat_ptr, img_a[p], img_b[p], idx_a[m], idx_b[m], &u, &v)) return PTZ_EINVAL;
    }
  }
  clear_stale_error(__func__);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) return PTZ_ENODEVICE;
  PTZ_DEVICE_GUARD(device_id);
  std::unique_ptr<ptz_tracks, TracksFree> t(new ptz_tracks());
  t->device = device_id; t->n_img = n_img; t->min_len = min_len; t->n_feat = n_feat;
  int64_t* d_sizes = nullptr;
  if (const int32_t rc = tracks_alloc(t.get(), &d_sizes)) return rc;
  const size_t np = (size_t)(n_pair > 0 ? n_pair : 1), nm = (size_t)(n_match > 0 ? n_match : 1);
  BlockLayout b;
  const size_t o_fptr = b.take(sizeof(int64_t) * ((size_t)n_img + 1)), o_ia = b.take(sizeof(int32_t) * np), o_ib = b.take(sizeof(int32_t) * np),
               o_mptr = b.take(sizeof(int64_t) * (np + 1)), o_xa = b.take(sizeof(int32_t) * nm), o_xb = b.take(sizeof(int32_t) * nm),
               o_ws = b.take((size_t)ptz_tracks_workspace_bytes(n_feat));
  CallHeld h;  // (declared after the tracks: the stream is waited for before tracks that are not returned give their block back)
  if (const int32_t rc = h.acquire(device_id, b.total())) { (void)hipGetLastError(); return rc; }
  char* d = h.base;
  PTZ_HIP_TRY(hipMemcpyAsync(d + o_fptr, feat_ptr, sizeof(int64_t) * ((size_t)n_img + 1), hipMemcpyHostToDevice, h.st));
  if (n_pair > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_ia, img_a, sizeof(int32_t) * n_pair, hipMemcpyHostToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_ib, img_b, sizeof(int32_t) * n_pair, hipMemcpyHostToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_mptr, match_ptr, sizeof(int64_t) * ((size_t)n_pair + 1), hipMemcpyHostToDevice, h.st));
  }
  if (n_match > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_xa, idx_a, sizeof(int32_t) * n_match, hipMemcpyHostToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_xb, idx_b, sizeof(int32_t) * n_match, hipMemcpyHostToDevice, h.st));
  }
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  const TrkIn a = {n_img, n_pair, min_len, n_feat, n_match, seg_max_of(n_feat), (const int64_t*)(d + o_fptr), (const int64_t*)(d + o_mptr),
                   (const int32_t*)(d + o_ia), (const int32_t*)(d + o_ib), (const int32_t*)(d + o_xa), (const int32_t*)(d + o_xb), nullptr};
  enqueue_tracks(a, d + o_ws, t->d_trk_ptr, t->d_trk_img, t->d_trk_feat, t->d_trk_node, t->d_trk_uv, d_sizes, h.st);
  if (const int32_t rc = tracks_finish(t.get(), h, d_sizes)) return rc;
  *out = t.release();
  return PTZ_OK;
}

extern "C" int32_t ptz_tracks_from_matches(const ptz_desc_set* set, const ptz_desc_matches* matches, const int32_t* img_a, const int32_t* img_b,
                                           int32_t min_len, ptz_tracks** out)
{
  using namespace ptz;
  if (!out) return PTZ_EINVAL;
  *out = nullptr;
  if (!set || !matches || min_len < 2) return PTZ_EINVAL;
  const int32_t n_pair = ptz_desc_matches_n_pairs(matches);
  const int64_t n_match = ptz_desc_matches_n_matches(matches);
  if (n_pair < 0 || n_match < 0 || (n_pair > 0 && (!img_a || !img_b))) return PTZ_EINVAL;
  for (int32_t p = 0; p < n_pair; ++p)
    if (img_a[p] < 0 || img_a[p] >= set->n_img || img_b[p] < 0 || img_b[p] >= set->n_img) return PTZ_EINVAL;
  if (set->n_feat >= ((int64_t)1 << 31) || n_match >= ((int64_t)1 << 31)) return PTZ_ELIMIT;
  const int64_t* d_mptr = nullptr;
  const int32_t *d_xa = nullptr, *d_xb = nullptr;
  if (const int32_t rc = ptz_desc_matches_device_ptrs(matches, &d_mptr, &d_xa, &d_xb, nullptr, nullptr, nullptr)) return rc;
  clear_stale_error(__func__);
  if (d_mptr) {
    int device = -1;
    if (const int32_t rc = owning_device(d_mptr, nullptr, &device)) return rc;
    if (device != set->device) return PTZ_EINVAL;
  }
  PTZ_DEVICE_GUARD(set->device);
  std::unique_ptr<ptz_tracks, TracksFree> t(new ptz_tracks());
  t->device = set->device; t->n_img = set->n_img; t->min_len = min_len; t->n_feat = set->n_feat;
  int64_t* d_sizes = nullptr;
  if (const int32_t rc = tracks_alloc(t.get(), &d_sizes)) return rc;
  const size_t np = (size_t)(n_pair > 0 ? n_pair : 1);
  BlockLayout b;
  const size_t o_ia = b.take(sizeof(int32_t) * np), o_ib = b.take(sizeof(int32_t) * np), o_ws = b.take((size_t)ptz_tracks_workspace_bytes(set->n_feat));
  CallHeld h;
  if (const int32_t rc = h.acquire(set->device, b.total())) { (void)hipGetLastError(); return rc; }
  char* d = h.base;
  if (n_pair > 0) {
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_ia, img_a, sizeof(int32_t) * n_pair, hipMemcpyHostToDevice, h.st));
    PTZ_HIP_TRY(hipMemcpyAsync(d + o_ib, img_b, sizeof(int32_t) * n_pair, hipMemcpyHostToDevice, h.st));
  }
  PTZ_HIP_TRY(hipEventRecord(h.ev[0], h.st));
  const TrkIn a = {set->n_img, n_pair, min_len, set->n_feat, d_mptr ? n_match : 0, seg_max_of(set->n_feat), set->d_feat_ptr, d_mptr,
                   (const int32_t*)(d + o_ia), (const int32_t*)(d + o_ib), d_xa, d_xb, set->d_kp};
  enqueue_tracks(a, d + o_ws, t->d_trk_ptr, t->d_trk_img, t->d_trk_feat, t->d_trk_node, t->d_trk_uv, d_sizes, h.st);
  if (const int32_t rc = tracks_finish(t.get(), h, d_sizes)) return rc;
  *out = t.release();
  return PTZ_OK;
}

extern "C" int32_t ptz_tracks_n_tracks(const ptz_tracks* t) { return t ? t->n_track : 0; }

extern "C" int64_t ptz_tracks_n_views(const ptz_tracks* t) { return t ? t->n_view : 0; }

extern "C" double ptz_tracks_device_ms(const ptz_tracks* t) { return t ? t->device_ms : 0.0; }

extern "C" int32_t ptz_tracks_counts(const ptz_tracks* t, int64_t* counts)
{
  if (!t || !counts) return PTZ_EINVAL;
  for (int k = 0; k < 4; ++k) counts[k] = t->counts[k];
  return PTZ_OK;
}

extern "C" int32_t ptz_tracks_device_ptrs(const ptz_tracks* t, const int64_t** d_trk_ptr, const int32_t** d_trk_img, const int32_t** d_trk_feat,
                                          const int32_t** d_trk_node, const float** d_trk_uv)
{
  if (!t) return PTZ_EINVAL;
  if (d_trk_ptr) *d_trk_ptr = t->d_trk_ptr;
  if (d_trk_img) *d_trk_img = t->d_trk_img;
  if (d_trk_feat) *d_trk_feat = t->d_trk_feat;
  if (d_trk_node) *d_trk_node = t->d_trk_node;
  if (d_trk_uv) *d_trk_uv = t->d_trk_uv;
  return PTZ_OK;
}

extern "C" int32_t ptz_tracks_download(const ptz_tracks* t, int64_t* trk_ptr, int32_t* trk_img, int32_t* trk_feat, int32_t* trk_node, float* trk_uv)
{
  using namespace ptz;
  if (!t) return PTZ_EINVAL;
  PTZ_DEVICE_GUARD(t->device);
  const size_t nv = (size_t)t->n_view;
  if (trk_ptr) PTZ_HIP_TRY(hipMemcpy(trk_ptr, t->d_trk_ptr, sizeof(int64_t) * ((size_t)t->n_track + 1), hipMemcpyDeviceToHost));
  if (nv == 0) return PTZ_OK;
  if (trk_img) PTZ_HIP_TRY(hipMemcpy(trk_img, t->d_trk_img, sizeof(int32_t) * nv, hipMemcpyDeviceToHost));
  if (trk_feat) PTZ_HIP_TRY(hipMemcpy(trk_feat, t->d_trk_feat, sizeof(int32_t) * nv, hipMemcpyDeviceToHost));
  if (trk_node) PTZ_HIP_TRY(hipMemcpy(trk_node, t->d_trk_node, sizeof(int32_t) * nv, hipMemcpyDeviceToHost));
  if (trk_uv) PTZ_HIP_TRY(hipMemcpy(trk_uv, t->d_trk_uv, sizeof(float) * 2 * nv, hipMemcpyDeviceToHost));
  return PTZ_OK;
}
